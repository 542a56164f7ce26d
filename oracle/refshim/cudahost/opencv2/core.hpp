/* oracle/refshim/cudahost: opencv2/core.hpp as the superres headers include it -- the stub core.  TEST INFRASTRUCTURE. */
#include "opencv2/core/cuda.hpp"
