/* oracle/refshim/cudahost: opencv2/video/tracking.hpp (superres/src/precomp.hpp includes it; nothing of it is used).  TEST INFRASTRUCTURE. */
#include "opencv2/video.hpp"
