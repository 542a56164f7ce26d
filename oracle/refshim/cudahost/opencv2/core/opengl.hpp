/* oracle/refshim/cudahost: nothing of opencv2/core/opengl.hpp is used by superres/src/btv_l1_cuda.cpp.  TEST INFRASTRUCTURE. */
