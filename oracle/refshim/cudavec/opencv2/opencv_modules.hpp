/* oracle/refshim/cudavec: opencv2/opencv_modules.hpp of a build with cudaarithm, cudawarping and cudafilters (superres/src/cuda/btv_l1_gpu.cu:45
 * compiles its body only then).  TEST INFRASTRUCTURE. */
#ifndef ORACLE_CUDASHIM_OPENCV_MODULES_HPP
#define ORACLE_CUDASHIM_OPENCV_MODULES_HPP
#define HAVE_OPENCV_CUDAARITHM
#define HAVE_OPENCV_CUDAWARPING
#define HAVE_OPENCV_CUDAFILTERS
#endif
