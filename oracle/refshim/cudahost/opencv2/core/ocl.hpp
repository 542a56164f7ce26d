/* oracle/refshim/cudahost: of opencv2/core/ocl.hpp only useOpenCL(), which superres/src/super_resolution.cpp asks; nothing is used by
 * xfeatures2d/src/surf.cuda.cpp.  TEST INFRASTRUCTURE. */
#ifndef ORACLE_CUDAHOST_OCL_HPP
#define ORACLE_CUDAHOST_OCL_HPP
namespace cv { namespace ocl { inline bool useOpenCL() { return false; } } }
#endif
