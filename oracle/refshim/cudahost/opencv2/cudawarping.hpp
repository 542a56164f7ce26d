/* oracle/refshim/cudahost: cuda::resize and cuda::remap as cudawarping.hpp declares them.  Both are DEFINED by the reference's own
 * cudawarping/src/resize.cpp and remap.cpp, compiled verbatim by oracle/Makefile.ref; the device::resize<T> / remap_gpu<T> they call
 * are in oracle/refshim/cudavec/btvl1_cu_host.cpp (the reference's kernels and launch wrappers, extracted).  TEST INFRASTRUCTURE. */
#ifndef ORACLE_CUDAHOST_CUDAWARPING_HPP
#define ORACLE_CUDAHOST_CUDAWARPING_HPP
#include "opencv2/core/cuda.hpp"
namespace cv { namespace cuda {
void resize(InputArray src, OutputArray dst, Size dsize, double fx = 0, double fy = 0, int interpolation = INTER_LINEAR, Stream &stream = Stream::Null());
void remap(InputArray src, OutputArray dst, InputArray xmap, InputArray ymap, int interpolation, int borderMode = BORDER_CONSTANT,
           Scalar borderValue = Scalar(), Stream &stream = Stream::Null());
// cudawarping.hpp: pyrDown(src, dst, stream); host glue cudawarping/src/pyramids.cpp (dst = ((rows + 1) / 2, (cols + 1) / 2)), kernel = the
// reference's pyrDown of libref_cu.so
void pyrDown(InputArray src, OutputArray dst, Stream &stream);
}}
#endif
