/* oracle/refshim/cudahost: of opencv2/cudafilters.hpp the Filter interface and the two factories BTVL1_CUDA reaches
 * (superres/src/btv_l1_cuda.cpp:324); both factories are the reference's own text (the slice of cudafilters/src/filtering.cpp that
 * oracle/Makefile.ref compiles).  TEST INFRASTRUCTURE. */
#ifndef ORACLE_CUDAHOST_CUDAFILTERS_HPP
#define ORACLE_CUDAHOST_CUDAFILTERS_HPP
#include "opencv2/core/cuda.hpp"
namespace cv { namespace cuda {
class Filter : public Algorithm {
public:
    virtual void apply(InputArray src, OutputArray dst, Stream &stream = Stream::Null()) = 0;
};
Ptr<Filter> createSeparableLinearFilter(int srcType, int dstType, InputArray rowKernel, InputArray columnKernel, Point anchor = Point(-1, -1),
                                        int rowBorderMode = BORDER_DEFAULT, int columnBorderMode = -1);
Ptr<Filter> createGaussianFilter(int srcType, int dstType, Size ksize, double sigma1, double sigma2 = 0, int rowBorderMode = BORDER_DEFAULT,
                                 int columnBorderMode = -1);
}}
#endif
