/* tools/orb_ref/orb_ref_filters.cpp -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.
 * C entry points over the two separable-filter kernels cv::cuda::ORB's blur runs (createGaussianFilter(CV_8UC1, -1, 7 x 7, 2, 2,
 * BORDER_REFLECT_101), orb.cpp:570): filter::linearRow<uchar, float> (cudafilters/src/cuda/row_filter.8uc1.cu) into an f32 buffer and
 * filter::linearColumn<float, uchar> (column_filter.8uc1.cu) out of it, as SeparableLinearFilter::apply calls them
 * (cudafilters/src/filtering.cpp).  The taps arrive from the caller: getGaussianKernel is a main-repository function. */
#include <vector>
#include "opencv2/core/cuda/common.hpp"

namespace filter {
template <typename T, typename D>
void linearRow(cv::cuda::PtrStepSzb src, cv::cuda::PtrStepSzb dst, const float *kernel, int ksize, int anchor, int brd_type, int cc, cudaStream_t stream);
template <typename T, typename D>
void linearColumn(cv::cuda::PtrStepSzb src, cv::cuda::PtrStepSzb dst, const float *kernel, int ksize, int anchor, int brd_type, int cc, cudaStream_t stream);
}

extern "C" void orb_ref_blur(const unsigned char *src, int rows, int cols, const float *taps, int ksize, unsigned char *dst, float *rowbuf)
{
    using cv::cuda::PtrStepSzb;
    const int BORDER_REFLECT_101 = 4;   /* main repository, core/base.hpp */
    PtrStepSzb s(rows, cols, (unsigned char *)src, (size_t)cols), b(rows, cols, (unsigned char *)rowbuf, (size_t)cols * 4),
        d(rows, cols, dst, (size_t)cols);
    filter::linearRow<unsigned char, float>(s, b, taps, ksize, ksize / 2, BORDER_REFLECT_101, 30, 0);
    filter::linearColumn<float, unsigned char>(b, d, taps, ksize, ksize / 2, BORDER_REFLECT_101, 30, 0);
}
