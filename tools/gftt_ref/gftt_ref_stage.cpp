/* tools/gftt_ref/gftt_ref_stage.cpp -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.
 * C entry points over the reference's own code for cv::cuda::CornernessCriteria / CornersDetector, compiled for the host by
 * tools/make_golden_gftt.py:
 *   filter::linearRow<uchar | float, float> and filter::linearColumn<float, float> (cudafilters/src/cuda/row_filter.*.cu,
 *   column_filter.32fc1.cu) as SeparableLinearFilter::apply calls them (cudafilters/src/filtering.cpp:458-505);
 *   cornerHarris_gpu / cornerMinEigenVal_gpu (cudaimgproc/src/cuda/corners.cu) and findCorners_gpu / sortCorners_gpu (cuda/gftt.cu);
 *   SLICES of cudaimgproc/src/corners.cpp (the scale, :93-101) and src/gftt.cpp (the capacity and the threshold with the call of
 *   findCorners_gpu, :122-124; the grid loop of minDistance, :147-207), #included below between the names they use.
 * Written here and not by the reference: the maximum of the plane (cuda::minMax is a cudaarithm kernel that is not built), the branch
 * on minDistance < 1 with the copy of the head (gftt.cpp:134-137, GpuMat calls), cvRound (main repository: lrint). */
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>
#include "opencv2/core/cuda/common.hpp"
#include "opencv2/core/cuda/utility.hpp"

using cv::cuda::PtrStepSzb;
using cv::cuda::PtrStepSzf;

namespace filter {
template <typename T, typename D>
void linearRow(PtrStepSzb src, PtrStepSzb dst, const float *kernel, int ksize, int anchor, int brd_type, int cc, cudaStream_t stream);
template <typename T, typename D>
void linearColumn(PtrStepSzb src, PtrStepSzb dst, const float *kernel, int ksize, int anchor, int brd_type, int cc, cudaStream_t stream);
}
namespace cv { namespace cuda { namespace device {
namespace imgproc {
void cornerHarris_gpu(int block_size, float k, PtrStepSzf Dx, PtrStepSzf Dy, PtrStepSzf dst, int border_type, cudaStream_t stream);
void cornerMinEigenVal_gpu(int block_size, PtrStepSzf Dx, PtrStepSzf Dy, PtrStepSzf dst, int border_type, cudaStream_t stream);
}
namespace gfft {
int findCorners_gpu(const PtrStepSzf eig, float threshold, PtrStepSzb mask, float2 *corners, int max_count, int *counterPtr, cudaStream_t stream);
void sortCorners_gpu(const PtrStepSzf eig, float2 *corners, int count, cudaStream_t stream);
}
}}}

static PtrStepSzf plane(const float *p, int rows, int cols) { return PtrStepSzf(rows, cols, (float *)p, (size_t)cols * 4); }

/* corners.cpp:93-101 */
extern "C" double gftt_ref_scale(int ksize_, int blockSize_, int is_8u)
{
    const int CV_8U = 0;
    const int sdepth = is_8u ? CV_8U : 5;
#include "corners_scale.gen.inc"
    return scale;
}

/* src: rows x cols of uchar or float with `step` bytes a row; rowbuf, dst: dense float planes */
extern "C" void gftt_ref_sobel(const void *src, size_t step, int rows, int cols, int is_f32, const float *row_taps, const float *col_taps,
                               int border, float *rowbuf, float *dst)
{
    PtrStepSzb s(rows, cols, (unsigned char *)src, step), b(rows, cols, (unsigned char *)rowbuf, (size_t)cols * 4),
        d(rows, cols, (unsigned char *)dst, (size_t)cols * 4);
    if (is_f32) filter::linearRow<float, float>(s, b, row_taps, 3, 1, border, 30, 0);
    else filter::linearRow<unsigned char, float>(s, b, row_taps, 3, 1, border, 30, 0);
    filter::linearColumn<float, float>(b, d, col_taps, 3, 1, border, 30, 0);
}

extern "C" void gftt_ref_corner(const float *dx, const float *dy, int rows, int cols, int block_size, int border, int harris, float k, float *dst)
{
    using namespace cv::cuda::device::imgproc;
    if (harris) cornerHarris_gpu(block_size, k, plane(dx, rows, cols), plane(dy, rows, cols), plane(dst, rows, cols), border, 0);
    else cornerMinEigenVal_gpu(block_size, plane(dx, rows, cols), plane(dy, rows, cols), plane(dst, rows, cols), border, 0);
}

extern "C" void gftt_ref_sort(const float *eig, int rows, int cols, float *corners, int count)
{
    cv::cuda::device::gfft::sortCorners_gpu(plane(eig, rows, cols), (float2 *)corners, count, 0);
}

namespace {
int cvRound(double v) { return (int)lrint(v); }
struct Point2f { float x, y; };
struct SizeGlue { int w, h; int area() const { return w * h; } };
struct ImageGlue { int rows, cols; SizeGlue size() const { return {cols, rows}; } };
struct TmpCorners {
    std::vector<float2> v;
    int cols = 0;
    template <class T> T *ptr() { return (T *)v.data(); }
};
const int CV_32FC2 = 13;
void ensureSizeIsEnough(int, int cols, int, TmpCorners &t) { t.v.resize(cols); t.cols = cols; }
}

/* GoodFeaturesToTrackDetector::detect from the response plane on, gftt.cpp:119-213.  candidates, sorted, out: room for
 * max(1000, (int)(area * 0.05)) float2 each.  -> the number of corners in out */
extern "C" int gftt_ref_detect_tail(const float *eig, int rows, int cols, const unsigned char *mask_data, double qualityLevel_, double minDistance_,
                                    int maxCorners_, float *threshold, int *capacity, float *candidates, int *total_out, float *sorted, float *out)
{
    using namespace cv::cuda::device::gfft;
    const ImageGlue image = {rows, cols};
    const PtrStepSzf eig_ = plane(eig, rows, cols);
    const PtrStepSzb mask(rows, cols, (unsigned char *)mask_data, (size_t)cols);
    double maxVal = eig[0];   /* cuda::minMax(eig_, 0, &maxVal) */
    for (long long i = 1; i < (long long)rows * cols; ++i) maxVal = eig[i] > maxVal ? eig[i] : maxVal;
    cudaStream_t stream_ = 0;
    TmpCorners tmpCorners_;
    int counter = 0, *counterPtr_ = &counter;
    float seen_threshold = 0;
    /* the slice calls findCorners_gpu(eig_, static_cast<float>(maxVal * qualityLevel_), ...): this one records the threshold on the way */
    auto findCorners_gpu = [&](const PtrStepSzf e, float th, PtrStepSzb m, float2 *c, int max_count, int *ctr, cudaStream_t st) {
        seen_threshold = th;
        return cv::cuda::device::gfft::findCorners_gpu(e, th, m, c, max_count, ctr, st);
    };
#include "gftt_capacity.gen.inc"
    *threshold = seen_threshold;
    *capacity = tmpCorners_.cols;
    *total_out = total;
    std::memcpy(candidates, tmpCorners_.v.data(), (size_t)total * sizeof(float2));
    if (total == 0) return 0;
    sortCorners_gpu(eig_, tmpCorners_.ptr<float2>(), total, stream_);
    std::memcpy(sorted, tmpCorners_.v.data(), (size_t)total * sizeof(float2));
    if (minDistance_ < 1) {   /* gftt.cpp:134-137 */
        const int n = maxCorners_ > 0 ? std::min(maxCorners_, total) : total;
        std::memcpy(out, tmpCorners_.v.data(), (size_t)n * sizeof(float2));
        return n;
    }
    std::vector<Point2f> tmp(total), tmp2;
    std::memcpy(tmp.data(), tmpCorners_.v.data(), (size_t)total * sizeof(float2));
    tmp2.reserve(total);
#include "gftt_grid.gen.inc"
    std::memcpy(out, tmp2.data(), tmp2.size() * sizeof(Point2f));
    return (int)tmp2.size();
}
