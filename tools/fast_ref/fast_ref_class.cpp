/* tools/fast_ref/fast_ref_class.cpp -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.
 * C entry points over the reference's host class cv::cuda::FastFeatureDetector: modules/cudafeatures2d/src/fast.cpp and
 * feature2d_async.cpp are compiled as they lie into their own objects; this file drives the class through its public interface (create,
 * setThreshold, setMaxNumPoints, getMaxNumPoints, detectAsync, detect, convert). */
#include <cstring>
#include "opencv2/cudafeatures2d.hpp"
#include "opencv2/core/private.cuda.hpp"

using cv::cuda::GpuMat;

/* the one member of the stub's GpuMat that FAST_Impl::convert reaches through InputArray::getGpuMat (fast.cpp:186); the stub defines it in
 * oracle/refshim/cudahost/cudahost.cpp, which is not linked here */
void cv::cuda::GpuMatStub::download(cv::MatStub &dst) const
{
    dst.create(rows, cols, type());
    for (int y = 0; y < rows; ++y) memcpy(dst.ptr<unsigned char>(y), ptr<unsigned char>(y), (size_t)cols * cv::elem_size_of(type()));
}

namespace {
GpuMat up(const unsigned char *p, int rows, int cols)
{
    GpuMat m(rows, cols, CV_8UC1);
    for (int y = 0; y < rows; ++y) memcpy(m.ptr(y), p + (size_t)y * cols, (size_t)cols);
    return m;
}
}  // namespace

extern "C" {
/* img, mask (or null): dense rows x cols bytes.  out: 2 x max_npoints elements of 4 bytes, receives the 2 x n matrix of detectAsync densely
 * (row 1 behind row 0 at n elements); kp: 5 floats per keypoint (x, y, size, angle, response) of convert(), room for max_npoints.
 * -> n of detectAsync, -1 if the class threw, -2 if detect() has another number of keypoints than detectAsync + convert. */
int fast_ref_detect(const unsigned char *img, const unsigned char *mask, int rows, int cols, int threshold, int nms, int max_npoints, void *out,
                    float *kp, int *max_npoints_after)
{
    try {
        /* created with other values, then set: the setters are part of what is recorded */
        cv::Ptr<cv::cuda::FastFeatureDetector> f = cv::cuda::FastFeatureDetector::create(threshold + 1, nms != 0, cv::FastFeatureDetector::TYPE_9_16,
                                                                                         max_npoints + 1);
        f->setThreshold(threshold);
        f->setMaxNumPoints(max_npoints);
        *max_npoints_after = f->getMaxNumPoints();
        GpuMat d_img = rows > 0 && cols > 0 ? up(img, rows, cols) : GpuMat();
        GpuMat d_mask = mask ? up(mask, rows, cols) : GpuMat();
        GpuMat d_kp;
        cv::cuda::Stream st;
        f->detectAsync(d_img, cv::_OutputArray(d_kp), d_mask, st);
        const int n = d_kp.empty() ? 0 : d_kp.cols;
        for (int r = 0; r < 2 && n; ++r) memcpy((unsigned char *)out + (size_t)r * n * 4, d_kp.ptr(r), (size_t)n * 4);
        std::vector<cv::KeyPoint> a, b;
        f->convert(d_kp, a);
        f->detect(d_img, b, d_mask);
        if ((int)a.size() != n || a.size() != b.size()) return -2;
        for (int i = 0; i < n; ++i) {
            kp[5 * i] = a[i].pt.x; kp[5 * i + 1] = a[i].pt.y; kp[5 * i + 2] = a[i].size; kp[5 * i + 3] = a[i].angle; kp[5 * i + 4] = a[i].response;
        }
        return n;
    } catch (const std::exception &) { return -1; }
}
/* 1 if create(type) returned, 0 if it threw */
int fast_ref_create_accepts_type(int type)
{
    try { cv::cuda::FastFeatureDetector::create(10, true, type, 5000); return 1; } catch (const std::exception &) { return 0; }
}
}
