// cv::cuda::CornernessCriteria and cv::cuda::CornersDetector over libmiflow: the producer of the points
// cv::cuda::SparsePyrLKOpticalFlow tracks (cudaoptflow/test/test_optflow.cpp:203, videostab/src/global_motion.cpp:796).
// Interface of modules/cudaimgproc/include/opencv2/cudaimgproc.hpp:535-618: createHarrisCorner, createMinEigenValCorner,
// createGoodFeaturesToTrackDetector with their defaults.  The work is mi_corner_compute / mi_gftt_detect (include/miflow/c_api.h).
// ksize: 3 only (cv::Error::StsNotImplemented otherwise; c_api.h says why).  The rest of cudaimgproc is not here.
#ifndef OPENCV_CUDAIMGPROC_MIFLOW_HPP
#define OPENCV_CUDAIMGPROC_MIFLOW_HPP

#include <algorithm>
#include "opencv2/core/cuda.hpp"

namespace cv {

#if !defined(MIFLOW_WITH_OPENCV) && !defined(MIFLOW_HAVE_BORDER_TYPES)
#define MIFLOW_HAVE_BORDER_TYPES
enum BorderTypes { BORDER_CONSTANT = 0, BORDER_REPLICATE = 1, BORDER_REFLECT = 2, BORDER_WRAP = 3, BORDER_REFLECT_101 = 4, BORDER_TRANSPARENT = 5,
                   BORDER_REFLECT101 = BORDER_REFLECT_101, BORDER_DEFAULT = BORDER_REFLECT_101, BORDER_ISOLATED = 16 };   // opencv2/core/base.hpp
#endif

namespace cuda {

/** cudaimgproc.hpp:538-549 */
class CV_EXPORTS_W CornernessCriteria : public Algorithm {
public:
    /** dst: CV_32FC1 of src's size */
    CV_WRAP virtual void compute(InputArray src, OutputArray dst, Stream &stream = Stream::Null()) = 0;
};

/** cudaimgproc.hpp:581-597 */
class CV_EXPORTS_W CornersDetector : public Algorithm {
public:
    /** corners: 1 x N CV_32FC2 {x, y}, strongest first; released when nothing is found */
    CV_WRAP virtual void detect(InputArray image, OutputArray corners, InputArray mask = GpuMat(), Stream &stream = Stream::Null()) = 0;
    CV_WRAP virtual void setMaxCorners(int maxCorners) = 0;
    CV_WRAP virtual void setMinDistance(double minDistance) = 0;
};

namespace miflow_detail {

class CornerImpl final : public CornernessCriteria {
public:
    explicit CornerImpl(const mi_corner_params &p) : h_(p) {}
    void compute(InputArray src, OutputArray dst, Stream &stream) override
    {
        dst.create(src.size(), CV_32FC1);   // corners.cpp:144,172
        mi_mat s = miMat(src), d = miMat(dst);
        miCheck(mi_corner_compute(h_.get(), &s, &d, stream.hipStream()));
    }
private:
    ParamHandle<mi_corner, mi_corner_params, mi_corner_create, nullptr, mi_corner_destroy> h_;   // no setter
};

class GfttImpl final : public CornersDetector {
public:
    explicit GfttImpl(const mi_gftt_params &p) : h_(p) {}
    void detect(InputArray image, OutputArray corners, InputArray mask, Stream &stream) override
    {
        CV_Assert(mask.empty() || (mask.type() == CV_8UC1 && mask.size() == image.size()));   // gftt.cpp:114
        CV_Assert(!image.empty());
        const int capacity = std::max(1000, static_cast<int>(image.size().area() * 0.05));   // gftt.cpp:122
        GpuMat out(1, h_.params().max_corners > 0 ? std::min(h_.params().max_corners, capacity) : capacity, CV_32FC2);
        mi_mat i = miMat(image), m = miMat(mask), o = miMat(out);
        int n = 0;
        miCheck(mi_gftt_detect(h_.get(), &i, mask.empty() ? nullptr : &m, &o, &n, stream.hipStream()));
        if (n == 0) { corners.release(); return; }   // gftt.cpp:126-130
        corners = out(Rect(0, 0, n, 1));
    }
    void setMaxCorners(int maxCorners) override { h_.set([=](auto &q) { q.max_corners = maxCorners; }); }
    void setMinDistance(double minDistance) override { h_.set([=](auto &q) { q.min_distance = minDistance; }); }
private:
    ParamHandle<mi_gftt, mi_gftt_params, mi_gftt_create, mi_gftt_set_params, mi_gftt_destroy> h_;
};

inline Ptr<CornernessCriteria> makeCorner(int srcType, int blockSize, int ksize, int borderType, bool harris, double k)
{
    mi_corner_params p;
    p.type = srcType; p.block_size = blockSize; p.ksize = ksize; p.border_type = borderType; p.harris = harris ? 1 : 0; p.k = k;
    return makePtr<CornerImpl>(p);
}

}  // namespace miflow_detail

/** cudaimgproc.hpp:562 */
inline Ptr<CornernessCriteria> createHarrisCorner(int srcType, int blockSize, int ksize, double k, int borderType = BORDER_REFLECT101)
{
    return miflow_detail::makeCorner(srcType, blockSize, ksize, borderType, true, k);
}

/** cudaimgproc.hpp:575 */
inline Ptr<CornernessCriteria> createMinEigenValCorner(int srcType, int blockSize, int ksize, int borderType = BORDER_REFLECT101)
{
    return miflow_detail::makeCorner(srcType, blockSize, ksize, borderType, false, 0.0);
}

/** cudaimgproc.hpp:617-618 */
inline Ptr<CornersDetector> createGoodFeaturesToTrackDetector(int srcType, int maxCorners = 1000, double qualityLevel = 0.01, double minDistance = 0.0,
                                                              int blockSize = 3, bool useHarrisDetector = false, double harrisK = 0.04)
{
    mi_gftt_params p;
    p.type = srcType; p.max_corners = maxCorners; p.quality_level = qualityLevel; p.min_distance = minDistance;
    p.block_size = blockSize; p.use_harris = useHarrisDetector ? 1 : 0; p.harris_k = harrisK;
    return makePtr<miflow_detail::GfttImpl>(p);
}

}  // namespace cuda
}  // namespace cv

#endif
