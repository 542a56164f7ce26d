// cv::cuda::DescriptorMatcher (brute force, NORM_L1 / NORM_L2, float descriptors) over libmiflow.
// Interface of modules/cudafeatures2d/include/opencv2/cudafeatures2d.hpp:75-372: createBFMatcher, the train collection,
// match / knnMatch / radiusMatch, their *Async forms (the reference's packed device matrices, brute_force_matcher.cpp:314-980)
// and *Convert unpackers (:440-495, 727-812, 982-1063).  The matching itself is mi_bf_knn_match / mi_bf_radius_match
// (include/miflow/c_api.h), which write straight into the rows of the packed matrix.
#ifndef OPENCV_CUDAFEATURES2D_MIFLOW_HPP
#define OPENCV_CUDAFEATURES2D_MIFLOW_HPP

#include <algorithm>
#include <vector>
#include "opencv2/core/cuda.hpp"
#include "opencv2/core/types.hpp"   // KeyPoint, shared with xfeatures2d/cuda.hpp

namespace cv {

#ifndef MIFLOW_HAVE_DMATCH
#define MIFLOW_HAVE_DMATCH
/** opencv2/core/types.hpp DMatch */
struct DMatch {
    DMatch() : queryIdx(-1), trainIdx(-1), imgIdx(-1), distance(3.402823466e+38f) {}
    DMatch(int q, int t, float d) : queryIdx(q), trainIdx(t), imgIdx(-1), distance(d) {}
    DMatch(int q, int t, int i, float d) : queryIdx(q), trainIdx(t), imgIdx(i), distance(d) {}
    int queryIdx, trainIdx, imgIdx;
    float distance;
    bool operator<(const DMatch &m) const { return distance < m.distance; }
};
#endif
#ifndef MIFLOW_HAVE_NORM_TYPES
#define MIFLOW_HAVE_NORM_TYPES
enum NormTypes { NORM_INF = 1, NORM_L1 = 2, NORM_L2 = 4, NORM_HAMMING = 6 };   // opencv2/core/base.hpp
#endif

namespace cuda {

class CV_EXPORTS_W DescriptorMatcher : public cv::Algorithm {
public:
    static Ptr<DescriptorMatcher> createBFMatcher(int normType = 4 /* cv::NORM_L2 */);
    virtual bool isMaskSupported() const = 0;
    virtual void add(const std::vector<GpuMat> &descriptors) = 0;
    virtual const std::vector<GpuMat> &getTrainDescriptors() const = 0;
    virtual void train() = 0;

    /** queries without an allowed candidate are skipped, like the reference's matchConvert */
    virtual void match(InputArray queryDescriptors, InputArray trainDescriptors, std::vector<DMatch> &matches,
                       InputArray mask = GpuMat()) = 0;
    virtual void match(InputArray queryDescriptors, std::vector<DMatch> &matches,
                       const std::vector<GpuMat> &masks = std::vector<GpuMat>()) = 0;
    virtual void matchAsync(InputArray queryDescriptors, InputArray trainDescriptors, OutputArray matches, InputArray mask = GpuMat(),
                            Stream &stream = Stream::Null()) = 0;
    virtual void matchAsync(InputArray queryDescriptors, OutputArray matches, const std::vector<GpuMat> &masks = std::vector<GpuMat>(),
                            Stream &stream = Stream::Null()) = 0;
    virtual void matchConvert(InputArray gpu_matches, std::vector<DMatch> &matches) = 0;

    virtual void knnMatch(InputArray queryDescriptors, InputArray trainDescriptors, std::vector<std::vector<DMatch> > &matches, int k,
                          InputArray mask = GpuMat(), bool compactResult = false) = 0;
    virtual void knnMatch(InputArray queryDescriptors, std::vector<std::vector<DMatch> > &matches, int k,
                          const std::vector<GpuMat> &masks = std::vector<GpuMat>(), bool compactResult = false) = 0;
    virtual void knnMatchAsync(InputArray queryDescriptors, InputArray trainDescriptors, OutputArray matches, int k,
                               InputArray mask = GpuMat(), Stream &stream = Stream::Null()) = 0;
    virtual void knnMatchAsync(InputArray queryDescriptors, OutputArray matches, int k,
                               const std::vector<GpuMat> &masks = std::vector<GpuMat>(), Stream &stream = Stream::Null()) = 0;
    virtual void knnMatchConvert(InputArray gpu_matches, std::vector<std::vector<DMatch> > &matches, bool compactResult = false) = 0;

    virtual void radiusMatch(InputArray queryDescriptors, InputArray trainDescriptors, std::vector<std::vector<DMatch> > &matches,
                             float maxDistance, InputArray mask = GpuMat(), bool compactResult = false) = 0;
    virtual void radiusMatch(InputArray queryDescriptors, std::vector<std::vector<DMatch> > &matches, float maxDistance,
                             const std::vector<GpuMat> &masks = std::vector<GpuMat>(), bool compactResult = false) = 0;
    virtual void radiusMatchAsync(InputArray queryDescriptors, InputArray trainDescriptors, OutputArray matches, float maxDistance,
                                  InputArray mask = GpuMat(), Stream &stream = Stream::Null()) = 0;
    virtual void radiusMatchAsync(InputArray queryDescriptors, OutputArray matches, float maxDistance,
                                  const std::vector<GpuMat> &masks = std::vector<GpuMat>(), Stream &stream = Stream::Null()) = 0;
    virtual void radiusMatchConvert(InputArray gpu_matches, std::vector<std::vector<DMatch> > &matches, bool compactResult = false) = 0;
};

namespace miflow_detail {

// rows [r0, r0 + n) of a packed CV_32S matrix seen as an n x c matrix of `type`
inline mi_mat packedRows(GpuMat &m, int r0, int n, int c, int type)
{
    mi_mat r;
    r.data = m.ptr<uchar>(r0); r.step = m.step; r.rows = n; r.cols = c; r.type = type;
    return r;
}
// one packed row of nq entries with cn channels, seen as the nq x cn matrix the C-ABI fills
inline mi_mat packedRow(GpuMat &m, int row, int nq, int cn, int type)
{
    mi_mat r;
    r.data = m.ptr<uchar>(row); r.step = (size_t)cn * 4; r.rows = nq; r.cols = cn; r.type = type;
    return r;
}

class BFMatcherImpl final : public DescriptorMatcher {
public:
    explicit BFMatcherImpl(int normType) : h_(normType, [](const int *norm, mi_bfmatcher **h) { return mi_bf_create(*norm, h); }) {}

    bool isMaskSupported() const override { return true; }
    void add(const std::vector<GpuMat> &descriptors) override { coll_.insert(coll_.end(), descriptors.begin(), descriptors.end()); }
    const std::vector<GpuMat> &getTrainDescriptors() const override { return coll_; }
    void clear() override { coll_.clear(); }
    bool empty() const override { return coll_.empty(); }
    void train() override {}

    // ------------------------------------------------------------------ match
    void match(InputArray query, InputArray train, std::vector<DMatch> &matches, InputArray mask) override
    {
        GpuMat g;
        matchAsync(query, train, g, mask, Stream::Null());
        matchConvert(g, matches);
    }
    void match(InputArray query, std::vector<DMatch> &matches, const std::vector<GpuMat> &masks) override
    {
        GpuMat g;
        matchAsync(query, g, masks, Stream::Null());
        matchConvert(g, matches);
    }
    void matchAsync(InputArray query, InputArray train, OutputArray matches, InputArray mask, Stream &stream) override
    {
        if (query.empty() || train.empty()) { matches.release(); return; }
        const int nq = query.rows;
        matches.create(2, nq, CV_32SC1);                                   // {trainIdx; distance}, brute_force_matcher.cpp:367-372
        mi_mat q = miMat(query), t = miMat(train), m = miMat(mask);
        mi_mat i = packedRow(matches, 0, nq, 1, CV_32SC1), d = packedRow(matches, 1, nq, 1, CV_32FC1);
        miCheck(mi_bf_knn_match(h_.get(), &q, &t, mask.empty() ? nullptr : &m, 1, 1, &i, nullptr, &d, stream.hipStream()));
    }
    void matchAsync(InputArray query, OutputArray matches, const std::vector<GpuMat> &masks, Stream &stream) override
    {
        if (query.empty() || coll_.empty()) { matches.release(); return; }
        const int nq = query.rows;
        matches.create(3, nq, CV_32SC1);                                   // {trainIdx; imgIdx; distance}, :429-435
        std::vector<mi_mat> ts, ms;
        collection(masks, ts, ms);
        mi_mat q = miMat(query);
        mi_mat i = packedRow(matches, 0, nq, 1, CV_32SC1), g = packedRow(matches, 1, nq, 1, CV_32SC1), d = packedRow(matches, 2, nq, 1, CV_32FC1);
        miCheck(mi_bf_knn_match(h_.get(), &q, ts.data(), ms.empty() ? nullptr : ms.data(), (int)ts.size(), 1, &i, &g, &d, stream.hipStream()));
    }
    void matchConvert(InputArray gpu_matches, std::vector<DMatch> &matches) override
    {
        matches.clear();
        if (gpu_matches.empty()) return;
        CV_Assert(gpu_matches.type() == CV_32SC1 && (gpu_matches.rows == 2 || gpu_matches.rows == 3));
        const int nq = gpu_matches.cols, nr = gpu_matches.rows;
        std::vector<int> h((size_t)nr * nq);
        gpu_matches.download(h.data(), sizeof(int) * nq);
        const int *idx = h.data(), *img = nr == 3 ? h.data() + nq : nullptr;
        const float *dist = reinterpret_cast<const float *>(h.data() + (size_t)(nr - 1) * nq);
        for (int q = 0; q < nq; ++q)
            if (idx[q] != -1) matches.push_back(DMatch(q, idx[q], img ? img[q] : 0, dist[q]));
    }

    // ------------------------------------------------------------------ knnMatch
    void knnMatch(InputArray query, InputArray train, std::vector<std::vector<DMatch> > &matches, int k, InputArray mask,
                  bool compactResult) override
    {
        GpuMat g;
        knnMatchAsync(query, train, g, k, mask, Stream::Null());
        knnMatchConvert(g, matches, compactResult);
    }
    void knnMatch(InputArray query, std::vector<std::vector<DMatch> > &matches, int k, const std::vector<GpuMat> &masks,
                  bool compactResult) override
    {
        if (k == 2) {
            GpuMat g;
            knnMatchAsync(query, g, k, masks, Stream::Null());
            knnMatchConvert(g, matches, compactResult);
            return;
        }
        // the reference merges per-image lists on the host (:527-571); the C-ABI searches the whole collection in one pass
        matches.clear();
        if (query.empty() || coll_.empty()) return;
        const int nq = query.rows;
        GpuMat g(3 * nq, k, CV_32SC1);
        std::vector<mi_mat> ts, ms;
        collection(masks, ts, ms);
        mi_mat q = miMat(query);
        mi_mat i = packedRows(g, 0, nq, k, CV_32SC1), im = packedRows(g, nq, nq, k, CV_32SC1), d = packedRows(g, 2 * nq, nq, k, CV_32FC1);
        miCheck(mi_bf_knn_match(h_.get(), &q, ts.data(), ms.empty() ? nullptr : ms.data(), (int)ts.size(), k, &i, &im, &d, nullptr));
        std::vector<int> h((size_t)3 * nq * k);
        g.download(h.data(), sizeof(int) * k);
        unpackLists(h.data(), h.data() + (size_t)nq * k, reinterpret_cast<const float *>(h.data() + (size_t)2 * nq * k), nq, k, k, nullptr,
                    compactResult, false, matches);
    }
    void knnMatchAsync(InputArray query, InputArray train, OutputArray matches, int k, InputArray mask, Stream &stream) override
    {
        if (query.empty() || train.empty()) { matches.release(); return; }
        const int nq = query.rows;
        mi_mat q = miMat(query), t = miMat(train), m = miMat(mask), i, d;
        if (k == 2) {
            matches.create(2, nq, CV_MAKETYPE(CV_32S, 2));                 // :619-626
            i = packedRow(matches, 0, nq, 2, CV_32SC1); d = packedRow(matches, 1, nq, 2, CV_32FC1);
        } else {
            matches.create(2 * nq, k, CV_32SC1);                           // :630-636 (no allDist buffer is needed here)
            i = packedRows(matches, 0, nq, k, CV_32SC1); d = packedRows(matches, nq, nq, k, CV_32FC1);
        }
        miCheck(mi_bf_knn_match(h_.get(), &q, &t, mask.empty() ? nullptr : &m, 1, k, &i, nullptr, &d, stream.hipStream()));
    }
    void knnMatchAsync(InputArray query, OutputArray matches, int k, const std::vector<GpuMat> &masks, Stream &stream) override
    {
        if (k != 2) CV_Error(Error::StsNotImplemented, "only k=2 mode is supported for now");   // :664-667
        if (query.empty() || coll_.empty()) { matches.release(); return; }
        const int nq = query.rows;
        matches.create(3, nq, CV_MAKETYPE(CV_32S, 2));                     // {trainIdx; imgIdx; distance} pairs
        std::vector<mi_mat> ts, ms;
        collection(masks, ts, ms);
        mi_mat q = miMat(query);
        mi_mat i = packedRow(matches, 0, nq, 2, CV_32SC1), g = packedRow(matches, 1, nq, 2, CV_32SC1), d = packedRow(matches, 2, nq, 2, CV_32FC1);
        miCheck(mi_bf_knn_match(h_.get(), &q, ts.data(), ms.empty() ? nullptr : ms.data(), (int)ts.size(), 2, &i, &g, &d, stream.hipStream()));
    }
    void knnMatchConvert(InputArray gpu_matches, std::vector<std::vector<DMatch> > &matches, bool compactResult) override
    {
        matches.clear();
        if (gpu_matches.empty()) return;
        const bool pairs = gpu_matches.type() == CV_MAKETYPE(CV_32S, 2);
        CV_Assert((pairs && (gpu_matches.rows == 2 || gpu_matches.rows == 3)) || gpu_matches.type() == CV_32SC1);
        const int cn = pairs ? 2 : 1;
        std::vector<int> h((size_t)gpu_matches.rows * gpu_matches.cols * cn);
        gpu_matches.download(h.data(), sizeof(int) * gpu_matches.cols * cn);
        if (pairs) {
            const int nq = gpu_matches.cols, nr = gpu_matches.rows;
            unpackLists(h.data(), nr == 3 ? h.data() + (size_t)2 * nq : nullptr, reinterpret_cast<const float *>(h.data() + (size_t)(nr - 1) * 2 * nq),
                        nq, 2, 2, nullptr, compactResult, false, matches);
        } else {
            const int nq = gpu_matches.rows / 2, k = gpu_matches.cols;
            unpackLists(h.data(), nullptr, reinterpret_cast<const float *>(h.data() + (size_t)nq * k), nq, k, k, nullptr, compactResult, false, matches);
        }
    }

    // ------------------------------------------------------------------ radiusMatch
    void radiusMatch(InputArray query, InputArray train, std::vector<std::vector<DMatch> > &matches, float maxDistance, InputArray mask,
                     bool compactResult) override
    {
        GpuMat g;
        radiusMatchAsync(query, train, g, maxDistance, mask, Stream::Null());
        radiusMatchConvert(g, matches, compactResult);
    }
    void radiusMatch(InputArray query, std::vector<std::vector<DMatch> > &matches, float maxDistance, const std::vector<GpuMat> &masks,
                     bool compactResult) override
    {
        GpuMat g;
        radiusMatchAsync(query, g, maxDistance, masks, Stream::Null());
        radiusMatchConvert(g, matches, compactResult);
    }
    void radiusMatchAsync(InputArray query, InputArray train, OutputArray matches, float maxDistance, InputArray mask, Stream &stream) override
    {
        if (query.empty() || train.empty()) { matches.release(); return; }
        const int nq = query.rows, cols = std::max(train.rows / 100, nq);
        matches.create(2 * nq + 1, cols, CV_32SC1);                        // :897-904
        mi_mat q = miMat(query), t = miMat(train), m = miMat(mask);
        mi_mat i = packedRows(matches, 0, nq, cols, CV_32SC1), d = packedRows(matches, nq, nq, cols, CV_32FC1);
        mi_mat n = packedRows(matches, 2 * nq, 1, nq, CV_32SC1);
        miCheck(mi_bf_radius_match(h_.get(), &q, &t, mask.empty() ? nullptr : &m, 1, maxDistance, &i, nullptr, &d, &n, stream.hipStream()));
    }
    void radiusMatchAsync(InputArray query, OutputArray matches, float maxDistance, const std::vector<GpuMat> &masks, Stream &stream) override
    {
        if (query.empty() || coll_.empty()) { matches.release(); return; }
        const int nq = query.rows;
        matches.create(3 * nq + 1, nq, CV_32FC1);                          // :969-975 (typed CV_32FC1 there too)
        std::vector<mi_mat> ts, ms;
        collection(masks, ts, ms);
        mi_mat q = miMat(query);
        mi_mat i = packedRows(matches, 0, nq, nq, CV_32SC1), g = packedRows(matches, nq, nq, nq, CV_32SC1);
        mi_mat d = packedRows(matches, 2 * nq, nq, nq, CV_32FC1), n = packedRows(matches, 3 * nq, 1, nq, CV_32SC1);
        miCheck(mi_bf_radius_match(h_.get(), &q, ts.data(), ms.empty() ? nullptr : ms.data(), (int)ts.size(), maxDistance, &i, &g, &d, &n,
                                   stream.hipStream()));
    }
    void radiusMatchConvert(InputArray gpu_matches, std::vector<std::vector<DMatch> > &matches, bool compactResult) override
    {
        matches.clear();
        if (gpu_matches.empty()) return;
        CV_Assert(gpu_matches.type() == CV_32SC1 || gpu_matches.type() == CV_32FC1);
        const bool coll = gpu_matches.type() == CV_32FC1;                  // :1007-1024
        const int cols = gpu_matches.cols, nq = (gpu_matches.rows - 1) / (coll ? 3 : 2);
        std::vector<int> h((size_t)gpu_matches.rows * cols);
        gpu_matches.download(h.data(), sizeof(int) * cols);
        const size_t blk = (size_t)nq * cols;
        unpackLists(h.data(), coll ? h.data() + blk : nullptr, reinterpret_cast<const float *>(h.data() + (coll ? 2 : 1) * blk), nq, cols, cols,
                    h.data() + (coll ? 3 : 2) * blk, compactResult, true, matches);
    }

private:
    // makeGpuCollection (brute_force_matcher.cpp:143-185)
    void collection(const std::vector<GpuMat> &masks, std::vector<mi_mat> &ts, std::vector<mi_mat> &ms) const
    {
        CV_Assert(masks.empty() || masks.size() == coll_.size());
        for (size_t j = 0; j < coll_.size(); ++j) ts.push_back(miMat(coll_[j]));
        for (size_t j = 0; j < masks.size(); ++j) {
            mi_mat m = miMat(masks[j]);
            if (masks[j].empty()) { m.data = nullptr; m.step = 0; m.rows = m.cols = 0; }
            ms.push_back(m);
        }
    }
    // idx / img / dist: nq rows of `stride` entries; n: entries valid per row (NULL: every entry whose trainIdx != -1)
    static void unpackLists(const int *idx, const int *img, const float *dist, int nq, int k, int stride, const int *n, bool compactResult,
                            bool sortRows, std::vector<std::vector<DMatch> > &matches)
    {
        for (int q = 0; q < nq; ++q) {
            std::vector<DMatch> row;
            const int cnt = n ? std::min(n[q], k) : k;
            for (int j = 0; j < cnt; ++j) {
                const size_t e = (size_t)q * stride + j;
                if (n || idx[e] != -1) row.push_back(DMatch(q, idx[e], img ? img[e] : 0, dist[e]));
            }
            if (sortRows) std::stable_sort(row.begin(), row.end());
            if (!compactResult || !row.empty()) matches.push_back(row);
        }
    }

    ParamHandle<mi_bfmatcher, int, nullptr, nullptr, mi_bf_destroy> h_;   // the norm type is its only parameter, fixed at create
    std::vector<GpuMat> coll_;
};
}  // namespace miflow_detail

inline Ptr<DescriptorMatcher> DescriptorMatcher::createBFMatcher(int normType) { return makePtr<miflow_detail::BFMatcherImpl>(normType); }

// ---------------------------------------------------------------- FastFeatureDetector
}  // namespace cuda

#ifndef MIFLOW_WITH_OPENCV
/** the constants of the main repository's cv::FastFeatureDetector (opencv2/features2d.hpp) that the factory's default names */
class FastFeatureDetector {
public:
    enum { TYPE_5_8 = 0, TYPE_7_12 = 1, TYPE_9_16 = 2 };
};
#endif

namespace cuda {

/** cudafeatures2d.hpp:377-418, of which the detector uses detectAsync and convert.  The reference derives it from cv::Feature2D (main
 * repository); here it stands on cv::Algorithm. */
class CV_EXPORTS_W Feature2DAsync : public cv::Algorithm {
public:
    virtual ~Feature2DAsync() {}
    virtual void detect(InputArray image, std::vector<KeyPoint> &keypoints, InputArray mask = GpuMat()) = 0;
    virtual void detectAsync(InputArray image, OutputArray keypoints, InputArray mask = GpuMat(), Stream &stream = Stream::Null()) = 0;
    virtual void convert(InputArray gpu_keypoints, std::vector<KeyPoint> &keypoints) = 0;
};

/** cudafeatures2d.hpp:426-442 over mi_fast_* (include/miflow/c_api.h).  Keypoints come in row-major order of the image (the reference:
 * in the arrival order of its atomics).  get/setThreshold's getter, get/setNonmaxSuppression and get/setType are FAST_Impl's
 * (fast.cpp:76-86); the reference's public class declares setThreshold, setMaxNumPoints and getMaxNumPoints only. */
class CV_EXPORTS_W FastFeatureDetector : public Feature2DAsync {
public:
    static const int LOCATION_ROW = 0;
    static const int RESPONSE_ROW = 1;
    static const int ROWS_COUNT = 2;
    static const int FEATURE_SIZE = 7;

    static Ptr<cuda::FastFeatureDetector> create(int threshold = 10, bool nonmaxSuppression = true,
                                                 int type = cv::FastFeatureDetector::TYPE_9_16, int max_npoints = 5000);
    virtual void setThreshold(int threshold) = 0;
    virtual int getThreshold() const = 0;
    virtual void setNonmaxSuppression(bool f) = 0;
    virtual bool getNonmaxSuppression() const = 0;
    virtual void setMaxNumPoints(int max_npoints) = 0;
    virtual int getMaxNumPoints() const = 0;
    virtual void setType(int type) = 0;
    virtual int getType() const = 0;
    /** shim-only: convert() of a matrix that already is on the host (the reference takes it through InputArray, fast.cpp:188-191):
     * rows of `step` bytes, npoints columns */
    virtual void convert(const void *host_keypoints, size_t step, int npoints, std::vector<KeyPoint> &keypoints) = 0;
    using Feature2DAsync::convert;
};

namespace miflow_detail {
/** twin of FAST_Impl, cudafeatures2d/src/fast.cpp:63-209 */
class FastImpl final : public cuda::FastFeatureDetector {
public:
    explicit FastImpl(const mi_fast_params &p) : h_(p) {}
    void detect(InputArray image, std::vector<KeyPoint> &keypoints, InputArray mask) override
    {
        if (image.empty()) { keypoints.clear(); return; }   // fast.cpp:109-113
        GpuMat k;
        detectAsync(image, k, mask, Stream::Null());
        convert(k, keypoints);
    }
    void detectAsync(InputArray image, OutputArray keypoints, InputArray mask, Stream &stream) override
    {
        GpuMat buf(ROWS_COUNT, h_.params().max_npoints, CV_32FC1);   // the pool's buffer of fast.cpp:116
        mi_mat i = miMat(image), m = miMat(mask), k = miMat(buf);
        int n = 0;
        miCheck(mi_fast_detect(h_.get(), &i, mask.empty() ? nullptr : &m, &k, &n, stream.hipStream()));
        if (n == 0) { keypoints.release(); return; }   // fast.cpp:146-150,158-161
        keypoints = buf(Rect(0, 0, n, ROWS_COUNT));    // keypoints.cols = count (:164)
    }
    void convert(InputArray gpu_keypoints, std::vector<KeyPoint> &keypoints) override
    {
        if (gpu_keypoints.empty()) { keypoints.clear(); return; }   // fast.cpp:177-181
        CV_Assert(gpu_keypoints.rows == ROWS_COUNT);
        CV_Assert(gpu_keypoints.elemSize() == 4);
        const int n = gpu_keypoints.cols;
        std::vector<float> host((size_t)ROWS_COUNT * n);
        gpu_keypoints.download(host.data(), (size_t)n * 4);
        convert(host.data(), (size_t)n * 4, n, keypoints);
    }
    void convert(const void *host_keypoints, size_t step, int npoints, std::vector<KeyPoint> &keypoints) override
    {
        keypoints.resize(npoints);   // fast.cpp:196-207
        const short *loc = (const short *)((const unsigned char *)host_keypoints + LOCATION_ROW * step);
        const float *resp = (const float *)((const unsigned char *)host_keypoints + RESPONSE_ROW * step);
        for (int i = 0; i < npoints; ++i) keypoints[i] = KeyPoint(loc[2 * i], loc[2 * i + 1], (float)FEATURE_SIZE, -1, resp[i]);
    }
    void setThreshold(int v) override { h_.set([=](auto &q) { q.threshold = v; }); }
    int getThreshold() const override { return h_.params().threshold; }
    void setNonmaxSuppression(bool f) override { h_.set([=](auto &q) { q.nonmax_suppression = f ? 1 : 0; }); }
    bool getNonmaxSuppression() const override { return h_.params().nonmax_suppression != 0; }
    void setMaxNumPoints(int v) override { h_.set([=](auto &q) { q.max_npoints = v; }); }
    int getMaxNumPoints() const override { return h_.params().max_npoints; }
    void setType(int type) override { CV_Assert(type == cv::FastFeatureDetector::TYPE_9_16); }   // fast.cpp:85
    int getType() const override { return cv::FastFeatureDetector::TYPE_9_16; }
private:
    ParamHandle<mi_fast, mi_fast_params, mi_fast_create, mi_fast_set_params, mi_fast_destroy> h_;
};
}  // namespace miflow_detail

inline Ptr<cuda::FastFeatureDetector> FastFeatureDetector::create(int threshold, bool nonmaxSuppression, int type, int max_npoints)
{
    CV_Assert(type == cv::FastFeatureDetector::TYPE_9_16);   // fast.cpp:213
    const mi_fast_params p = {threshold, nonmaxSuppression ? 1 : 0, max_npoints};
    return makePtr<miflow_detail::FastImpl>(p);
}

// ---------------------------------------------------------------- ORB
}  // namespace cuda

#ifndef MIFLOW_WITH_OPENCV
/** the constants of the main repository's cv::ORB (opencv2/features2d.hpp) that the factory's defaults and descriptorSize() name */
class ORB {
public:
    enum { kBytes = 32, HARRIS_SCORE = 0, FAST_SCORE = 1 };
};
#endif

namespace cuda {

/** cudafeatures2d.hpp:452-505 over mi_orb_* (include/miflow/c_api.h).  DESIGN.md 4.11 has what differs from the reference: the pool of
 * test points is an argument (`pattern0`, 512 points {x, y}; none: makeRandomPattern for every patch size), the culls keep FAST's
 * row-major order among equal responses, and setters take effect on quotas, u_max and pattern at once. */
class CV_EXPORTS_W ORB : public Feature2DAsync {
public:
    static const int X_ROW = 0;
    static const int Y_ROW = 1;
    static const int RESPONSE_ROW = 2;
    static const int ANGLE_ROW = 3;
    static const int OCTAVE_ROW = 4;
    static const int SIZE_ROW = 5;
    static const int ROWS_COUNT = 6;
    enum { PATTERN_RANDOM = 0, PATTERN_PROVIDED = 1 };

    static Ptr<cuda::ORB> create(int nfeatures = 500, float scaleFactor = 1.2f, int nlevels = 8, int edgeThreshold = 31, int firstLevel = 0,
                                 int WTA_K = 2, int scoreType = cv::ORB::HARRIS_SCORE, int patchSize = 31, int fastThreshold = 20,
                                 bool blurForDescriptor = false);
    /** shim-only: the same with the caller's pool of 512 test points {x, y} (an OpenCV binding passes the learned table of its cv::ORB) */
    static Ptr<cuda::ORB> create(const int *pattern0, int nfeatures, float scaleFactor, int nlevels, int edgeThreshold, int firstLevel, int WTA_K,
                                 int scoreType, int patchSize, int fastThreshold, bool blurForDescriptor);
    virtual void detectAndCompute(InputArray image, InputArray mask, std::vector<KeyPoint> &keypoints, OutputArray descriptors,
                                  bool useProvidedKeypoints = false) = 0;
    virtual void detectAndComputeAsync(InputArray image, InputArray mask, OutputArray keypoints, OutputArray descriptors,
                                       bool useProvidedKeypoints = false, Stream &stream = Stream::Null()) = 0;
    virtual int descriptorSize() const = 0;
    virtual int descriptorType() const = 0;
    virtual int defaultNorm() const = 0;
    virtual void setMaxFeatures(int maxFeatures) = 0;
    virtual int getMaxFeatures() const = 0;
    virtual void setScaleFactor(double scaleFactor) = 0;
    virtual double getScaleFactor() const = 0;
    virtual void setNLevels(int nlevels) = 0;
    virtual int getNLevels() const = 0;
    virtual void setEdgeThreshold(int edgeThreshold) = 0;
    virtual int getEdgeThreshold() const = 0;
    virtual void setFirstLevel(int firstLevel) = 0;
    virtual int getFirstLevel() const = 0;
    virtual void setWTA_K(int wta_k) = 0;
    virtual int getWTA_K() const = 0;
    virtual void setScoreType(int scoreType) = 0;
    virtual int getScoreType() const = 0;
    virtual void setPatchSize(int patchSize) = 0;
    virtual int getPatchSize() const = 0;
    virtual void setFastThreshold(int fastThreshold) = 0;
    virtual int getFastThreshold() const = 0;
    virtual void setBlurForDescriptor(bool blurForDescriptor) = 0;
    virtual bool getBlurForDescriptor() const = 0;
    /** shim-only: PATTERN_RANDOM or PATTERN_PROVIDED */
    virtual int getPatternSource() const = 0;
};

namespace miflow_detail {
/** twin of ORB_Impl, cudafeatures2d/src/orb.cpp:338-913 */
class OrbImpl final : public cuda::ORB {
public:
    OrbImpl(const int *pattern0, const mi_orb_params &p)
        : h_(p, [=](const mi_orb_params *q, mi_orb **h) {
              mi_mat pool = {const_cast<int *>(pattern0), 8, 512, 2, MI_32SC1};
              return mi_orb_create(q, pattern0 ? &pool : nullptr, h);
          })
    {
    }

    void detect(InputArray image, std::vector<KeyPoint> &keypoints, InputArray mask) override
    {
        GpuMat k;
        run(image, mask, &k, nullptr, Stream::Null());
        convert(k, keypoints);
    }
    void detectAsync(InputArray image, OutputArray keypoints, InputArray mask, Stream &stream) override
    {
        GpuMat k;
        run(image, mask, &k, nullptr, stream);
        if (k.empty()) keypoints.release(); else keypoints = k;
    }
    void detectAndCompute(InputArray image, InputArray mask, std::vector<KeyPoint> &keypoints, OutputArray descriptors,
                          bool useProvidedKeypoints) override
    {
        if (useProvidedKeypoints) { provided(image, keypoints, descriptors); return; }
        GpuMat k, d;
        run(image, mask, &k, &d, Stream::Null());
        if (d.empty()) descriptors.release(); else descriptors = d;
        convert(k, keypoints);   // orb.cpp:639-641
    }
    void detectAndComputeAsync(InputArray image, InputArray mask, OutputArray keypoints, OutputArray descriptors, bool useProvidedKeypoints,
                               Stream &stream) override
    {
        CV_Assert(!useProvidedKeypoints);   // the provided keypoints live in detectAndCompute's vector (orb.cpp:581-635)
        GpuMat k, d;
        run(image, mask, &k, &d, stream);
        if (k.empty()) keypoints.release(); else keypoints = k;
        if (d.empty()) descriptors.release(); else descriptors = d;
    }
    void convert(InputArray gpu_keypoints, std::vector<KeyPoint> &keypoints) override
    {
        if (gpu_keypoints.empty()) { keypoints.clear(); return; }   // orb.cpp:870-874
        CV_Assert(gpu_keypoints.rows == ROWS_COUNT);
        CV_Assert(gpu_keypoints.type() == CV_32FC1);
        const int n = gpu_keypoints.cols;
        std::vector<float> h((size_t)ROWS_COUNT * n);
        gpu_keypoints.download(h.data(), (size_t)n * 4);
        keypoints.resize(n);   // orb.cpp:889-912
        for (int i = 0; i < n; ++i) {
            KeyPoint kp(h[(size_t)X_ROW * n + i], h[(size_t)Y_ROW * n + i], h[(size_t)SIZE_ROW * n + i], h[(size_t)ANGLE_ROW * n + i],
                        h[(size_t)RESPONSE_ROW * n + i]);
            kp.octave = (int)h[(size_t)OCTAVE_ROW * n + i];
            keypoints[i] = kp;
        }
    }
    int descriptorSize() const override { return cv::ORB::kBytes; }
    int descriptorType() const override { return CV_8U; }
    int defaultNorm() const override { return NORM_HAMMING; }
    void setMaxFeatures(int v) override { h_.set([=](auto &q) { q.nfeatures = v; }); }
    int getMaxFeatures() const override { return h_.params().nfeatures; }
    void setScaleFactor(double v) override { h_.set([=](auto &q) { q.scale_factor = (float)v; }); }
    double getScaleFactor() const override { return h_.params().scale_factor; }
    void setNLevels(int v) override { h_.set([=](auto &q) { q.nlevels = v; }); }
    int getNLevels() const override { return h_.params().nlevels; }
    void setEdgeThreshold(int v) override { h_.set([=](auto &q) { q.edge_threshold = v; }); }
    int getEdgeThreshold() const override { return h_.params().edge_threshold; }
    void setFirstLevel(int v) override { h_.set([=](auto &q) { q.first_level = v; }); }
    int getFirstLevel() const override { return h_.params().first_level; }
    void setWTA_K(int v) override { CV_Assert(v == 2 || v == 3 || v == 4); h_.set([=](auto &q) { q.wta_k = v; }); }   // orb.cpp:376
    int getWTA_K() const override { return h_.params().wta_k; }
    void setScoreType(int v) override { h_.set([=](auto &q) { q.score_type = v; }); }
    int getScoreType() const override { return h_.params().score_type; }
    void setPatchSize(int v) override { CV_Assert(v >= 2); h_.set([=](auto &q) { q.patch_size = v; }); }             // orb.cpp:382
    int getPatchSize() const override { return h_.params().patch_size; }
    void setFastThreshold(int v) override { h_.set([=](auto &q) { q.fast_threshold = v; }); }
    int getFastThreshold() const override { return h_.params().fast_threshold; }
    void setBlurForDescriptor(bool v) override { h_.set([=](auto &q) { q.blur_for_descriptor = v ? 1 : 0; }); }
    bool getBlurForDescriptor() const override { return h_.params().blur_for_descriptor != 0; }
    int getPatternSource() const override { int s = 0; miCheck(mi_orb_pattern_source(h_.get(), &s)); return s; }
private:
    // detection: *kp (and *desc, if wanted) receive the first n columns / rows, or stay empty
    void run(InputArray image, InputArray mask, GpuMat *kp, GpuMat *desc, Stream &stream)
    {
        const int cap = h_.params().nfeatures > 0 ? h_.params().nfeatures : 1;
        GpuMat kbuf(ROWS_COUNT, cap, CV_32FC1), dbuf;
        if (desc) dbuf.create(cap, cv::ORB::kBytes, CV_8UC1);
        mi_mat i = miMat(image), m = miMat(mask), k = miMat(kbuf), d = miMat(dbuf);
        int n = 0;
        miCheck(mi_orb_detect_and_compute(h_.get(), &i, mask.empty() ? nullptr : &m, &k, desc ? &d : nullptr, &n, 0, stream.hipStream()));
        if (n == 0) return;   // orb.cpp:793-797,834-838: released
        *kp = kbuf(Rect(0, 0, n, ROWS_COUNT));
        if (desc) *desc = dbuf(Rect(0, 0, cv::ORB::kBytes, n));
    }
    void provided(InputArray image, std::vector<KeyPoint> &keypoints, OutputArray descriptors)
    {
        int n = (int)keypoints.size();
        if (n == 0) { descriptors.release(); return; }
        std::vector<float> h((size_t)ROWS_COUNT * n);
        for (int i = 0; i < n; ++i) {
            const KeyPoint &kp = keypoints[i];
            CV_Assert(kp.octave >= 0);   // orb.cpp:591
            h[(size_t)X_ROW * n + i] = kp.pt.x; h[(size_t)Y_ROW * n + i] = kp.pt.y; h[(size_t)RESPONSE_ROW * n + i] = kp.response;
            h[(size_t)ANGLE_ROW * n + i] = kp.angle; h[(size_t)OCTAVE_ROW * n + i] = (float)kp.octave; h[(size_t)SIZE_ROW * n + i] = kp.size;
        }
        GpuMat dbuf(n, cv::ORB::kBytes, CV_8UC1);
        mi_mat i = miMat(image), k = {h.data(), (size_t)n * 4, ROWS_COUNT, n, MI_32FC1}, d = miMat(dbuf);
        const int rc = mi_orb_detect_and_compute(h_.get(), &i, nullptr, &k, &d, &n, 1, nullptr);
        h_.refresh([](const mi_orb *h, mi_orb_params *q) { mi_orb_get_params(h, q); return 0; });   // nlevels is overwritten (orb.cpp:587-594); rc is reported first
        miCheck(rc);
        descriptors = dbuf;
    }
    ParamHandle<mi_orb, mi_orb_params, nullptr, mi_orb_set_params, mi_orb_destroy> h_;   // created with the pattern: see the constructor
};
}  // namespace miflow_detail

inline Ptr<cuda::ORB> ORB::create(int nfeatures, float scaleFactor, int nlevels, int edgeThreshold, int firstLevel, int WTA_K, int scoreType,
                                  int patchSize, int fastThreshold, bool blurForDescriptor)
{
    return create(static_cast<const int *>(nullptr), nfeatures, scaleFactor, nlevels, edgeThreshold, firstLevel, WTA_K, scoreType, patchSize,
                  fastThreshold, blurForDescriptor);
}

inline Ptr<cuda::ORB> ORB::create(const int *pattern0, int nfeatures, float scaleFactor, int nlevels, int edgeThreshold, int firstLevel, int WTA_K,
                                  int scoreType, int patchSize, int fastThreshold, bool blurForDescriptor)
{
    CV_Assert(patchSize >= 2);                               // orb.cpp:500
    CV_Assert(WTA_K == 2 || WTA_K == 3 || WTA_K == 4);       // orb.cpp:501
    const mi_orb_params p = {nfeatures, scaleFactor, nlevels, edgeThreshold, firstLevel, WTA_K, scoreType, patchSize, fastThreshold, blurForDescriptor ? 1 : 0};
    return makePtr<miflow_detail::OrbImpl>(pattern0, p);
}

}  // namespace cuda
}  // namespace cv
#endif
