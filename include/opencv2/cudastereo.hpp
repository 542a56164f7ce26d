// Drop-in for modules/cudastereo/include/opencv2/cudastereo.hpp (cuda::StereoBM, StereoBeliefPropagation, StereoSGM,
// DisparityBilateralFilter and their create functions).
#ifndef MIFLOW_OPENCV_CUDASTEREO_HPP
#define MIFLOW_OPENCV_CUDASTEREO_HPP

#include "opencv2/core/cuda.hpp"

namespace cv {

#ifndef MIFLOW_WITH_OPENCV
/** the part of cv::StereoMatcher / cv::StereoBM (main repo calib3d.hpp) that cuda::StereoBM inherits */
class StereoMatcher : public Algorithm {
public:
    virtual int getMinDisparity() const = 0;       virtual void setMinDisparity(int) = 0;
    virtual int getNumDisparities() const = 0;     virtual void setNumDisparities(int) = 0;
    virtual int getBlockSize() const = 0;          virtual void setBlockSize(int) = 0;
    virtual int getSpeckleWindowSize() const = 0;  virtual void setSpeckleWindowSize(int) = 0;
    virtual int getSpeckleRange() const = 0;       virtual void setSpeckleRange(int) = 0;
    virtual int getDisp12MaxDiff() const = 0;      virtual void setDisp12MaxDiff(int) = 0;
};
class StereoBM : public StereoMatcher {
public:
    enum { PREFILTER_NORMALIZED_RESPONSE = 0, PREFILTER_XSOBEL = 1 };
    virtual int getPreFilterType() const = 0;      virtual void setPreFilterType(int) = 0;
    virtual int getPreFilterSize() const = 0;      virtual void setPreFilterSize(int) = 0;
    virtual int getPreFilterCap() const = 0;       virtual void setPreFilterCap(int) = 0;
    virtual int getTextureThreshold() const = 0;   virtual void setTextureThreshold(int) = 0;
    virtual int getUniquenessRatio() const = 0;    virtual void setUniquenessRatio(int) = 0;
    virtual int getSmallerBlockSize() const = 0;   virtual void setSmallerBlockSize(int) = 0;
    virtual Rect getROI1() const = 0;              virtual void setROI1(Rect) = 0;
    virtual Rect getROI2() const = 0;              virtual void setROI2(Rect) = 0;
};
#endif

namespace cuda {

/** cudastereo.hpp:72-84 */
class StereoBM : public cv::StereoBM {
public:
    virtual void compute(InputArray left, InputArray right, OutputArray disparity) = 0;
    virtual void compute(InputArray left, InputArray right, OutputArray disparity, Stream &stream) = 0;
};

namespace miflow_detail {
/** twin of StereoBMImpl, cudastereo/src/stereobm.cpp:67-132 (no-op setters and constant getters included) */
class StereoBMImpl final : public cuda::StereoBM {
public:
    explicit StereoBMImpl(const mi_stereobm_params &p) : h_(p) {}
    void compute(InputArray left, InputArray right, OutputArray disparity) override { compute(left, right, disparity, Stream::Null()); }
    void compute(InputArray left, InputArray right, OutputArray disparity, Stream &stream) override
    {
        disparity.create(left.size(), CV_8UC1);   // stereobm.cpp:154
        mi_mat l = miMat(left), r = miMat(right), d = miMat(disparity);
        miCheck(mi_stereobm_compute(h_.get(), &l, &r, &d, stream.hipStream()));
    }
    // n pairs through this object (miflow extension; reached through cv::cuda::miflow::computeBatch)
    void computeBatch(const std::vector<GpuMat> &lefts, const std::vector<GpuMat> &rights, std::vector<GpuMat> &disps, Stream &stream)
    {
        CV_Assert(!lefts.empty() && lefts.size() == rights.size());
        disps.resize(lefts.size());
        std::vector<mi_mat> l(lefts.size()), r(lefts.size()), d(lefts.size());
        for (size_t i = 0; i < lefts.size(); ++i) {
            disps[i].create(lefts[i].size(), CV_8UC1);
            l[i] = miMat(lefts[i]); r[i] = miMat(rights[i]); d[i] = miMat(disps[i]);
        }
        miCheck(mi_stereobm_compute_batch(h_.get(), (int)l.size(), l.data(), r.data(), d.data(), stream.hipStream()));
    }
    int getMinDisparity() const override { return 0; }           void setMinDisparity(int) override {}
    int getNumDisparities() const override { return h_.params().num_disparities; }
    void setNumDisparities(int v) override { h_.set([=](auto &q) { q.num_disparities = v; }); }
    int getBlockSize() const override { return h_.params().block_size; }   void setBlockSize(int v) override { h_.set([=](auto &q) { q.block_size = v; }); }
    int getSpeckleWindowSize() const override { return 0; }      void setSpeckleWindowSize(int) override {}
    int getSpeckleRange() const override { return 0; }           void setSpeckleRange(int) override {}
    int getDisp12MaxDiff() const override { return 0; }          void setDisp12MaxDiff(int) override {}
    int getPreFilterType() const override { return h_.params().prefilter_type; }  void setPreFilterType(int v) override { h_.set([=](auto &q) { q.prefilter_type = v; }); }
    int getPreFilterSize() const override { return h_.params().prefilter_size; }  void setPreFilterSize(int v) override { h_.set([=](auto &q) { q.prefilter_size = v; }); }
    int getPreFilterCap() const override { return h_.params().prefilter_cap; }    void setPreFilterCap(int v) override { h_.set([=](auto &q) { q.prefilter_cap = v; }); }
    int getTextureThreshold() const override { return (int)h_.params().texture_threshold; }
    void setTextureThreshold(int v) override { h_.set([=](auto &q) { q.texture_threshold = (float)v; }); }
    int getUniquenessRatio() const override { return h_.params().uniqueness_ratio; }  void setUniquenessRatio(int v) override { h_.set([=](auto &q) { q.uniqueness_ratio = v; }); }
    int getSmallerBlockSize() const override { return 0; }       void setSmallerBlockSize(int) override {}
    Rect getROI1() const override { return Rect(); }             void setROI1(Rect) override {}
    Rect getROI2() const override { return Rect(); }             void setROI2(Rect) override {}
private:
    ParamHandle<mi_stereobm, mi_stereobm_params, mi_stereobm_create, mi_stereobm_set_params, mi_stereobm_destroy> h_;
};
}  // namespace miflow_detail

/** cudastereo.hpp:90 */
inline Ptr<cuda::StereoBM> createStereoBM(int numDisparities = 64, int blockSize = 19)
{
    mi_stereobm_params p;
    mi_stereobm_default_params(&p);
    p.num_disparities = numDisparities; p.block_size = blockSize;
    return makePtr<miflow_detail::StereoBMImpl>(p);
}

namespace miflow {
/** n stereo pairs through one StereoBM object, back to back on the stream (miflow extension). */
inline void computeBatch(const Ptr<cuda::StereoBM> &bm, const std::vector<GpuMat> &lefts, const std::vector<GpuMat> &rights,
                         std::vector<GpuMat> &disps, Stream &stream = Stream::Null())
{
    auto *impl = dynamic_cast<miflow_detail::StereoBMImpl *>(bm.get());
    CV_Assert(impl);
    impl->computeBatch(lefts, rights, disps, stream);
}
}  // namespace miflow

/** cudastereo.hpp: class StereoSGM (cv::StereoSGBM interface subset used by the CUDA class, cudastereo/src/stereosgm.cpp:20-80) */
class CV_EXPORTS_W StereoSGM : public cv::StereoMatcher {
public:
    enum { MODE_SGBM = 0, MODE_HH = 1, MODE_SGBM_3WAY = 2, MODE_HH4 = 3 };
    virtual void compute(InputArray left, InputArray right, OutputArray disparity) = 0;
    virtual void compute(InputArray left, InputArray right, OutputArray disparity, Stream &stream) = 0;
    virtual int getPreFilterCap() const = 0;      virtual void setPreFilterCap(int) = 0;
    virtual int getUniquenessRatio() const = 0;   virtual void setUniquenessRatio(int) = 0;
    virtual int getP1() const = 0;                virtual void setP1(int) = 0;
    virtual int getP2() const = 0;                virtual void setP2(int) = 0;
    virtual int getMode() const = 0;              virtual void setMode(int) = 0;
};

namespace miflow_detail {
/** twin of StereoSGMImpl, cudastereo/src/stereosgm.cpp:20-146 */
class StereoSGMImpl final : public cuda::StereoSGM {
public:
    explicit StereoSGMImpl(const mi_stereosgm_params &p) : h_(p) {}
    void compute(InputArray left, InputArray right, OutputArray disparity) override { compute(left, right, disparity, Stream::Null()); }
    void compute(InputArray left, InputArray right, OutputArray disparity, Stream &stream) override
    {
        disparity.create(left.size(), CV_MAKETYPE(3 /* CV_16S */, 1));   // stereosgm.cpp:110
        mi_mat l = miMat(left), r = miMat(right), d = miMat(disparity);
        miCheck(mi_stereosgm_compute(h_.get(), &l, &r, &d, stream.hipStream()));
    }
    int getBlockSize() const override { return -1; }             void setBlockSize(int) override {}
    int getDisp12MaxDiff() const override { return 1; }          void setDisp12MaxDiff(int) override {}
    int getMinDisparity() const override { return h_.params().min_disparity; }       void setMinDisparity(int v) override { h_.set([=](auto &q) { q.min_disparity = v; }); }
    int getNumDisparities() const override { return h_.params().num_disparities; }   void setNumDisparities(int v) override { h_.set([=](auto &q) { q.num_disparities = v; }); }
    int getSpeckleWindowSize() const override { return 0; }      void setSpeckleWindowSize(int) override {}
    int getSpeckleRange() const override { return 0; }           void setSpeckleRange(int) override {}
    int getP1() const override { return h_.params().P1; }                 void setP1(int v) override { h_.set([=](auto &q) { q.P1 = v; }); }
    int getP2() const override { return h_.params().P2; }                 void setP2(int v) override { h_.set([=](auto &q) { q.P2 = v; }); }
    int getUniquenessRatio() const override { return h_.params().uniqueness_ratio; } void setUniquenessRatio(int v) override { h_.set([=](auto &q) { q.uniqueness_ratio = v; }); }
    int getMode() const override { return h_.params().mode; }             void setMode(int v) override { h_.set([=](auto &q) { q.mode = v; }); }
    int getPreFilterCap() const override { return -1; }          void setPreFilterCap(int) override {}
private:
    ParamHandle<mi_stereosgm, mi_stereosgm_params, mi_stereosgm_create, mi_stereosgm_set_params, mi_stereosgm_destroy> h_;
};
}  // namespace miflow_detail

/** cudastereo.hpp: createStereoSGM */
inline Ptr<cuda::StereoSGM> createStereoSGM(int minDisparity = 0, int numDisparities = 128, int P1 = 10, int P2 = 120, int uniquenessRatio = 5,
                                            int mode = cuda::StereoSGM::MODE_HH4)
{
    mi_stereosgm_params p;
    mi_stereosgm_default_params(&p);
    p.min_disparity = minDisparity; p.num_disparities = numDisparities; p.P1 = P1; p.P2 = P2;
    p.uniqueness_ratio = uniquenessRatio; p.mode = mode;
    return makePtr<miflow_detail::StereoSGMImpl>(p);
}

#ifndef CV_16S
#define CV_16S 3
#endif

/** cudastereo.hpp:128-179 */
class CV_EXPORTS_W StereoBeliefPropagation : public cv::StereoMatcher {
public:
    virtual void compute(InputArray left, InputArray right, OutputArray disparity) = 0;
    virtual void compute(InputArray left, InputArray right, OutputArray disparity, Stream &stream) = 0;
    /** data: the caller's cost volume, (ndisp * rows) x cols of the message type */
    virtual void compute(InputArray data, OutputArray disparity, Stream &stream = Stream::Null()) = 0;
    virtual int getNumIters() const = 0;           virtual void setNumIters(int iters) = 0;
    virtual int getNumLevels() const = 0;          virtual void setNumLevels(int levels) = 0;
    virtual double getMaxDataTerm() const = 0;     virtual void setMaxDataTerm(double max_data_term) = 0;
    virtual double getDataWeight() const = 0;      virtual void setDataWeight(double data_weight) = 0;
    virtual double getMaxDiscTerm() const = 0;     virtual void setMaxDiscTerm(double max_disc_term) = 0;
    virtual double getDiscSingleJump() const = 0;  virtual void setDiscSingleJump(double disc_single_jump) = 0;
    virtual int getMsgType() const = 0;            virtual void setMsgType(int msg_type) = 0;
    /** stereobp.cpp:367-378 */
    static void estimateRecommendedParams(int width, int height, int &ndisp, int &iters, int &levels)
    {
        miCheck(mi_stereobp_estimate_recommended_params(width, height, &ndisp, &iters, &levels));
    }
};

namespace miflow_detail {
/** twin of StereoBPImpl, cudastereo/src/stereobp.cpp:78-359 (no-op setters and constant getters included) */
class StereoBPImpl final : public cuda::StereoBeliefPropagation {
public:
    explicit StereoBPImpl(const mi_stereobp_params &p) : h_(p) {}
    void compute(InputArray left, InputArray right, OutputArray disparity) override { compute(left, right, disparity, Stream::Null()); }
    void compute(InputArray left, InputArray right, OutputArray disparity, Stream &stream) override
    {
        disparity.create(left.size(), out_type(disparity));
        mi_mat l = miMat(left), r = miMat(right), d = miMat(disparity);
        miCheck(mi_stereobp_compute(h_.get(), &l, &r, &d, stream.hipStream()));
    }
    void compute(InputArray data, OutputArray disparity, Stream &stream) override
    {
        if (h_.params().ndisp > 0) disparity.create(data.rows / h_.params().ndisp, data.cols, out_type(disparity));
        mi_mat m = miMat(data), d = miMat(disparity);
        miCheck(mi_stereobp_compute_data(h_.get(), &m, &d, stream.hipStream()));
    }
    int getMinDisparity() const override { return 0; }           void setMinDisparity(int) override {}
    int getNumDisparities() const override { return h_.params().ndisp; }  void setNumDisparities(int v) override { h_.set([=](auto &q) { q.ndisp = v; }); }
    int getBlockSize() const override { return 0; }              void setBlockSize(int) override {}
    int getSpeckleWindowSize() const override { return 0; }      void setSpeckleWindowSize(int) override {}
    int getSpeckleRange() const override { return 0; }           void setSpeckleRange(int) override {}
    int getDisp12MaxDiff() const override { return 0; }          void setDisp12MaxDiff(int) override {}
    int getNumIters() const override { return h_.params().iters; }        void setNumIters(int v) override { h_.set([=](auto &q) { q.iters = v; }); }
    int getNumLevels() const override { return h_.params().levels; }      void setNumLevels(int v) override { h_.set([=](auto &q) { q.levels = v; }); }
    double getMaxDataTerm() const override { return h_.params().max_data_term; }       void setMaxDataTerm(double v) override { h_.set([=](auto &q) { q.max_data_term = (float)v; }); }
    double getDataWeight() const override { return h_.params().data_weight; }          void setDataWeight(double v) override { h_.set([=](auto &q) { q.data_weight = (float)v; }); }
    double getMaxDiscTerm() const override { return h_.params().max_disc_term; }       void setMaxDiscTerm(double v) override { h_.set([=](auto &q) { q.max_disc_term = (float)v; }); }
    double getDiscSingleJump() const override { return h_.params().disc_single_jump; } void setDiscSingleJump(double v) override { h_.set([=](auto &q) { q.disc_single_jump = (float)v; }); }
    int getMsgType() const override { return h_.params().msg_type; }      void setMsgType(int v) override { h_.set([=](auto &q) { q.msg_type = v; }); }
private:
    // stereobp.cpp:342: a disparity matrix the caller has given a supported type keeps it (the reference asks fixedType()); else CV_16SC1
    static int out_type(const GpuMat &d)
    {
        const int t = d.type();
        return !d.empty() && (t == CV_8UC1 || t == CV_32SC1 || t == CV_32FC1) ? t : CV_MAKETYPE(CV_16S, 1);
    }
    ParamHandle<mi_stereobp, mi_stereobp_params, mi_stereobp_create, mi_stereobp_set_params, mi_stereobp_destroy> h_;   // values are validated at compute, as in the reference
};
}  // namespace miflow_detail

/** cudastereo.hpp:188-189 */
inline Ptr<cuda::StereoBeliefPropagation> createStereoBeliefPropagation(int ndisp = 64, int iters = 5, int levels = 5, int msg_type = CV_32F)
{
    mi_stereobp_params p;
    mi_stereobp_default_params(&p);
    p.ndisp = ndisp; p.iters = iters; p.levels = levels; p.msg_type = msg_type;
    return makePtr<miflow_detail::StereoBPImpl>(p);
}

/** cudastereo.hpp:217-231 */
class CV_EXPORTS_W StereoConstantSpaceBP : public cuda::StereoBeliefPropagation {
public:
    virtual int getNrPlane() const = 0;                  virtual void setNrPlane(int nr_plane) = 0;
    virtual bool getUseLocalInitDataCost() const = 0;    virtual void setUseLocalInitDataCost(bool use_local_init_data_cost) = 0;
    /** stereocsbp.cpp:342-355 */
    static void estimateRecommendedParams(int width, int height, int &ndisp, int &iters, int &levels, int &nr_plane)
    {
        miCheck(mi_stereocsbp_estimate_recommended_params(width, height, &ndisp, &iters, &levels, &nr_plane));
    }
};

namespace miflow_detail {
/** twin of StereoCSBPImpl, cudastereo/src/stereocsbp.cpp:60-334 (no-op setters and constant getters included) */
class StereoCSBPImpl final : public cuda::StereoConstantSpaceBP {
public:
    explicit StereoCSBPImpl(const mi_stereocsbp_params &p) : h_(p) {}
    void compute(InputArray left, InputArray right, OutputArray disparity) override { compute(left, right, disparity, Stream::Null()); }
    void compute(InputArray left, InputArray right, OutputArray disparity, Stream &stream) override
    {
        disparity.create(left.size(), out_type(disparity));
        mi_mat l = miMat(left), r = miMat(right), d = miMat(disparity);
        miCheck(mi_stereocsbp_compute(h_.get(), &l, &r, &d, stream.hipStream()));
        h_.refresh(mi_stereocsbp_get_params);   // levels_ is clamped by compute (stereocsbp.cpp:171)
    }
    void compute(InputArray, OutputArray, Stream &) override { CV_Error(Error::StsNotImplemented, "Not implemented"); }   // :331-334
    int getMinDisparity() const override { return h_.params().min_disp_th; }  void setMinDisparity(int v) override { h_.set([=](auto &q) { q.min_disp_th = v; }); }
    int getNumDisparities() const override { return h_.params().ndisp; }  void setNumDisparities(int v) override { h_.set([=](auto &q) { q.ndisp = v; }); }
    int getBlockSize() const override { return 0; }              void setBlockSize(int) override {}
    int getSpeckleWindowSize() const override { return 0; }      void setSpeckleWindowSize(int) override {}
    int getSpeckleRange() const override { return 0; }           void setSpeckleRange(int) override {}
    int getDisp12MaxDiff() const override { return 0; }          void setDisp12MaxDiff(int) override {}
    int getNumIters() const override { return h_.params().iters; }        void setNumIters(int v) override { h_.set([=](auto &q) { q.iters = v; }); }
    int getNumLevels() const override { return h_.params().levels; }      void setNumLevels(int v) override { h_.set([=](auto &q) { q.levels = v; }); }
    double getMaxDataTerm() const override { return h_.params().max_data_term; }       void setMaxDataTerm(double v) override { h_.set([=](auto &q) { q.max_data_term = (float)v; }); }
    double getDataWeight() const override { return h_.params().data_weight; }          void setDataWeight(double v) override { h_.set([=](auto &q) { q.data_weight = (float)v; }); }
    double getMaxDiscTerm() const override { return h_.params().max_disc_term; }       void setMaxDiscTerm(double v) override { h_.set([=](auto &q) { q.max_disc_term = (float)v; }); }
    double getDiscSingleJump() const override { return h_.params().disc_single_jump; } void setDiscSingleJump(double v) override { h_.set([=](auto &q) { q.disc_single_jump = (float)v; }); }
    int getMsgType() const override { return h_.params().msg_type; }      void setMsgType(int v) override { h_.set([=](auto &q) { q.msg_type = v; }); }
    int getNrPlane() const override { return h_.params().nr_plane; }      void setNrPlane(int v) override { h_.set([=](auto &q) { q.nr_plane = v; }); }
    bool getUseLocalInitDataCost() const override { return h_.params().use_local_init_data_cost != 0; }
    void setUseLocalInitDataCost(bool v) override { h_.set([=](auto &q) { q.use_local_init_data_cost = v ? 1 : 0; }); }
private:
    // stereocsbp.cpp:303: a disparity matrix the caller has given a supported type keeps it (the reference asks fixedType()); else CV_16SC1
    static int out_type(const GpuMat &d)
    {
        const int t = d.type();
        return !d.empty() && (t == CV_8UC1 || t == CV_32SC1 || t == CV_32FC1) ? t : CV_MAKETYPE(CV_16S, 1);
    }
    ParamHandle<mi_stereocsbp, mi_stereocsbp_params, mi_stereocsbp_create, mi_stereocsbp_set_params, mi_stereocsbp_destroy> h_;   // values are validated at compute, as in the reference
};
}  // namespace miflow_detail

/** cudastereo.hpp:241-242 */
inline Ptr<cuda::StereoConstantSpaceBP> createStereoConstantSpaceBP(int ndisp = 128, int iters = 8, int levels = 4, int nr_plane = 4,
                                                                    int msg_type = CV_32F)
{
    mi_stereocsbp_params p;
    mi_stereocsbp_default_params(&p);
    p.ndisp = ndisp; p.iters = iters; p.levels = levels; p.nr_plane = nr_plane; p.msg_type = msg_type;
    return makePtr<miflow_detail::StereoCSBPImpl>(p);
}

/** cudastereo.hpp:298-330 */
class CV_EXPORTS_W DisparityBilateralFilter : public cv::Algorithm {
public:
    virtual void apply(InputArray disparity, InputArray image, OutputArray dst, Stream &stream = Stream::Null()) = 0;
    virtual int getNumDisparities() const = 0;        virtual void setNumDisparities(int numDisparities) = 0;
    virtual int getRadius() const = 0;                virtual void setRadius(int radius) = 0;
    virtual int getNumIters() const = 0;              virtual void setNumIters(int iters) = 0;
    virtual double getEdgeThreshold() const = 0;      virtual void setEdgeThreshold(double edge_threshold) = 0;
    virtual double getMaxDiscThreshold() const = 0;   virtual void setMaxDiscThreshold(double max_disc_threshold) = 0;
    virtual double getSigmaRange() const = 0;         virtual void setSigmaRange(double sigma_range) = 0;
};

namespace miflow_detail {
/** twin of DispBilateralFilterImpl, cudastereo/src/disparity_bilateral_filter.cpp:58-190 */
class DispBilateralFilterImpl final : public cuda::DisparityBilateralFilter {
public:
    explicit DispBilateralFilterImpl(const mi_disp_bilateral_params &p) : h_(p) {}
    void apply(InputArray disparity, InputArray image, OutputArray dst, Stream &stream) override
    {
        if (dst.data != disparity.data) dst.create(disparity.size(), disparity.type());   // disparity_bilateral_filter.cpp:152
        mi_mat d = miMat(disparity), i = miMat(image), o = miMat(dst);
        miCheck(mi_disp_bilateral_apply(h_.get(), &d, &i, &o, stream.hipStream()));
    }
    int getNumDisparities() const override { return h_.params().ndisp; }                  void setNumDisparities(int v) override { h_.set([=](auto &q) { q.ndisp = v; }); }
    int getRadius() const override { return h_.params().radius; }                         void setRadius(int v) override { h_.set([=](auto &q) { q.radius = v; }); }
    int getNumIters() const override { return h_.params().iters; }                        void setNumIters(int v) override { h_.set([=](auto &q) { q.iters = v; }); }
    double getEdgeThreshold() const override { return h_.params().edge_threshold; }       void setEdgeThreshold(double v) override { h_.set([=](auto &q) { q.edge_threshold = (float)v; }); }
    double getMaxDiscThreshold() const override { return h_.params().max_disc_threshold; } void setMaxDiscThreshold(double v) override { h_.set([=](auto &q) { q.max_disc_threshold = (float)v; }); }
    double getSigmaRange() const override { return h_.params().sigma_range; }             void setSigmaRange(double v) override { h_.set([=](auto &q) { q.sigma_range = (float)v; }); }
private:
    ParamHandle<mi_disp_bilateral, mi_disp_bilateral_params, mi_disp_bilateral_create, mi_disp_bilateral_set_params, mi_disp_bilateral_destroy> h_;
};
}  // namespace miflow_detail

/** cudastereo.hpp:338-339 */
inline Ptr<cuda::DisparityBilateralFilter> createDisparityBilateralFilter(int ndisp = 64, int radius = 3, int iters = 1)
{
    mi_disp_bilateral_params p;
    mi_disp_bilateral_default_params(&p);
    p.ndisp = ndisp; p.radius = radius; p.iters = iters;
    return makePtr<miflow_detail::DispBilateralFilterImpl>(p);
}

}}  // namespace cv::cuda
#endif
