// Drop-in for modules/cudaoptflow/include/opencv2/cudaoptflow.hpp (the classes on the hot path):
// same class names, factory signatures, defaults and getters/setters; implementation = the miflow
// C-ABI (include/miflow/c_api.h, libmiflow.so) running hand-written gfx950 HIP kernels.
#ifndef MIFLOW_OPENCV_CUDAOPTFLOW_HPP
#define MIFLOW_OPENCV_CUDAOPTFLOW_HPP

#include "opencv2/core/cuda.hpp"

namespace cv { namespace cuda {

/** cudaoptflow.hpp:70-81 */
class DenseOpticalFlow : public Algorithm {
public:
    virtual void calc(InputArray I0, InputArray I1, InputOutputArray flow, Stream &stream = Stream::Null()) = 0;
};

/** cudaoptflow.hpp:305-386; implementation twin of OpticalFlowDual_TVL1_Impl, cudaoptflow/src/tvl1flow.cpp:80-168 */
class OpticalFlowDual_TVL1 : public DenseOpticalFlow {
public:
    virtual double getTau() const = 0;             virtual void setTau(double tau) = 0;
    virtual double getLambda() const = 0;          virtual void setLambda(double lambda) = 0;
    virtual double getGamma() const = 0;           virtual void setGamma(double gamma) = 0;
    virtual double getTheta() const = 0;           virtual void setTheta(double theta) = 0;
    virtual int getNumScales() const = 0;          virtual void setNumScales(int nscales) = 0;
    virtual int getNumWarps() const = 0;           virtual void setNumWarps(int warps) = 0;
    virtual double getEpsilon() const = 0;         virtual void setEpsilon(double epsilon) = 0;
    virtual int getNumIterations() const = 0;      virtual void setNumIterations(int iterations) = 0;
    virtual double getScaleStep() const = 0;       virtual void setScaleStep(double scaleStep) = 0;
    virtual bool getUseInitialFlow() const = 0;    virtual void setUseInitialFlow(bool useInitialFlow) = 0;

    static Ptr<OpticalFlowDual_TVL1> create(double tau = 0.25, double lambda = 0.15, double theta = 0.3, int nscales = 5,
                                            int warps = 5, double epsilon = 0.01, int iterations = 300,
                                            double scaleStep = 0.8, double gamma = 0.0, bool useInitialFlow = false);
};

namespace miflow_detail {
class TVL1Impl final : public OpticalFlowDual_TVL1 {
public:
    explicit TVL1Impl(const mi_tvl1_params &p) : h_(p) {}
    void calc(InputArray I0, InputArray I1, InputOutputArray flow, Stream &stream) override
    {
        // BufferPool/merge of the reference (tvl1flow.cpp:175-182): the flow matrix is (re)allocated by the callee
        if (!h_.params().use_initial_flow) flow.create(I0.size(), CV_32FC2);
        mi_mat a = miMat(I0), b = miMat(I1), f = miMat(flow);
        miCheck(mi_tvl1_calc(h_.get(), &a, &b, &f, stream.hipStream()));
        // the reference shrinks nscales_ for good when a pyramid level falls below 16 px (tvl1flow.cpp:243-247)
        h_.refresh(mi_tvl1_get_params);
    }
    // Batched-frames mode (miflow extension; reached through cv::cuda::miflow::calcBatch): n independent pairs of one size and
    // type per launch sequence, blockIdx.z = pair.  flows[i] is (re)allocated like calc() does.
    void calcBatch(const std::vector<GpuMat> &I0s, const std::vector<GpuMat> &I1s, std::vector<GpuMat> &flows, Stream &stream)
    {
        CV_Assert(!I0s.empty() && I0s.size() == I1s.size());
        if (!h_.params().use_initial_flow) flows.resize(I0s.size());
        CV_Assert(flows.size() == I0s.size());
        std::vector<mi_mat> a(I0s.size()), b(I0s.size()), f(I0s.size());
        for (size_t i = 0; i < I0s.size(); ++i) {
            if (!h_.params().use_initial_flow) flows[i].create(I0s[i].size(), CV_32FC2);
            a[i] = miMat(I0s[i]); b[i] = miMat(I1s[i]); f[i] = miMat(flows[i]);
        }
        miCheck(mi_tvl1_calc_batch(h_.get(), (int)a.size(), a.data(), b.data(), f.data(), stream.hipStream()));
        h_.refresh(mi_tvl1_get_params);
    }
    void setExtra(int semantics, int exact_math, int time_block, int lanes)
    {
        h_.set([=](auto &q) { q.semantics = semantics; q.exact_math = exact_math; q.time_block = time_block; q.lanes = lanes; });
    }
    void setStopSlack(int slack) { h_.set([=](auto &q) { q.stop_slack = slack; }); }
    void setHostFeedback(int mode) { h_.set([=](auto &q) { q.host_feedback = mode; }); }
    const mi_tvl1_params &params() const { return h_.params(); }
    String getDefaultName() const override { return "DenseOpticalFlow.OpticalFlowDual_TVL1"; }   // tvl1flow.cpp:122
#define MIFLOW_PROP(T, Name, field) \
    T get##Name() const override { return (T)h_.params().field; } \
    void set##Name(T v) override { h_.set([=](auto &q) { q.field = v; }); }
    MIFLOW_PROP(double, Tau, tau) MIFLOW_PROP(double, Lambda, lambda) MIFLOW_PROP(double, Gamma, gamma)
    MIFLOW_PROP(double, Theta, theta) MIFLOW_PROP(int, NumScales, nscales) MIFLOW_PROP(int, NumWarps, warps)
    MIFLOW_PROP(double, Epsilon, epsilon) MIFLOW_PROP(int, NumIterations, iterations) MIFLOW_PROP(double, ScaleStep, scale_step)
#undef MIFLOW_PROP
    bool getUseInitialFlow() const override { return h_.params().use_initial_flow != 0; }
    void setUseInitialFlow(bool v) override { h_.set([=](auto &q) { q.use_initial_flow = v; }); }
    mi_tvl1 *handle() { return h_.get(); }
private:
    ParamHandle<mi_tvl1, mi_tvl1_params, mi_tvl1_create, mi_tvl1_set_params, mi_tvl1_destroy> h_;
};
}  // namespace miflow_detail

inline Ptr<OpticalFlowDual_TVL1> OpticalFlowDual_TVL1::create(double tau, double lambda, double theta, int nscales, int warps,
                                                              double epsilon, int iterations, double scaleStep, double gamma,
                                                              bool useInitialFlow)
{
    mi_tvl1_params p;
    mi_tvl1_default_params(&p);
    p.tau = tau; p.lambda = lambda; p.theta = theta; p.nscales = nscales; p.warps = warps; p.epsilon = epsilon;
    p.iterations = iterations; p.scale_step = scaleStep; p.gamma = gamma; p.use_initial_flow = useInitialFlow;
    return makePtr<miflow_detail::TVL1Impl>(p);
}

/** miflow extensions to OpticalFlowDual_TVL1 -- everything the reference class does not have lives in this namespace, the class
 *  declaration above is the reference's.  NOTE ON NUMERICS: a default-constructed object computes with the arithmetic of the
 *  CPU class cv::optflow::DualTVL1OpticalFlow (MI_SEM_CPU_REF: the acceptance reference of this path, "EPE vs CPU ref") in fast
 *  device math, iterations fused per HBM pass; cv::cuda's own kernels differ from the CPU class by ~0.1 px mean EPE (border
 *  addressing, resize convention, check schedule) and are selected with setSemantics(alg, MI_SEM_CUDA_COMPAT). */
namespace miflow {
/** MI_SEM_CPU_REF (default) = the arithmetic of cv::optflow::DualTVL1OpticalFlow (cv::remap warp, cv::resize pyramid,
 *  convergence test after every iteration); MI_SEM_CUDA_COMPAT = cv::cuda's kernels (normalised a = -0.5 bicubic with clamp
 *  addressing, cuda::resize, sparse check schedule), bit-pinned on the reference's OpenCL twins. */
inline void setSemantics(const Ptr<OpticalFlowDual_TVL1> &alg, int semantics)
{
    auto *impl = dynamic_cast<miflow_detail::TVL1Impl *>(alg.get());
    CV_Assert(impl);
    impl->setExtra(semantics, impl->params().exact_math, impl->params().time_block, impl->params().lanes);
}
/** true: IEEE divide, f64 hypot, separately rounded operations in the reference's order (fused in blocks of up to 5 iterations when epsilon == 0)
 *  (bit-comparable with the CPU restatement); false (default): v_rcp / v_sqrt / fma, temporally blocked. */
inline void setExactMath(const Ptr<OpticalFlowDual_TVL1> &alg, bool exact)
{
    auto *impl = dynamic_cast<miflow_detail::TVL1Impl *>(alg.get());
    CV_Assert(impl);
    impl->setExtra(impl->params().semantics, exact ? 1 : 0, impl->params().time_block, impl->params().lanes);
}
/** 0 (default): the inner loop of a warp stops exactly where the reference's convergence test stops it; s > 0: it may run up
 *  to s iterations further (mi_tvl1_params.stop_slack). */
inline void setStopSlack(const Ptr<OpticalFlowDual_TVL1> &alg, int slack)
{
    auto *impl = dynamic_cast<miflow_detail::TVL1Impl *>(alg.get());
    CV_Assert(impl);
    impl->setStopSlack(slack);
}
/** mi_tvl1_params.host_feedback: 0 (default) = a convergence-checked calc() of one or two pairs waits for the device about once per
 *  warp -- as the reference's class does at every convergence check (cudaoptflow/src/tvl1flow.cpp:362-368) -- and stops enqueuing
 *  launches for a warp that has converged; -1 = never wait inside calc(); 1 = for every single-lane call.  Same flows either way. */
inline void setHostFeedback(const Ptr<OpticalFlowDual_TVL1> &alg, int mode)
{
    auto *impl = dynamic_cast<miflow_detail::TVL1Impl *>(alg.get());
    CV_Assert(impl);
    impl->setHostFeedback(mode);
}
/** n independent image pairs of identical size and type in one pass (the batched-frames mode of BASELINE configs[4]). */
inline void calcBatch(const Ptr<OpticalFlowDual_TVL1> &alg, const std::vector<GpuMat> &I0s, const std::vector<GpuMat> &I1s,
                      std::vector<GpuMat> &flows, Stream &stream = Stream::Null())
{
    auto *impl = dynamic_cast<miflow_detail::TVL1Impl *>(alg.get());
    CV_Assert(impl);
    impl->calcBatch(I0s, I1s, flows, stream);
}
}  // namespace miflow

/** cudaoptflow.hpp:258-294; implementation twin of FarnebackOpticalFlowImpl, cudaoptflow/src/farneback.cpp:96-165 */
class FarnebackOpticalFlow : public DenseOpticalFlow {
public:
    virtual int getNumLevels() const = 0;        virtual void setNumLevels(int numLevels) = 0;
    virtual double getPyrScale() const = 0;      virtual void setPyrScale(double pyrScale) = 0;
    virtual bool getFastPyramids() const = 0;    virtual void setFastPyramids(bool fastPyramids) = 0;
    virtual int getWinSize() const = 0;          virtual void setWinSize(int winSize) = 0;
    virtual int getNumIters() const = 0;         virtual void setNumIters(int numIters) = 0;
    virtual int getPolyN() const = 0;            virtual void setPolyN(int polyN) = 0;
    virtual double getPolySigma() const = 0;     virtual void setPolySigma(double polySigma) = 0;
    virtual int getFlags() const = 0;            virtual void setFlags(int flags) = 0;

    static Ptr<FarnebackOpticalFlow> create(int numLevels = 5, double pyrScale = 0.5, bool fastPyramids = false, int winSize = 13,
                                            int numIters = 10, int polyN = 5, double polySigma = 1.1, int flags = 0);
};

namespace miflow_detail {
class FarnebackImpl final : public FarnebackOpticalFlow {
public:
    explicit FarnebackImpl(const mi_farneback_params &p) : h_(p) {}
    void calc(InputArray I0, InputArray I1, InputOutputArray flow, Stream &stream) override
    {
        if (!(h_.params().flags & MI_OPTFLOW_USE_INITIAL_FLOW)) flow.create(I0.size(), CV_32FC2);   // farneback.cpp:189-198 (create + merge)
        mi_mat a = miMat(I0), b = miMat(I1), f = miMat(flow);
        miCheck(mi_farneback_calc(h_.get(), &a, &b, &f, stream.hipStream()));
    }
    // Batched-frames mode (miflow extension; reached through cv::cuda::miflow::calcBatch)
    void calcBatch(const std::vector<GpuMat> &I0s, const std::vector<GpuMat> &I1s, std::vector<GpuMat> &flows, Stream &stream)
    {
        CV_Assert(!I0s.empty() && I0s.size() == I1s.size());
        const bool init = (h_.params().flags & MI_OPTFLOW_USE_INITIAL_FLOW) != 0;
        if (!init) flows.resize(I0s.size());
        CV_Assert(flows.size() == I0s.size());
        std::vector<mi_mat> a(I0s.size()), b(I0s.size()), f(I0s.size());
        for (size_t i = 0; i < I0s.size(); ++i) {
            if (!init) flows[i].create(I0s[i].size(), CV_32FC2);
            a[i] = miMat(I0s[i]); b[i] = miMat(I1s[i]); f[i] = miMat(flows[i]);
        }
        miCheck(mi_farneback_calc_batch(h_.get(), (int)a.size(), a.data(), b.data(), f.data(), stream.hipStream()));
    }
    String getDefaultName() const override { return "DenseOpticalFlow.FarnebackOpticalFlow"; }   // farneback.cpp:132
#define MIFLOW_PROP(T, Name, field) \
    T get##Name() const override { return (T)h_.params().field; } \
    void set##Name(T v) override { h_.set([=](auto &q) { q.field = v; }); }
    MIFLOW_PROP(int, NumLevels, num_levels) MIFLOW_PROP(double, PyrScale, pyr_scale) MIFLOW_PROP(int, WinSize, win_size)
    MIFLOW_PROP(int, NumIters, num_iters) MIFLOW_PROP(int, PolyN, poly_n) MIFLOW_PROP(double, PolySigma, poly_sigma)
    MIFLOW_PROP(int, Flags, flags)
#undef MIFLOW_PROP
    bool getFastPyramids() const override { return h_.params().fast_pyramids != 0; }
    void setFastPyramids(bool v) override { h_.set([=](auto &q) { q.fast_pyramids = v; }); }
private:
    ParamHandle<mi_farneback, mi_farneback_params, mi_farneback_create, mi_farneback_set_params, mi_farneback_destroy> h_;
};
}  // namespace miflow_detail

inline Ptr<FarnebackOpticalFlow> FarnebackOpticalFlow::create(int numLevels, double pyrScale, bool fastPyramids, int winSize,
                                                              int numIters, int polyN, double polySigma, int flags)
{
    mi_farneback_params p;
    mi_farneback_default_params(&p);
    p.num_levels = numLevels; p.pyr_scale = pyrScale; p.fast_pyramids = fastPyramids; p.win_size = winSize;
    p.num_iters = numIters; p.poly_n = polyN; p.poly_sigma = polySigma; p.flags = flags;
    return makePtr<miflow_detail::FarnebackImpl>(p);
}

namespace miflow {
/** n independent pairs in one pass through a FarnebackOpticalFlow object (blockIdx.z = pair in every kernel of the level loop). */
inline void calcBatch(const Ptr<FarnebackOpticalFlow> &alg, const std::vector<GpuMat> &I0s, const std::vector<GpuMat> &I1s,
                      std::vector<GpuMat> &flows, Stream &stream = Stream::Null())
{
    auto *impl = dynamic_cast<miflow_detail::FarnebackImpl *>(alg.get());
    CV_Assert(impl);
    impl->calcBatch(I0s, I1s, flows, stream);
}
}  // namespace miflow

/** cudaoptflow.hpp: class DensePyrLKOpticalFlow; implementation twin of DensePyrLKOpticalFlowImpl, cudaoptflow/src/pyrlk.cpp:354-406 */
class DensePyrLKOpticalFlow : public DenseOpticalFlow {
public:
    virtual Size getWinSize() const = 0;          virtual void setWinSize(Size winSize) = 0;
    virtual int getMaxLevel() const = 0;          virtual void setMaxLevel(int maxLevel) = 0;
    virtual int getNumIters() const = 0;          virtual void setNumIters(int iters) = 0;
    virtual bool getUseInitialFlow() const = 0;   virtual void setUseInitialFlow(bool useInitialFlow) = 0;
    static Ptr<DensePyrLKOpticalFlow> create(Size winSize = Size(13, 13), int maxLevel = 3, int iters = 30, bool useInitialFlow = false);
};

namespace miflow_detail {
class DensePyrLKImpl final : public DensePyrLKOpticalFlow {
public:
    explicit DensePyrLKImpl(const mi_densepyrlk_params &p) : h_(p) {}
    void calc(InputArray prevImg, InputArray nextImg, InputOutputArray flow, Stream &stream) override
    {
        flow.create(prevImg.size(), CV_32FC2);   // cuda::merge into _flow, pyrlk.cpp:390-391
        mi_mat a = miMat(prevImg), b = miMat(nextImg), f = miMat(flow);
        miCheck(mi_densepyrlk_calc(h_.get(), &a, &b, &f, stream.hipStream()));
    }
    String getDefaultName() const override { return "DenseOpticalFlow.DensePyrLKOpticalFlow"; }   // pyrlk.cpp:394
    Size getWinSize() const override { return Size(h_.params().win_width, h_.params().win_height); }
    void setWinSize(Size v) override { h_.set([=](auto &q) { q.win_width = v.width; q.win_height = v.height; }); }
    int getMaxLevel() const override { return h_.params().max_level; }           void setMaxLevel(int v) override { h_.set([=](auto &q) { q.max_level = v; }); }
    int getNumIters() const override { return h_.params().iters; }               void setNumIters(int v) override { h_.set([=](auto &q) { q.iters = v; }); }
    bool getUseInitialFlow() const override { return h_.params().use_initial_flow != 0; }
    void setUseInitialFlow(bool v) override { h_.set([=](auto &q) { q.use_initial_flow = v; }); }
private:
    ParamHandle<mi_densepyrlk, mi_densepyrlk_params, mi_densepyrlk_create, mi_densepyrlk_set_params, mi_densepyrlk_destroy> h_;
};
}  // namespace miflow_detail

inline Ptr<DensePyrLKOpticalFlow> DensePyrLKOpticalFlow::create(Size winSize, int maxLevel, int iters, bool useInitialFlow)
{
    mi_densepyrlk_params p;
    mi_densepyrlk_default_params(&p);
    p.win_width = winSize.width; p.win_height = winSize.height; p.max_level = maxLevel; p.iters = iters; p.use_initial_flow = useInitialFlow;
    return makePtr<miflow_detail::DensePyrLKImpl>(p);
}

/** cudaoptflow.hpp:155-186 class BroxOpticalFlow; implementation twin of BroxOpticalFlowImpl, cudaoptflow/src/brox.cpp:56-188, and of
 *  NCVBroxOpticalFlow, cudalegacy/src/cuda/NCVBroxOpticalFlow.cu.  CV_32FC1 frames of one size, each side at least 4.  The parameters
 *  live in the handle as binary32, as NCVBroxOpticalFlowDescriptor holds them (brox.cpp:151-156): a getter returns the float's value. */
class BroxOpticalFlow : public DenseOpticalFlow {
public:
    virtual double getFlowSmoothness() const = 0;                 virtual void setFlowSmoothness(double alpha) = 0;
    virtual double getGradientConstancyImportance() const = 0;    virtual void setGradientConstancyImportance(double gamma) = 0;
    virtual double getPyramidScaleFactor() const = 0;             virtual void setPyramidScaleFactor(double scale_factor) = 0;
    virtual int getInnerIterations() const = 0;                   virtual void setInnerIterations(int inner_iterations) = 0;
    virtual int getOuterIterations() const = 0;                   virtual void setOuterIterations(int outer_iterations) = 0;
    virtual int getSolverIterations() const = 0;                  virtual void setSolverIterations(int solver_iterations) = 0;
    static Ptr<BroxOpticalFlow> create(double alpha = 0.197, double gamma = 50.0, double scale_factor = 0.8, int inner_iterations = 5,
                                       int outer_iterations = 150, int solver_iterations = 10);
};

namespace miflow_detail {
class BroxImpl final : public BroxOpticalFlow {
public:
    explicit BroxImpl(const mi_brox_params &p) : h_(p) {}
    void calc(InputArray I0, InputArray I1, InputOutputArray flow, Stream &stream) override
    {
        flow.create(I0.size(), CV_32FC2);   // brox.cpp:183-185
        mi_mat a = miMat(I0), b = miMat(I1), f = miMat(flow);
        miCheck(mi_brox_calc(h_.get(), &a, &b, &f, stream.hipStream()));
    }
    String getDefaultName() const override { return "DenseOpticalFlow.BroxOpticalFlow"; }   // brox.cpp:67
    double getFlowSmoothness() const override { return h_.params().alpha; }
    void setFlowSmoothness(double v) override { h_.set([=](auto &q) { q.alpha = (float)v; }); }
    double getGradientConstancyImportance() const override { return h_.params().gamma; }
    void setGradientConstancyImportance(double v) override { h_.set([=](auto &q) { q.gamma = (float)v; }); }
    double getPyramidScaleFactor() const override { return h_.params().scale_factor; }
    void setPyramidScaleFactor(double v) override { h_.set([=](auto &q) { q.scale_factor = (float)v; }); }
    int getInnerIterations() const override { return h_.params().inner_iterations; }
    void setInnerIterations(int v) override { h_.set([=](auto &q) { q.inner_iterations = v; }); }
    int getOuterIterations() const override { return h_.params().outer_iterations; }
    void setOuterIterations(int v) override { h_.set([=](auto &q) { q.outer_iterations = v; }); }
    int getSolverIterations() const override { return h_.params().solver_iterations; }
    void setSolverIterations(int v) override { h_.set([=](auto &q) { q.solver_iterations = v; }); }
    mi_brox *handle() const { return h_.get(); }   // miflow::setSolverForm
private:
    ParamHandle<mi_brox, mi_brox_params, mi_brox_create, mi_brox_set_params, mi_brox_destroy> h_;
};
}  // namespace miflow_detail

inline Ptr<BroxOpticalFlow> BroxOpticalFlow::create(double alpha, double gamma, double scale_factor, int inner_iterations, int outer_iterations,
                                                    int solver_iterations)
{
    const mi_brox_params p = {(float)alpha, (float)gamma, (float)scale_factor, inner_iterations, outer_iterations, solver_iterations};
    return makePtr<miflow_detail::BroxImpl>(p);
}

namespace miflow {
/** miflow extension: the solver's form, MI_BROX_FORM_AUTO / PLAIN / BLOCKED; the bits do not depend on it */
inline void setSolverForm(const Ptr<BroxOpticalFlow> &alg, int form)
{
    auto *impl = dynamic_cast<miflow_detail::BroxImpl *>(alg.get());
    CV_Assert(impl);
    miCheck(mi_brox_set_form(impl->handle(), form));
}
}  // namespace miflow

/** cudaoptflow.hpp:85-104 SparseOpticalFlow, :203-223 SparsePyrLKOpticalFlow; implementation twin of SparsePyrLKOpticalFlowImpl,
 *  cudaoptflow/src/pyrlk.cpp:308-352.  CV_8UC1 frames.  `err` defaults to cuda::noArray() (a shared empty GpuMat): not computed. */
inline GpuMat &noArray() { static thread_local GpuMat none; none.release(); return none; }

class SparseOpticalFlow : public Algorithm {
public:
    virtual void calc(InputArray prevImg, InputArray nextImg, InputArray prevPts, InputOutputArray nextPts, OutputArray status,
                      OutputArray err = noArray(), Stream &stream = Stream::Null()) = 0;
};

class SparsePyrLKOpticalFlow : public SparseOpticalFlow {
public:
    virtual Size getWinSize() const = 0;          virtual void setWinSize(Size winSize) = 0;
    virtual int getMaxLevel() const = 0;          virtual void setMaxLevel(int maxLevel) = 0;
    virtual int getNumIters() const = 0;          virtual void setNumIters(int iters) = 0;
    virtual bool getUseInitialFlow() const = 0;   virtual void setUseInitialFlow(bool useInitialFlow) = 0;
    static Ptr<SparsePyrLKOpticalFlow> create(Size winSize = Size(21, 21), int maxLevel = 3, int iters = 30, bool useInitialFlow = false);
};

namespace miflow_detail {
class SparsePyrLKImpl final : public SparsePyrLKOpticalFlow {
public:
    explicit SparsePyrLKImpl(const mi_sparsepyrlk_params &p) : h_(p) {}
    void calc(InputArray prevImg, InputArray nextImg, InputArray prevPts, InputOutputArray nextPts, OutputArray status, OutputArray err,
              Stream &stream) override
    {
        const bool wantErr = &err != &noArray();
        if (prevPts.empty()) {                                    // pyrlk.cpp:209-215
            nextPts.release(); status.release();
            if (wantErr) err.release();
            return;
        }
        if (h_.params().use_initial_flow) CV_Assert(nextPts.size() == prevPts.size() && nextPts.type() == prevPts.type());   // :159-160
        else nextPts.create(1, prevPts.cols, prevPts.type());
        status.create(1, prevPts.cols, CV_8UC1);
        if (wantErr) err.create(1, prevPts.cols, CV_32FC1);
        mi_mat a = miMat(prevImg), b = miMat(nextImg), pp = miMat(prevPts), np = miMat(nextPts), st = miMat(status), er = miMat(err);
        miCheck(mi_sparsepyrlk_calc(h_.get(), &a, &b, &pp, &np, &st, wantErr ? &er : nullptr, stream.hipStream()));
    }
    String getDefaultName() const override { return "SparseOpticalFlow.SparsePyrLKOpticalFlow"; }   // pyrlk.cpp:351
    Size getWinSize() const override { return Size(h_.params().win_width, h_.params().win_height); }
    void setWinSize(Size v) override { h_.set([=](auto &q) { q.win_width = v.width; q.win_height = v.height; }); }
    int getMaxLevel() const override { return h_.params().max_level; }           void setMaxLevel(int v) override { h_.set([=](auto &q) { q.max_level = v; }); }
    int getNumIters() const override { return h_.params().iters; }               void setNumIters(int v) override { h_.set([=](auto &q) { q.iters = v; }); }
    bool getUseInitialFlow() const override { return h_.params().use_initial_flow != 0; }
    void setUseInitialFlow(bool v) override { h_.set([=](auto &q) { q.use_initial_flow = v; }); }
private:
    ParamHandle<mi_sparsepyrlk, mi_sparsepyrlk_params, mi_sparsepyrlk_create, mi_sparsepyrlk_set_params, mi_sparsepyrlk_destroy> h_;
};
}  // namespace miflow_detail

inline Ptr<SparsePyrLKOpticalFlow> SparsePyrLKOpticalFlow::create(Size winSize, int maxLevel, int iters, bool useInitialFlow)
{
    mi_sparsepyrlk_params p;
    mi_sparsepyrlk_default_params(&p);
    p.win_width = winSize.width; p.win_height = winSize.height; p.max_level = maxLevel; p.iters = iters; p.use_initial_flow = useInitialFlow;
    return makePtr<miflow_detail::SparsePyrLKImpl>(p);
}

}}  // namespace cv::cuda
#endif
