// cv::superres::createSuperResolution_BTVL1_CUDA() over libmiflow: BTV-L1 super-resolution, the one consumer of the superres
// optical-flow adapters in the reference.
//
// Same declarations as the reference (superres/include/opencv2/superres.hpp:60-203): FrameSource, createFrameSource_Empty(),
// SuperResolution with its accessors, createSuperResolution_BTVL1_CUDA().  The classes follow superres/src/super_resolution.cpp
// (setInput / nextFrame / reset) and superres/src/btv_l1_cuda.cpp:209-588: BTVL1_CUDA_Base::process is one call of the C-ABI
// (mi_btvl1_process: three set-up launches, then two launches per iteration), the frame ring, the two flow calls per new frame and
// the window / baseIdx selection of BTVL1_CUDA are restated here line by line.
// Shim differences: frames are cv::cuda::GpuMat where the reference has OutputArray (this repository's stand-in core has no cv::Mat);
// the video / camera frame sources are absent (no videoio), createFrameSource_List() stands in for them; frames are CV_8U or
// CV_32F with 1, 3 or 4 channels.
#ifndef OPENCV_SUPERRES_MIFLOW_HPP
#define OPENCV_SUPERRES_MIFLOW_HPP

#include <algorithm>
#include <utility>
#include <vector>
#include "opencv2/core/cuda.hpp"
#include "opencv2/superres/optical_flow.hpp"

namespace cv {
namespace superres {

class CV_EXPORTS FrameSource {
public:
    virtual ~FrameSource() {}

    virtual void nextFrame(cuda::OutputArray frame) = 0;
    virtual void reset() = 0;
};

class CV_EXPORTS SuperResolution : public cv::Algorithm, public FrameSource {
public:
    void setInput(const Ptr<FrameSource> &frameSource)
    {
        frameSource_ = frameSource;
        firstCall_ = true;
    }

    void nextFrame(cuda::OutputArray frame) CV_OVERRIDE
    {
        if (firstCall_) {
            initImpl(frameSource_);
            firstCall_ = false;
        }
        processImpl(frameSource_, frame);
    }
    void reset() CV_OVERRIDE
    {
        frameSource_->reset();
        firstCall_ = true;
    }

    virtual void collectGarbage() {}

    virtual int getScale() const = 0;
    virtual void setScale(int val) = 0;
    virtual int getIterations() const = 0;
    virtual void setIterations(int val) = 0;
    virtual double getTau() const = 0;
    virtual void setTau(double val) = 0;
    virtual double getLambda() const = 0;
    virtual void setLambda(double val) = 0;
    virtual double getAlpha() const = 0;
    virtual void setAlpha(double val) = 0;
    virtual int getKernelSize() const = 0;
    virtual void setKernelSize(int val) = 0;
    virtual int getBlurKernelSize() const = 0;
    virtual void setBlurKernelSize(int val) = 0;
    virtual double getBlurSigma() const = 0;
    virtual void setBlurSigma(double val) = 0;
    virtual int getTemporalAreaRadius() const = 0;
    virtual void setTemporalAreaRadius(int val) = 0;
    virtual Ptr<cv::superres::DenseOpticalFlowExt> getOpticalFlow() const = 0;
    virtual void setOpticalFlow(const Ptr<cv::superres::DenseOpticalFlowExt> &val) = 0;

protected:
    SuperResolution();

    virtual void initImpl(Ptr<FrameSource> &frameSource) = 0;
    virtual void processImpl(Ptr<FrameSource> &frameSource, cuda::OutputArray output) = 0;

    bool isUmat_;

private:
    Ptr<FrameSource> frameSource_;
    bool firstCall_;
};

namespace detail {

class EmptyFrameSource : public FrameSource {
public:
    void nextFrame(cuda::OutputArray frame) CV_OVERRIDE { frame.release(); }
    void reset() CV_OVERRIDE {}
};

// shim-only: a source over frames already on the device
class ListFrameSource : public FrameSource {
public:
    explicit ListFrameSource(const std::vector<cuda::GpuMat> &frames) : frames_(frames), pos_(0) {}
    void nextFrame(cuda::OutputArray frame) CV_OVERRIDE
    {
        if (pos_ >= frames_.size()) { frame.release(); return; }
        frame = frames_[pos_++];
    }
    void reset() CV_OVERRIDE { pos_ = 0; }

private:
    std::vector<cuda::GpuMat> frames_;
    size_t pos_;
};

// GpuMat::convertTo(dst, depth) between CV_8U and CV_32F (saturate_cast), or copyTo for equal depths
inline void convertDepth(const cuda::GpuMat &src, cuda::GpuMat &dst, int depth)
{
    dst.create(src.size(), CV_MAKETYPE(depth, src.channels()));
    mi_mat s = cuda::miMat(src), d = cuda::miMat(dst);
    cuda::miCheck(mi_btvl1_convert(&s, &d, nullptr));
}

// the reference's at(index, items): ring access
template <typename T> inline T &at(int index, std::vector<T> &items)
{
    const int len = static_cast<int>(items.size());
    return items[((index % len) + len) % len];
}

typedef std::pair<cuda::GpuMat, cuda::GpuMat> MotionPair;

class BTVL1_CUDA_Base : public cv::superres::SuperResolution {
public:
    BTVL1_CUDA_Base() : handle_(nullptr)
    {
        mi_btvl1_params p;
        mi_btvl1_default_params(&p);   // btv_l1_cuda.cpp:280-289
        scale_ = p.scale; iterations_ = p.iterations; lambda_ = p.lambda; tau_ = p.tau; alpha_ = p.alpha;
        btvKernelSize_ = p.btv_kernel_size; blurKernelSize_ = p.blur_kernel_size; blurSigma_ = p.blur_sigma;
        opticalFlow_ = createOptFlow_Farneback_CUDA();   // :292
        temporalAreaRadius_ = 0;
        cuda::miCheck(mi_btvl1_create(&p, &handle_));
    }
    ~BTVL1_CUDA_Base() { mi_btvl1_destroy(handle_); }
    BTVL1_CUDA_Base(const BTVL1_CUDA_Base &) = delete;
    BTVL1_CUDA_Base &operator=(const BTVL1_CUDA_Base &) = delete;

    // btv_l1_cuda.cpp:306-400; the result is ready when the call returns
    void process(const std::vector<cuda::GpuMat> &src, cuda::GpuMat &dst, const std::vector<MotionPair> &forwardMotions,
                 const std::vector<MotionPair> &backwardMotions, int baseIdx)
    {
        CV_Assert(!src.empty() && forwardMotions.size() == src.size() && backwardMotions.size() == src.size());
        mi_btvl1_params p;
        p.scale = scale_; p.iterations = iterations_; p.tau = tau_; p.lambda = lambda_; p.alpha = alpha_;
        p.btv_kernel_size = btvKernelSize_; p.blur_kernel_size = blurKernelSize_; p.blur_sigma = blurSigma_;
        cuda::miCheck(mi_btvl1_set_params(handle_, &p));
        const size_t n = src.size();
        std::vector<mi_mat> f(n), fx(n), fy(n), bx(n), by(n);
        for (size_t i = 0; i < n; ++i) {
            f[i] = cuda::miMat(src[i]);
            fx[i] = cuda::miMat(forwardMotions[i].first); fy[i] = cuda::miMat(forwardMotions[i].second);
            bx[i] = cuda::miMat(backwardMotions[i].first); by[i] = cuda::miMat(backwardMotions[i].second);
        }
        CV_Assert(scale_ > 1 && btvKernelSize_ > 0);
        dst.create(src[0].rows * scale_ - 2 * btvKernelSize_, src[0].cols * scale_ - 2 * btvKernelSize_, src[0].type());
        CV_Assert(!dst.empty());
        mi_mat d = cuda::miMat(dst);
        cuda::miCheck(mi_btvl1_process(handle_, static_cast<int>(n), f.data(), fx.data(), fy.data(), bx.data(), by.data(), baseIdx, &d, nullptr));
        cuda::miCheck(mi_stream_synchronize(nullptr));
    }

    void collectGarbage() CV_OVERRIDE
    {
        mi_btvl1_destroy(handle_);   // the scratch arena goes, the parameters stay (btv_l1_cuda.cpp:402-422)
        handle_ = nullptr;
        cuda::miCheck(mi_btvl1_create(nullptr, &handle_));
    }

    int getScale() const CV_OVERRIDE { return scale_; }
    void setScale(int val) CV_OVERRIDE { scale_ = val; }
    int getIterations() const CV_OVERRIDE { return iterations_; }
    void setIterations(int val) CV_OVERRIDE { iterations_ = val; }
    double getTau() const CV_OVERRIDE { return tau_; }
    void setTau(double val) CV_OVERRIDE { tau_ = val; }
    double getLambda() const CV_OVERRIDE { return lambda_; }
    void setLambda(double val) CV_OVERRIDE { lambda_ = val; }
    double getAlpha() const CV_OVERRIDE { return alpha_; }
    void setAlpha(double val) CV_OVERRIDE { alpha_ = val; }
    int getKernelSize() const CV_OVERRIDE { return btvKernelSize_; }
    void setKernelSize(int val) CV_OVERRIDE { btvKernelSize_ = val; }
    int getBlurKernelSize() const CV_OVERRIDE { return blurKernelSize_; }
    void setBlurKernelSize(int val) CV_OVERRIDE { blurKernelSize_ = val; }
    double getBlurSigma() const CV_OVERRIDE { return blurSigma_; }
    void setBlurSigma(double val) CV_OVERRIDE { blurSigma_ = val; }
    int getTemporalAreaRadius() const CV_OVERRIDE { return temporalAreaRadius_; }
    void setTemporalAreaRadius(int val) CV_OVERRIDE { temporalAreaRadius_ = val; }
    Ptr<cv::superres::DenseOpticalFlowExt> getOpticalFlow() const CV_OVERRIDE { return opticalFlow_; }
    void setOpticalFlow(const Ptr<cv::superres::DenseOpticalFlowExt> &val) CV_OVERRIDE { opticalFlow_ = val; }

protected:
    int scale_;
    int iterations_;
    double lambda_;
    double tau_;
    double alpha_;
    int btvKernelSize_;
    int blurKernelSize_;
    double blurSigma_;
    int temporalAreaRadius_;
    Ptr<cv::superres::DenseOpticalFlowExt> opticalFlow_;

private:
    mi_btvl1 *handle_;
};

class BTVL1_CUDA : public BTVL1_CUDA_Base {
public:
    BTVL1_CUDA() : storePos_(-1), procPos_(0), outPos_(-1) { temporalAreaRadius_ = 4; }   // btv_l1_cuda.cpp:459-462

    void collectGarbage() CV_OVERRIDE
    {
        curFrame_.release(); prevFrame_.release();
        frames_.clear(); forwardMotions_.clear(); backwardMotions_.clear(); outputs_.clear();
        srcFrames_.clear(); srcForwardMotions_.clear(); srcBackwardMotions_.clear();
        SuperResolution::collectGarbage();
        BTVL1_CUDA_Base::collectGarbage();
    }

protected:
    void initImpl(Ptr<FrameSource> &frameSource) CV_OVERRIDE   // btv_l1_cuda.cpp:483-502
    {
        const int cacheSize = 2 * temporalAreaRadius_ + 1;
        frames_.assign(cacheSize, cuda::GpuMat());
        forwardMotions_.assign(cacheSize, MotionPair());
        backwardMotions_.assign(cacheSize, MotionPair());
        outputs_.assign(cacheSize, cuda::GpuMat());
        storePos_ = -1;
        for (int t = -temporalAreaRadius_; t <= temporalAreaRadius_; ++t) readNextFrame(frameSource);
        // the reference runs processFrame(0 .. radius) whatever the source held; only the frames that exist are processed here
        for (int i = 0; i <= std::min(temporalAreaRadius_, storePos_); ++i) processFrame(i);
        procPos_ = temporalAreaRadius_;
        outPos_ = -1;
    }

    void processImpl(Ptr<FrameSource> &frameSource, cuda::OutputArray output) CV_OVERRIDE   // :504-530
    {
        if (outPos_ >= storePos_) {
            output.release();
            return;
        }
        readNextFrame(frameSource);
        if (procPos_ < storePos_) {
            ++procPos_;
            processFrame(procPos_);
        }
        ++outPos_;
        convertDepth(at(outPos_, outputs_), output, CV_8U);
        cuda::miCheck(mi_stream_synchronize(nullptr));
    }

private:
    void readNextFrame(Ptr<FrameSource> &frameSource)   // :532-552
    {
        frameSource->nextFrame(curFrame_);
        if (curFrame_.empty()) return;
        ++storePos_;
        convertDepth(curFrame_, at(storePos_, frames_), CV_32F);
        if (storePos_ > 0) {
            MotionPair &forwardMotion = at(storePos_ - 1, forwardMotions_);
            MotionPair &backwardMotion = at(storePos_, backwardMotions_);
            opticalFlow_->calc(prevFrame_, curFrame_, forwardMotion.first, &forwardMotion.second);
            opticalFlow_->calc(curFrame_, prevFrame_, backwardMotion.first, &backwardMotion.second);
        }
        convertDepth(curFrame_, prevFrame_, curFrame_.depth());   // curFrame_.copyTo(prevFrame_)
    }

    void processFrame(int idx)   // :554-582
    {
        const int startIdx = std::max(idx - temporalAreaRadius_, 0);
        const int procIdx = idx;
        const int endIdx = std::min(startIdx + 2 * temporalAreaRadius_, storePos_);
        const int count = endIdx - startIdx + 1;
        srcFrames_.assign(count, cuda::GpuMat());
        srcForwardMotions_.assign(count, MotionPair());
        srcBackwardMotions_.assign(count, MotionPair());
        int baseIdx = -1;
        for (int i = startIdx, k = 0; i <= endIdx; ++i, ++k) {
            if (i == procIdx) baseIdx = k;
            srcFrames_[k] = at(i, frames_);
            if (i < endIdx) srcForwardMotions_[k] = at(i, forwardMotions_);
            if (i > startIdx) srcBackwardMotions_[k] = at(i, backwardMotions_);
        }
        process(srcFrames_, at(idx, outputs_), srcForwardMotions_, srcBackwardMotions_, baseIdx);
    }

    cuda::GpuMat curFrame_, prevFrame_;
    std::vector<cuda::GpuMat> frames_;
    std::vector<MotionPair> forwardMotions_, backwardMotions_;
    std::vector<cuda::GpuMat> outputs_;
    int storePos_, procPos_, outPos_;
    std::vector<cuda::GpuMat> srcFrames_;
    std::vector<MotionPair> srcForwardMotions_, srcBackwardMotions_;
};

}  // namespace detail

inline SuperResolution::SuperResolution() : isUmat_(false), frameSource_(makePtr<detail::EmptyFrameSource>()), firstCall_(true) {}

inline Ptr<FrameSource> createFrameSource_Empty() { return makePtr<detail::EmptyFrameSource>(); }
// shim-only (the reference's createFrameSource_Video / _Camera need videoio)
inline Ptr<FrameSource> createFrameSource_List(const std::vector<cuda::GpuMat> &frames) { return makePtr<detail::ListFrameSource>(frames); }

inline Ptr<SuperResolution> createSuperResolution_BTVL1_CUDA() { return makePtr<detail::BTVL1_CUDA>(); }

}  // namespace superres
}  // namespace cv

#endif
