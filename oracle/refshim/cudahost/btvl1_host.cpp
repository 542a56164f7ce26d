/*
 * oracle/refshim/cudahost/btvl1_host.cpp -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.
 * The C entry points of libref_cu.so for superres' BTV-L1: the reference's host file modules/superres/src/btv_l1_cuda.cpp is #included
 * below AS IT LIES (not a byte of it is changed or copied), so that this translation unit can name what that file keeps in its unnamed
 * namespace: calcRelativeMotions, upscaleMotions, calcBtvWeights, the class BTVL1_CUDA with BTVL1_CUDA_Base::process.  `private` is
 * spelled `public` while the file is read -- after every header it includes has been read -- which is how btvWeights_ is returned
 * without editing it.  Everything the file calls is the reference's too: btv_l1_gpu.cu, resize.cpp / remap.cpp over resize.cu /
 * remap.cu, the separable-filter slice of filtering.cpp over row_filter.hpp / column_filter.hpp (all on the fiber shim), the
 * functors of cudaarithm; super_resolution.cpp and frame_source.cpp (verbatim) supply SuperResolution::nextFrame and FrameSource.
 * Written here: the list-backed FrameSource, the DenseOpticalFlowExt that replays given flows in call order, arrCopy for GpuMat, and
 * a createOptFlow_Farneback that returns no algorithm (the constructor asks for one; every caller here sets its own).
 */
#include <algorithm>
#include <cstring>
#include <limits>
#include <memory>
#include <string>
#include <utility>
#include <vector>
#include "precomp.hpp"   // superres/src/precomp.hpp: the stub core, the reference's superres.hpp / optical_flow.hpp / ring_buffer.hpp

#define private public
#include "btv_l1_cuda.cpp"
#undef private

namespace btv_l1_cudev { }
using cv::cuda::GpuMat;

namespace {
GpuMat up(const float *p, int rows, int cols, int cn)
{
    GpuMat m(rows, cols, CV_MAKETYPE(CV_32F, cn));
    for (int y = 0; y < rows; ++y) memcpy(m.ptr<unsigned char>(y), p + (size_t)y * cols * cn, sizeof(float) * cols * cn);
    return m;
}
GpuMat up8(const unsigned char *p, int rows, int cols, int cn)
{
    GpuMat m(rows, cols, CV_MAKETYPE(CV_8U, cn));
    for (int y = 0; y < rows; ++y) memcpy(m.ptr<unsigned char>(y), p + (size_t)y * cols * cn, (size_t)cols * cn);
    return m;
}
void down(const GpuMat &m, void *p)
{
    const size_t rb = (size_t)m.cols * cv::elem_size_of(m.type());
    for (int y = 0; y < m.rows; ++y) memcpy((unsigned char *)p + y * rb, m.ptr<unsigned char>(y), rb);
}
typedef std::vector<std::pair<GpuMat, GpuMat> > Motions;
// n entries of (x plane, y plane), dense, present[i] == 0 leaves the pair empty (the reference must not read it)
Motions motions(const float *p, const int *present, int n, int rows, int cols)
{
    Motions m(n);
    for (int i = 0; i < n; ++i)
        if (present[i]) {
            m[i].first = up(p + (size_t)(2 * i) * rows * cols, rows, cols, 1);
            m[i].second = up(p + (size_t)(2 * i + 1) * rows * cols, rows, cols, 1);
        }
    return m;
}
void set_params(cv::superres::SuperResolution &a, int scale, int iterations, double tau, double lambda, double alpha, int btv_ksize, int blur_ksize,
                double blur_sigma)
{
    a.setScale(scale); a.setIterations(iterations); a.setTau(tau); a.setLambda(lambda); a.setAlpha(alpha);
    a.setKernelSize(btv_ksize); a.setBlurKernelSize(blur_ksize); a.setBlurSigma(blur_sigma);
}

class ListSource : public cv::superres::FrameSource {
public:
    std::vector<GpuMat> frames;
    size_t pos = 0;
    void nextFrame(cv::OutputArray frame) CV_OVERRIDE
    {
        if (pos >= frames.size()) { frame.release(); return; }
        frames[pos++].copyTo(frame.getGpuMatRef());
    }
    void reset() CV_OVERRIDE { pos = 0; }
};

// opticalFlow_->calc(frame0, frame1, flowx, flowy): the k-th call returns the k-th given flow; which two frames were asked for is recorded
class ReplayFlow : public cv::superres::DenseOpticalFlowExt {
public:
    const std::vector<GpuMat> *frames = nullptr;
    std::vector<GpuMat> flows;   // 2 planes per call
    std::vector<int> calls;      // (index of frame0, index of frame1) per call, -1 = not one of the frames
    int index_of(const GpuMat &m) const
    {
        const size_t rb = (size_t)m.cols * cv::elem_size_of(m.type());
        for (size_t i = 0; i < frames->size(); ++i) {
            const GpuMat &f = (*frames)[i];
            if (f.rows != m.rows || f.cols != m.cols || f.type() != m.type()) continue;
            bool same = true;
            for (int y = 0; y < m.rows && same; ++y) same = memcmp(f.ptr<unsigned char>(y), m.ptr<unsigned char>(y), rb) == 0;
            if (same) return (int)i;
        }
        return -1;
    }
    void calc(cv::InputArray frame0, cv::InputArray frame1, cv::OutputArray flow1, cv::OutputArray flow2) CV_OVERRIDE
    {
        const size_t k = calls.size() / 2;
        calls.push_back(index_of(frame0.getGpuMat()));
        calls.push_back(index_of(frame1.getGpuMat()));
        if (2 * k + 1 >= flows.size()) throw std::runtime_error("more flow requests than flows given");
        flows[2 * k].copyTo(flow1.getGpuMatRef());
        flows[2 * k + 1].copyTo(flow2.getGpuMatRef());
    }
    void collectGarbage() CV_OVERRIDE {}
};
}  // namespace

// what superres/src/input_array_utility.cpp and optical_flow.cpp would supply (both need the main repo's Mat / UMat / video modules)
void cv::superres::arrCopy(InputArray src, OutputArray dst) { src.getGpuMat().copyTo(dst.getGpuMatRef()); }
cv::Ptr<cv::superres::FarnebackOpticalFlow> cv::superres::createOptFlow_Farneback() { return cv::Ptr<cv::superres::FarnebackOpticalFlow>(); }

#define REF_TRY try {
#define REF_CATCH return 0; } catch (const std::exception &) { return 1; }

extern "C" {
/* ---- steps: the wrappers of btv_l1_gpu.cu and the helpers of btv_l1_cuda.cpp's unnamed namespace ---- */
int ref_cuhost_btv_motion_maps(const float *fx, const float *fy, const float *bx, const float *by, int rows, int cols, float *fmx, float *fmy,
                               float *bmx, float *bmy)
{
    REF_TRY
    std::pair<GpuMat, GpuMat> f(up(fx, rows, cols, 1), up(fy, rows, cols, 1)), b(up(bx, rows, cols, 1), up(by, rows, cols, 1)), fm, bm;
    buildMotionMaps(f, b, fm, bm);
    down(fm.first, fmx); down(fm.second, fmy); down(bm.first, bmx); down(bm.second, bmy);
    REF_CATCH
}
int ref_cuhost_btv_upscale(const float *src, int rows, int cols, int cn, int scale, float *dst)
{
    REF_TRY
    GpuMat s = up(src, rows, cols, cn), d;
    cv::cuda::Stream st;
    upscale(s, d, scale, st);
    down(d, dst);
    REF_CATCH
}
int ref_cuhost_btv_diff_sign(const float *a, const float *b, int rows, int cols, int cn, float *dst)
{
    REF_TRY
    GpuMat s1 = up(a, rows, cols, cn), s2 = up(b, rows, cols, cn), d;
    cv::cuda::Stream st;
    diffSign(s1, s2, d, st);
    down(d, dst);
    REF_CATCH
}
/* weights: what calcBtvWeights would have loaded (count floats); the kernel then runs as calcBtvRegularization runs it */
int ref_cuhost_btv_regularization(const float *src, int rows, int cols, int cn, int btv_ksize, const float *weights, int count, float *dst)
{
    REF_TRY
    btv_l1_cudev::loadBtvWeights(weights, (size_t)count);
    GpuMat s = up(src, rows, cols, cn), d;
    calcBtvRegularization(s, d, btv_ksize);
    down(d, dst);
    REF_CATCH
}
/* calcBtvWeights(btvKernelSize, alpha, btvWeights): out has btvKernelSize^2 floats (the vector's size; only the enumerated ones are set) */
int ref_cuhost_btv_weights(int btv_ksize, double alpha, float *out)
{
    REF_TRY
    std::vector<float> w;
    calcBtvWeights(btv_ksize, alpha, w);
    memcpy(out, w.data(), sizeof(float) * w.size());
    REF_CATCH
}
/* upscaleMotions(lowRes, highRes, scale) of n motion pairs; out: n * 2 planes of (rows * scale) x (cols * scale) */
int ref_cuhost_btv_upscale_motions(const float *m, int n, int rows, int cols, int scale, float *out)
{
    REF_TRY
    std::vector<int> present(n, 1);
    Motions lo = motions(m, present.data(), n, rows, cols), hi;
    upscaleMotions(lo, hi, scale);
    const size_t plane = (size_t)rows * scale * cols * scale;
    for (int i = 0; i < n; ++i) { down(hi[i].first, out + (size_t)(2 * i) * plane); down(hi[i].second, out + (size_t)(2 * i + 1) * plane); }
    REF_CATCH
}
/* calcRelativeMotions: out_f / out_b: n * 2 planes each */
int ref_cuhost_btv_relative_motions(const float *fwd, const int *fwd_present, const float *bwd, const int *bwd_present, int n, int rows, int cols,
                                    int base, float *out_f, float *out_b)
{
    REF_TRY
    Motions f = motions(fwd, fwd_present, n, rows, cols), b = motions(bwd, bwd_present, n, rows, cols), rf, rb;
    calcRelativeMotions(f, b, rf, rb, base, cv::Size(cols, rows));
    const size_t plane = (size_t)rows * cols;
    for (int i = 0; i < n; ++i) {
        down(rf[i].first, out_f + (size_t)(2 * i) * plane); down(rf[i].second, out_f + (size_t)(2 * i + 1) * plane);
        down(rb[i].first, out_b + (size_t)(2 * i) * plane); down(rb[i].second, out_b + (size_t)(2 * i + 1) * plane);
    }
    REF_CATCH
}
/* ---- the cv::cuda functions the class calls ---- */
int ref_cuhost_gaussian_kernel(int n, double sigma, float *out)
{
    REF_TRY
    cv::Mat k = cv::getGaussianKernel(n, sigma, CV_32F);
    memcpy(out, k.ptr<float>(0), sizeof(float) * n);
    REF_CATCH
}
/* cuda::createGaussianFilter(type, -1, Size(ksize, ksize), sigma)->apply(src, dst, stream), as btv_l1_cuda.cpp:324,371 */
int ref_cuhost_gauss_filter(const float *src, int rows, int cols, int cn, int ksize, double sigma, float *dst)
{
    REF_TRY
    GpuMat s = up(src, rows, cols, cn), d;
    cv::Ptr<cv::cuda::Filter> f = cv::cuda::createGaussianFilter(s.type(), -1, cv::Size(ksize, ksize), sigma);
    cv::cuda::Stream st;
    f->apply(s, d, st);
    down(d, dst);
    REF_CATCH
}
/* cuda::createSeparableLinearFilter(type, -1, k, k)->apply(src, dst, stream) with an arbitrary kernel of n taps (anchor n / 2,
 * BORDER_DEFAULT): what createGaussianFilter builds, without the symmetry of a Gaussian -- tap order and anchor show */
int ref_cuhost_separable_filter(const float *src, int rows, int cols, int cn, const float *k, int n, float *dst)
{
    REF_TRY
    GpuMat s = up(src, rows, cols, cn), d;
    cv::Mat kernel(cv::Size(1, n), CV_32FC1, (void *)k);
    cv::Ptr<cv::cuda::Filter> f = cv::cuda::createSeparableLinearFilter(s.type(), -1, kernel, kernel);
    cv::cuda::Stream st;
    f->apply(s, d, st);
    down(d, dst);
    REF_CATCH
}
/* cuda::resize(src, dst, Size(dcols, drows), 0, 0, interpolation[, a stream of its own]) */
int ref_cuhost_resize(const float *src, int rows, int cols, int cn, int drows, int dcols, int interpolation, int own_stream, float *dst)
{
    REF_TRY
    GpuMat s = up(src, rows, cols, cn), d;
    cv::cuda::Stream st;
    cv::cuda::resize(s, d, cv::Size(dcols, drows), 0, 0, interpolation, own_stream ? st : cv::cuda::Stream::Null());
    down(d, dst);
    REF_CATCH
}
/* cuda::remap(src, dst, mapx, mapy, INTER_NEAREST, BORDER_REPLICATE, Scalar(), a stream of its own), as btv_l1_cuda.cpp:369,382 */
int ref_cuhost_remap_nearest_replicate(const float *src, int rows, int cols, int cn, const float *mapx, const float *mapy, int mrows, int mcols,
                                       float *dst)
{
    REF_TRY
    GpuMat s = up(src, rows, cols, cn), mx = up(mapx, mrows, mcols, 1), my = up(mapy, mrows, mcols, 1), d;
    cv::cuda::Stream st;
    cv::cuda::remap(s, d, mx, my, cv::INTER_NEAREST, cv::BORDER_REPLICATE, cv::Scalar(), st);
    down(d, dst);
    REF_CATCH
}

/* ---- BTVL1_CUDA_Base::process on an object that lives across calls ---- */
void *ref_cuhost_btvl1_new(void) { try { return new BTVL1_CUDA(); } catch (const std::exception &) { return nullptr; } }
void ref_cuhost_btvl1_delete(void *h) { delete static_cast<BTVL1_CUDA *>(h); }
/* frames: n dense rows x cols x cn float images; fwd / bwd: n pairs of planes with their present flags; out: (rows * scale - 2 btv) x
 * (cols * scale - 2 btv) x cn floats; weights_out (may be NULL): btvWeights_ after the call, btv_ksize^2 floats.  1 if the class threw. */
int ref_cuhost_btvl1_process(void *h, const float *frames, int n, int rows, int cols, int cn, const float *fwd, const int *fwd_present,
                             const float *bwd, const int *bwd_present, int base, int scale, int iterations, double tau, double lambda, double alpha,
                             int btv_ksize, int blur_ksize, double blur_sigma, float *out, float *weights_out)
{
    REF_TRY
    BTVL1_CUDA &alg = *static_cast<BTVL1_CUDA *>(h);
    set_params(alg, scale, iterations, tau, lambda, alpha, btv_ksize, blur_ksize, blur_sigma);
    std::vector<GpuMat> src(n);
    for (int i = 0; i < n; ++i) src[i] = up(frames + (size_t)i * rows * cols * cn, rows, cols, cn);
    Motions f = motions(fwd, fwd_present, n, rows, cols), b = motions(bwd, bwd_present, n, rows, cols);
    GpuMat dst;
    alg.process(src, dst, f, b, base);
    if (dst.rows != rows * scale - 2 * btv_ksize || dst.cols != cols * scale - 2 * btv_ksize || dst.type() != src[0].type()) return 2;
    down(dst, out);
    if (weights_out) memcpy(weights_out, alg.btvWeights_.data(), sizeof(float) * alg.btvWeights_.size());
    REF_CATCH
}

/* ---- the whole class: createSuperResolution_BTVL1_CUDA(), setInput(list of frames), setOpticalFlow(replay), nextFrame until it returns
 * nothing.  frames: n images, type 0 = CV_8U, 1 = CV_32F, cn channels; flows: nflows pairs of rows x cols planes, handed out in call order.
 * out: room for max_out frames of (rows * scale - 2 btv) x (cols * scale - 2 btv) x cn bytes; *n_out = frames returned before the first empty
 * one (at most max_out calls are made; *ended = 1 if an empty frame was seen, and a further call was empty again); calls: 2 ints per flow
 * request (indices of frame0, frame1), *n_calls of them.  1 if the class threw. */
int ref_cuhost_btvl1_sequence(const void *frames, int n, int rows, int cols, int cn, int type, const float *flows, int nflows, int radius, int scale,
                              int iterations, double tau, double lambda, double alpha, int btv_ksize, int blur_ksize, double blur_sigma,
                              unsigned char *out, int max_out, int *n_out, int *ended, int *calls, int max_calls, int *n_calls)
{
    *n_out = *ended = *n_calls = 0;
    REF_TRY
    cv::Ptr<cv::superres::SuperResolution> alg = cv::superres::createSuperResolution_BTVL1_CUDA();
    set_params(*alg, scale, iterations, tau, lambda, alpha, btv_ksize, blur_ksize, blur_sigma);
    alg->setTemporalAreaRadius(radius);
    cv::Ptr<ListSource> source = cv::makePtr<ListSource>();
    const size_t fsz = (size_t)rows * cols * cn;
    for (int i = 0; i < n; ++i)
        source->frames.push_back(type == 0 ? up8((const unsigned char *)frames + i * fsz, rows, cols, cn) : up((const float *)frames + i * fsz, rows, cols, cn));
    cv::Ptr<ReplayFlow> flow = cv::makePtr<ReplayFlow>();
    flow->frames = &source->frames;
    for (int i = 0; i < 2 * nflows; ++i) flow->flows.push_back(up(flows + (size_t)i * rows * cols, rows, cols, 1));
    alg->setOpticalFlow(flow);
    alg->setInput(source);
    const int orows = rows * scale - 2 * btv_ksize, ocols = cols * scale - 2 * btv_ksize;
    int rc = 0;
    for (int i = 0; i < max_out; ++i) {
        GpuMat o;
        alg->nextFrame(o);
        if (o.empty()) {
            GpuMat again;
            alg->nextFrame(again);
            *ended = again.empty() ? 1 : 0;
            break;
        }
        if (o.rows != orows || o.cols != ocols || o.type() != CV_MAKETYPE(CV_8U, cn)) { rc = 2; break; }
        down(o, out + (size_t)*n_out * orows * ocols * cn);
        ++*n_out;
    }
    *n_calls = (int)flow->calls.size() / 2;
    for (int i = 0; i < (int)flow->calls.size() && i < 2 * max_calls; ++i) calls[i] = flow->calls[i];
    if (rc) return rc;
    REF_CATCH
}
}
