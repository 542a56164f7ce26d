// cv::cuda::FarnebackOpticalFlow: handle, the executor of a call's plan (fb_plan.h) and C-ABI entry points.  Host-side twin of
// FarnebackOpticalFlowImpl (modules/cudaoptflow/src/farneback.cpp:96-492), ordered on ONE stream (the
// reference fans out over 5 streams and blocks the host once per level, :319-324,366,456).
#include "farneback_dev.h"
#include "mi_selftest.h"
#include "tvl1_dev.h"   // tvl1::resize == cuda::resize(INTER_LINEAR) on dense f32 planes
#include <cfloat>
#include <cmath>
#include <vector>

using namespace mi;
using namespace mi::fb;

namespace mi { namespace fb {

// cv::getGaussianKernel(n, sigma, CV_32F) (main repo imgproc): fixed tables for n <= 7 with sigma <= 0,
// else exp(-x^2/(2 sigma^2)) normalised to sum 1
void gaussian_kernel(int n, double sigma, float *k)
{
    static const float t1[] = {1.f}, t3[] = {0.25f, 0.5f, 0.25f}, t5[] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f},
                       t7[] = {0.03125f, 0.109375f, 0.21875f, 0.28125f, 0.21875f, 0.109375f, 0.03125f};
    if (sigma <= 0 && n <= 7 && (n & 1)) {
        const float *t = n == 1 ? t1 : n == 3 ? t3 : n == 5 ? t5 : t7;
        for (int i = 0; i < n; ++i) k[i] = t[i];
        return;
    }
    const double sx = sigma > 0 ? sigma : ((n - 1) * 0.5 - 1) * 0.3 + 0.8;
    const double scale2 = -0.5 / (sx * sx);
    std::vector<double> w(n);
    double sum = 0;
    for (int i = 0; i < n; ++i) { const double x = i - (n - 1) * 0.5; w[i] = std::exp(scale2 * x * x); sum += w[i]; }
    for (int i = 0; i < n; ++i) k[i] = (float)(w[i] / sum);
}

// prepareGaussian, farneback.cpp:209-260: Gaussian-weighted moments and the 4 used entries of inv(G)
int prepare_gaussian(int n, double sigma, PolyC *C)
{
    if (sigma < FLT_EPSILON) sigma = n * 0.3;   // :270-271
    float gb[17], *g = gb + 8;
    double s = 0.;
    for (int x = -n; x <= n; x++) { g[x] = (float)std::exp(-x * x / (2 * sigma * sigma)); s += g[x]; }
    s = 1. / s;
    memset(C, 0, sizeof(*C));
    for (int x = -n; x <= n; x++) {
        g[x] = (float)(g[x] * s);
        if (x >= 0) { C->g[x] = g[x]; C->xg[x] = (float)(x * g[x]); C->xxg[x] = (float)(x * x * g[x]); }
    }
    double G[6][6] = {{0}};
    for (int y = -n; y <= n; y++)
        for (int x = -n; x <= n; x++) {
            G[0][0] += g[y] * g[x];
            G[1][1] += g[y] * g[x] * x * x;
            G[3][3] += g[y] * g[x] * x * x * x * x;
            G[5][5] += g[y] * g[x] * x * x * y * y;
        }
    G[2][2] = G[0][3] = G[0][4] = G[3][0] = G[4][0] = G[1][1];
    G[4][4] = G[3][3];
    G[3][4] = G[4][3] = G[5][5];
    // inv(G) by Cholesky (Mat::inv(DECOMP_CHOLESKY), :254)
    double L[6][6] = {{0}}, inv[6][6];
    for (int i = 0; i < 6; ++i)
        for (int j = 0; j <= i; ++j) {
            double a = G[i][j];
            for (int k = 0; k < j; ++k) a -= L[i][k] * L[j][k];
            if (i == j) { if (a <= 0) { set_error("moment matrix is not positive definite"); return MI_ERR_BAD_ARG; } L[i][i] = std::sqrt(a); }
            else L[i][j] = a / L[j][j];
        }
    for (int c = 0; c < 6; ++c) {
        double yv[6], xv[6];
        for (int i = 0; i < 6; ++i) { double a = i == c ? 1.0 : 0.0; for (int k = 0; k < i; ++k) a -= L[i][k] * yv[k]; yv[i] = a / L[i][i]; }
        for (int i = 5; i >= 0; --i) { double a = yv[i]; for (int k = i + 1; k < 6; ++k) a -= L[k][i] * xv[k]; xv[i] = a / L[i][i]; }
        for (int i = 0; i < 6; ++i) inv[i][c] = xv[i];
    }
    C->ig11 = (float)inv[1][1]; C->ig03 = (float)inv[0][3]; C->ig33 = (float)inv[3][3]; C->ig55 = (float)inv[5][5];
    return MI_OK;
}

}}  // namespace mi::fb

struct mi_farneback {
    mi_farneback_params P;
    DevBuf<float> arena;        // capB per-pair blocks (FbLayout, fb_plan.h): every plane of pair b lives at (plane of pair 0) + b * bs
    int capW = 0, capH = 0, capB = 0;
    // internal stream + events of the two-chain pair groups (chain 1 of the plan).  ONE calc in flight per handle: a handle used from two host
    // threads, or on two streams without a synchronisation in between, races on the arena AND on this stream's ordering (c_api.h).
    Event ev_join, ev_fork;
    Stream aux;   // (declared last: it goes first, drained, then the events, then the arena)
    ~mi_farneback() { if (aux.get()) (void)hipStreamSynchronize(aux.get()); }
};

extern "C" {

void mi_farneback_default_params(mi_farneback_params *p)
{
    if (!p) return;
    // cv::cuda::FarnebackOpticalFlow::create defaults, cudaoptflow.hpp:285-293
    p->num_levels = 5; p->pyr_scale = 0.5; p->fast_pyramids = 0; p->win_size = 13; p->num_iters = 10;
    p->poly_n = 5; p->poly_sigma = 1.1; p->flags = 0;
}

static int validate(const mi_farneback_params *p)
{
    MI_REQUIRE(p, MI_ERR_BAD_ARG, "null params");
    MI_REQUIRE(p->poly_n == 5 || p->poly_n == 7, MI_ERR_BAD_ARG, "polyN must be 5 or 7");                                   // farneback.cpp:316
    MI_REQUIRE(!p->fast_pyramids || std::abs(p->pyr_scale - 0.5) < 1e-6, MI_ERR_BAD_ARG, "fastPyramids requires pyrScale == 0.5");  // :317
    MI_REQUIRE(p->num_levels >= 0 && p->num_levels <= 32, MI_ERR_BAD_ARG, "numLevels out of range");
    MI_REQUIRE(p->pyr_scale > 0 && p->pyr_scale < 1, MI_ERR_BAD_ARG, "pyrScale must be in (0,1)");
    MI_REQUIRE(p->win_size >= 1 && (p->win_size & 1) && p->win_size / 2 <= MI_FB_MAX_KSIZE_HALF, MI_ERR_BAD_ARG, "winSize must be odd and <= 201");
    MI_REQUIRE(p->num_iters >= 0, MI_ERR_BAD_ARG, "numIters must be >= 0");
    return MI_OK;
}

int mi_farneback_create(const mi_farneback_params *p, mi_farneback **out)
{
    MI_REQUIRE(out, MI_ERR_BAD_ARG, "null out");
    *out = nullptr;
    mi_farneback_params d;
    if (!p) { mi_farneback_default_params(&d); p = &d; }
    MI_TRY(require_device());
    mi_farneback *h = new mi_farneback();
    h->P = *p;   // validated at calc(), like the reference (CV_Assert inside calcImpl)
    *out = h;
    return MI_OK;
}

int mi_farneback_set_params(mi_farneback *h, const mi_farneback_params *p)
{
    MI_REQUIRE(h && p, MI_ERR_BAD_ARG, "null argument");
    h->P = *p;
    return MI_OK;
}

int mi_farneback_get_params(const mi_farneback *h, mi_farneback_params *p)
{
    MI_REQUIRE(h && p, MI_ERR_BAD_ARG, "null argument");
    *p = h->P;
    return MI_OK;
}

void mi_farneback_destroy(mi_farneback *h) { delete h; }

static int ensure(mi_farneback *h, int W, int H, int B)
{
    if (h->arena.p && h->capW == W && h->capH == H && h->capB >= B) return MI_OK;
    h->arena.release();   // another frame size or a larger batch: re-made (not only grown)
    MI_TRY(h->arena.ensure((size_t)fb_layout(W, H).bs * (size_t)B));
    h->capW = W; h->capH = H; h->capB = B;
    return MI_OK;
}

static void geo_tvl1(const Plane &p, mi::tvl1::Geo &g) { g.w = p.w; g.h = p.h; g.ld = p.ld; g.ps = p.batch > 1 ? p.bs : (long long)p.ld * p.h; g.batch = p.batch; }

// cuda::resize(src -> dst, Size(dw,dh), INTER_LINEAR) followed by convertTo(*alpha) on up to 2 planes
static int resize2(const float *s0, const float *s1, const Plane &gs, float *d0, float *d1, const Plane &gd, float alpha, hipStream_t st)
{
    if (gs.w == gd.w && gs.h == gd.h && alpha == 1.f) {   // dsize == src.size(): copy (cudawarping/src/resize.cpp:89-93)
        const size_t bytes = sizeof(float) * (size_t)gs.ld * gs.h, pitch = sizeof(float) * (size_t)(gs.batch > 1 ? gs.bs : (long long)gs.ld * gs.h);
        MI_HIP_TRY(hipMemcpy2DAsync(d0, pitch, s0, pitch, bytes, (size_t)gs.batch, hipMemcpyDeviceToDevice, st));
        if (s1) MI_HIP_TRY(hipMemcpy2DAsync(d1, pitch, s1, pitch, bytes, (size_t)gs.batch, hipMemcpyDeviceToDevice, st));
        return MI_OK;
    }
    mi::tvl1::Geo a, b;
    geo_tvl1(gs, a); geo_tvl1(gd, b);
    const float *src[3][2] = {{s0, nullptr}, {s1, nullptr}, {nullptr, nullptr}};
    float *dst[3] = {d0, d1, nullptr};
    const float post[3] = {alpha, alpha, 1.f};
    return mi::tvl1::resize(MI_SEM_CUDA_COMPAT, s1 ? 2 : 1, src, 1, dst, a, b, (double)gd.w / gs.w, (double)gd.h / gs.h, post, nullptr, 0, st);
}

static int check_pair(const mi_mat *I0, const mi_mat *I1, const mi_mat *flow, const mi_mat *ref)
{
    MI_REQUIRE(I0 && I1 && flow && I0->data && I1->data && flow->data, MI_ERR_BAD_ARG, "null matrix");
    // CV_Assert(frame0.channels() == 1 && frame1.channels() == 1)  farneback.cpp:173; depths supported here: 8U, 32F
    MI_REQUIRE((I0->type == MI_8UC1 || I0->type == MI_32FC1) && I1->type == I0->type, MI_ERR_BAD_TYPE, "frames must be CV_8UC1 or CV_32FC1, same type");
    MI_REQUIRE(I0->rows == I1->rows && I0->cols == I1->cols, MI_ERR_BAD_SIZE, "frame0.size() != frame1.size()");   // :174
    MI_REQUIRE(flow->type == MI_32FC2 && flow->rows == I0->rows && flow->cols == I0->cols, MI_ERR_BAD_SIZE, "flow must be CV_32FC2 of the frame size");  // :181-182
    MI_REQUIRE(flow->step % 8 == 0 && ((uintptr_t)flow->data % 8) == 0, MI_ERR_BAD_ARG, "flow must be 8-byte aligned");
    if (I0->type == MI_32FC1) MI_REQUIRE(I0->step % 4 == 0 && I1->step % 4 == 0, MI_ERR_BAD_ARG, "float frames must be 4-byte aligned");
    MI_REQUIRE(I0->rows == ref->rows && I0->cols == ref->cols && I0->type == ref->type, MI_ERR_BAD_SIZE, "all pairs of a batch must share size and type");
    return MI_OK;
}

// the caller's matrices of n pairs as the by-value table of a batched format step (b == nullptr: one matrix per pair)
static FmtTab fmt_tab(const mi_mat *a, const mi_mat *b, int n)
{
    FmtTab T;
    memset(&T, 0, sizeof(T));
    for (int j = 0; j < n; ++j) {
        T.a[j] = a[j].data; T.sa[j] = (long long)a[j].step;
        if (b) { T.b[j] = b[j].data; T.sb[j] = (long long)b[j].step; }
    }
    return T;
}

// centre + positive half of cv::getGaussianKernel(n, sigma)
static Taps half_taps(int n, double sigma)
{
    std::vector<float> k(n);
    gaussian_kernel(n, sigma, k.data());
    Taps K;
    memset(&K, 0, sizeof(K));
    for (int i = 0; i <= n / 2; ++i) K.k[i] = k[n / 2 + i];
    return K;
}

// n independent pairs per launch sequence: blockIdx.z = pair in every kernel of the level loop (a 640 x 480 pair alone is about
// 70 launches of 5-50 us, i.e. launch-latency bound; batched, the same 70 launches carry n pairs).
// Every decision of the call is the plan's (fb_plan.h: levels, forms, scratch layout, the ordered launches and their chains; unit-tested
// without a device).  Here: validation, the host constants, and ONE loop that turns the plan's offsets into pointers and launches.
int mi_farneback_calc_batch(mi_farneback *h, int nb, const mi_mat *I0s, const mi_mat *I1s, mi_mat *flows, void *stream)
{
    MI_REQUIRE(h, MI_ERR_BAD_ARG, "null handle");
    MI_REQUIRE(nb > 0 && I0s && I1s && flows, MI_ERR_BAD_ARG, "empty batch");
    hipStream_t st = (hipStream_t)stream;
    const mi_farneback_params &P = h->P;
    int rc = validate(&P);
    if (rc) return rc;
    for (int i = 0; i < nb; ++i) if ((rc = check_pair(&I0s[i], &I1s[i], &flows[i], &I0s[0]))) return rc;
    const int W = I0s[0].cols, H = I0s[0].rows, B = nb, type = I0s[0].type;
    MI_REQUIRE(W >= 2 && H >= 2, MI_ERR_BAD_SIZE, "frames too small");

    FbKnobs knobs = fb_knobs();
    {   // groups alternate over two streams only while the caller's stream is NOT being captured (a captured graph stays one chain);
        // asked once per call
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        if (knobs.chains == 2 && (hipStreamIsCapturing(st, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone)) { (void)hipGetLastError(); knobs.chains = 1; }
    }
    const bool gauss = (P.flags & MI_OPTFLOW_FARNEBACK_GAUSSIAN) != 0;
    const FbShape shape = {W, H, B, P.num_levels, P.pyr_scale, P.fast_pyramids != 0, P.num_iters, (P.flags & MI_OPTFLOW_USE_INITIAL_FLOW) != 0, P.win_size, P.poly_n};
    const FbPlan plan = fb_make_plan(shape, knobs);
    for (int k = 0; k <= plan.levels; ++k)
        MI_REQUIRE(plan.lv[k].smooth / 2 <= MI_FB_MAX_KSIZE_HALF, MI_ERR_BAD_ARG, "pyramid smoothing kernel too large (MAX_KSIZE_HALF)");
    if ((rc = ensure(h, W, H, B))) return rc;

    // host constants: setPolynomialExpansionConsts :361, the Gaussian window of the iterations :460-464, each level's pre-blur :434-446
    PolyC C;
    if ((rc = prepare_gaussian(P.poly_n, P.poly_sigma, &C))) return rc;
    const Taps wk = gauss ? half_taps(P.win_size, (double)(P.win_size / 2 * 0.3f)) : Taps();
    std::vector<Taps> blur_taps(P.fast_pyramids ? 0 : plan.levels + 1);
    for (size_t k = 0; k < blur_taps.size(); ++k) blur_taps[k] = half_taps(plan.lv[k].smooth, plan.lv[k].sigma);

    const FbLayout &A = plan.lay;
    const long long pn = A.pn, bs = A.bs;
    const Plane g0s = plane_of(W, H);   // single-pair view for the per-pair format kernels
    const float zoom_alpha = (float)(1. / P.pyr_scale);
    // an error return between a fork and its join still orders the caller's stream behind whatever the internal one was given
    struct ChainJoin {
        hipStream_t st, aux; hipEvent_t ev; bool armed;
        ~ChainJoin() { if (armed) { (void)hipEventRecord(ev, aux); (void)hipStreamWaitEvent(st, ev, 0); } }
    } chain_join = {st, nullptr, nullptr, false};
    for (const FbLaunch &l : plan.launches) {
        const FbLevel &L = plan.lv[l.level], &Lc = plan.lv[std::min(l.level + 1, plan.levels)], &Lf = plan.lv[std::max(l.level - 1, 0)];   // the level, the coarser, the finer
        hipStream_t sx = l.chain ? h->aux.get() : st;
        float *const pb = h->arena.p + (long long)l.b0 * bs;   // the block of the group's first pair
        const Plane g = plane_of(L.w, L.h, bs, l.nb), gf = plane_of(W, H, bs, l.nb), gc = plane_of(Lc.w, Lc.h, bs, l.nb);
        float *const fx = pb + L.flow, *const fy = fx + pn, *const cx = pb + Lc.flow, *const cy = cx + pn;
        float *const frames = pb + A.frames, *const blurred = pb + A.blurred, *const lvl = pb + A.lvl;
        float *const R0 = pb + A.R, *const R1 = R0 + 5 * pn;
        float *const Min = pb + (l.flip ? A.bufM : A.M), *const Mout = pb + (l.flip ? A.M : A.bufM);
        void *const mg = l.writes_merged ? flows[0].data : nullptr;
        const long long mg_step = l.writes_merged ? (long long)flows[0].step : 0;
        switch (l.op) {
        case FB_CONVERT:   // convertTo(CV_32F), farneback.cpp:342-345
            rc = l.form ? convert_batch(fmt_tab(I0s + l.b0, I1s + l.b0, l.nb), l.nb, type, frames, frames + pn, bs, g0s, sx)
                        : convert(I0s[0].data, (long long)I0s[0].step, I1s[0].data, (long long)I1s[0].step, type, frames, frames + pn, g0s, sx);
            break;
        case FB_SPLIT_FLOW: rc = split_flow(flows[l.b0].data, (long long)flows[l.b0].step, fx, fy, g0s, sx); break;
        case FB_PYR_DOWN: rc = pyr_down(pb + Lf.img[l.iter], plane_of(Lf.w, Lf.h, bs, l.nb), pb + L.img[l.iter], g, sx); break;
        case FB_INIT_RESIZE: rc = resize2(pb + A.flow[0], pb + A.flow[0] + pn, gf, fx, fy, g, (float)L.scale, sx); break;
        case FB_CLEAR_FLOW: {
            const size_t bytes = sizeof(float) * (size_t)g.ld * g.h, pitch = sizeof(float) * (size_t)bs;
            if (l.form == 1) MI_HIP_TRY(hipMemset2DAsync(fx, pitch, 0, sizeof(float) * (size_t)pn + bytes, (size_t)l.nb, sx));
            else {
                MI_HIP_TRY(hipMemset2DAsync(fx, pitch, 0, bytes, (size_t)l.nb, sx));
                MI_HIP_TRY(hipMemset2DAsync(fy, pitch, 0, bytes, (size_t)l.nb, sx));
            }
        } break;
        case FB_ZOOM: rc = resize2(cx, cy, gc, fx, fy, g, zoom_alpha, sx); break;
        case FB_BLUR: rc = gaussian_blur(frames, blurred, gf, L.smooth / 2, blur_taps[l.level], MI_BORDER_REFLECT101, sx, 2, pn, (BlurForm)l.form); break;
        case FB_BLUR_DIRECT:
            rc = gaussian_blur_tab(fmt_tab(I0s + l.b0, I1s + l.b0, l.nb), type, blurred, gf, L.smooth / 2, blur_taps[l.level], sx, pn);
            break;
        case FB_LEVEL_RESIZE: rc = resize2(blurred, blurred + pn, gf, lvl, lvl + pn, g, 1.f, sx); break;
        case FB_POLY_EXP: rc = poly_exp(pb + L.img[0], R0, g, P.poly_n, C, sx, 2, L.img[1] - L.img[0], 5 * pn, nullptr, (PolyForm)l.form); break;
        case FB_POLY_EXP_RESIZED: rc = poly_exp(blurred, R0, g, P.poly_n, C, sx, 2, pn, 5 * pn, &gf, (PolyForm)l.form); break;
        case FB_UPDATE_MATRICES: rc = update_matrices(L.zero_flow ? nullptr : fx, L.zero_flow ? nullptr : fy, R0, R1, pb + A.M, g, sx); break;
        case FB_UPDATE_MATRICES_ZOOM: rc = update_matrices_resized(cx, cy, gc, zoom_alpha, fx, fy, R0, R1, pb + A.M, g, sx); break;
        case FB_ITERATE: rc = iterate(Min, R0, R1, fx, fy, Mout, g, P.win_size, gauss ? &wk : nullptr, l.update, sx, mg, mg_step, (IterForm)l.form); break;
        case FB_ITERATE2: rc = iterate2(Min, R0, R1, fx, fy, Mout, g, P.win_size, gauss ? &wk : nullptr, l.update, sx, mg, mg_step); break;
        case FB_MERGE:   // cuda::merge :197-198
            rc = l.form ? merge_flow_batch(fx, fy, fmt_tab(flows + l.b0, nullptr, l.nb), l.nb, bs, g0s, sx)
                        : merge_flow(fx, fy, flows[l.b0].data, (long long)flows[l.b0].step, g0s, sx);
            break;
        case FB_FORK:
            MI_TRY(h->aux.ensure());
            MI_TRY(h->ev_fork.ensure());
            MI_TRY(h->ev_join.ensure());
            MI_HIP_TRY(hipEventRecord(h->ev_fork.get(), st));
            MI_HIP_TRY(hipStreamWaitEvent(h->aux.get(), h->ev_fork.get(), 0));
            chain_join.aux = h->aux.get(); chain_join.ev = h->ev_join.get(); chain_join.armed = true;
            break;
        case FB_JOIN:
            chain_join.armed = false;
            MI_HIP_TRY(hipEventRecord(h->ev_join.get(), h->aux.get()));
            MI_HIP_TRY(hipStreamWaitEvent(st, h->ev_join.get(), 0));
            break;
        }
        if (rc) return rc;
    }
    return MI_OK;
}


int mi_farneback_calc(mi_farneback *h, const mi_mat *I0, const mi_mat *I1, mi_mat *flow, void *stream)
{
    return mi_farneback_calc_batch(h, 1, I0, I1, flow, stream);
}

// test hook (mi_selftest.h): NaNs over the whole arena
int miflow_selftest_farneback_poison(mi_farneback *h, void *stream)
{
    MI_REQUIRE(h && h->arena.p, MI_ERR_BAD_ARG, "no arena yet: run a calc first");
    MI_HIP_TRY(hipMemsetAsync(h->arena.p, 0xff, sizeof(float) * (size_t)fb_layout(h->capW, h->capH).bs * (size_t)h->capB, (hipStream_t)stream));
    return MI_OK;
}

}  // extern "C"

// ------------------------------------------------------------------ stage-level entry points
namespace {
int check_f32(const mi_mat *m, const char *name)
{
    MI_REQUIRE(m && m->data, MI_ERR_BAD_ARG, "%s: null matrix", name);
    MI_REQUIRE(m->type == MI_32FC1, MI_ERR_BAD_TYPE, "%s: must be CV_32FC1", name);
    MI_REQUIRE(m->rows > 0 && m->cols > 0, MI_ERR_BAD_SIZE, "%s: empty", name);
    MI_REQUIRE(m->step >= (size_t)m->cols * 4 && m->step % 4 == 0, MI_ERR_BAD_ARG, "%s: bad step", name);
    return MI_OK;
}
// rows x cols matrix (rows may be 5*h) -> dense plane(s) with pitch ld
int stage_in(DevTmp &S, const mi_mat *m, int ld, float **out, hipStream_t st)
{
    float *p;
    MI_TRY(S.alloc(&p, (size_t)ld * m->rows));
    MI_HIP_TRY(hipMemcpy2DAsync(p, (size_t)ld * 4, m->data, m->step, (size_t)m->cols * 4, (size_t)m->rows, hipMemcpyDeviceToDevice, st));
    *out = p;
    return MI_OK;
}
int stage_out(const float *p, int ld, mi_mat *m, hipStream_t st)
{
    MI_HIP_TRY(hipMemcpy2DAsync(m->data, m->step, p, (size_t)ld * 4, (size_t)m->cols * 4, (size_t)m->rows, hipMemcpyDeviceToDevice, st));
    return MI_OK;
}
int make_win_taps(int ksize, Taps *K)
{
    MI_REQUIRE(ksize >= 1 && (ksize & 1) && ksize / 2 <= MI_FB_MAX_KSIZE_HALF, MI_ERR_BAD_ARG, "ksize must be odd and <= 201");
    *K = half_taps(ksize, (double)(ksize / 2 * 0.3f));
    return MI_OK;
}
}  // namespace

extern "C" {

int mi_farneback_poly_exp(const mi_mat *src, mi_mat *dst5, int poly_n, double poly_sigma, void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    MI_TRY(check_f32(src, "src")); MI_TRY(check_f32(dst5, "dst"));
    MI_REQUIRE(dst5->rows == 5 * src->rows && dst5->cols == src->cols, MI_ERR_BAD_SIZE, "dst must be 5*rows x cols");
    MI_REQUIRE(poly_n == 5 || poly_n == 7, MI_ERR_BAD_ARG, "polyN must be 5 or 7");
    const Plane g = plane_of(src->cols, src->rows);
    DevTmp S;
    float *in = nullptr, *out;
    MI_TRY(S.alloc(&out, (size_t)g.ld * g.h * 5));
    MI_TRY(stage_in(S, src, g.ld, &in, st));
    PolyC C;
    MI_TRY(prepare_gaussian(poly_n, poly_sigma, &C));
    MI_TRY(poly_exp(in, out, g, poly_n, C, st));
    MI_TRY(stage_out(out, g.ld, dst5, st));
    MI_HIP_TRY(hipStreamSynchronize(st));
    return MI_OK;
}

int mi_farneback_update_matrices(const mi_mat *flowx, const mi_mat *flowy, const mi_mat *R0, const mi_mat *R1, mi_mat *M5, void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    MI_TRY(check_f32(flowx, "flowx")); MI_TRY(check_f32(flowy, "flowy")); MI_TRY(check_f32(R0, "R0")); MI_TRY(check_f32(R1, "R1")); MI_TRY(check_f32(M5, "M"));
    const int w = flowx->cols, hh = flowx->rows;
    MI_REQUIRE(flowy->rows == hh && flowy->cols == w && R0->rows == 5 * hh && R1->rows == 5 * hh && M5->rows == 5 * hh &&
               R0->cols == w && R1->cols == w && M5->cols == w, MI_ERR_BAD_SIZE, "size mismatch");
    const Plane g = plane_of(w, hh);
    DevTmp S;
    float *fx, *fy, *r0, *r1, *m;
    MI_TRY(S.alloc(&m, (size_t)g.ld * hh * 5));
    MI_TRY(stage_in(S, flowx, g.ld, &fx, st)); MI_TRY(stage_in(S, flowy, g.ld, &fy, st));
    MI_TRY(stage_in(S, R0, g.ld, &r0, st)); MI_TRY(stage_in(S, R1, g.ld, &r1, st));
    MI_TRY(update_matrices(fx, fy, r0, r1, m, g, st));
    MI_TRY(stage_out(m, g.ld, M5, st));
    MI_HIP_TRY(hipStreamSynchronize(st));
    return MI_OK;
}

int mi_farneback_blur5(const mi_mat *M5, mi_mat *dst5, int ksize, int gaussian, void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    MI_TRY(check_f32(M5, "M")); MI_TRY(check_f32(dst5, "dst"));
    MI_REQUIRE(M5->rows % 5 == 0 && dst5->rows == M5->rows && dst5->cols == M5->cols, MI_ERR_BAD_SIZE, "size mismatch");
    const Plane g = plane_of(M5->cols, M5->rows / 5);
    Taps K;
    MI_TRY(make_win_taps(ksize, &K));
    DevTmp S;
    float *m, *out;
    MI_TRY(S.alloc(&out, (size_t)g.ld * g.h * 5));
    MI_TRY(stage_in(S, M5, g.ld, &m, st));
    MI_TRY(blur5(m, out, g, ksize, gaussian ? &K : nullptr, st));
    MI_TRY(stage_out(out, g.ld, dst5, st));
    MI_HIP_TRY(hipStreamSynchronize(st));
    return MI_OK;
}

int mi_farneback_update_flow(const mi_mat *M5, mi_mat *flowx, mi_mat *flowy, void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    MI_TRY(check_f32(M5, "M")); MI_TRY(check_f32(flowx, "flowx")); MI_TRY(check_f32(flowy, "flowy"));
    MI_REQUIRE(M5->rows == 5 * flowx->rows && M5->cols == flowx->cols && flowy->rows == flowx->rows && flowy->cols == flowx->cols,
               MI_ERR_BAD_SIZE, "size mismatch");
    const Plane g = plane_of(flowx->cols, flowx->rows);
    DevTmp S;
    float *m, *fx, *fy;
    MI_TRY(S.alloc(&fx, (size_t)g.ld * g.h)); MI_TRY(S.alloc(&fy, (size_t)g.ld * g.h));
    MI_TRY(stage_in(S, M5, g.ld, &m, st));
    MI_TRY(update_flow(m, fx, fy, g, st));
    MI_TRY(stage_out(fx, g.ld, flowx, st)); MI_TRY(stage_out(fy, g.ld, flowy, st));
    MI_HIP_TRY(hipStreamSynchronize(st));
    return MI_OK;
}

int mi_farneback_iterate(const mi_mat *M5, const mi_mat *R0, const mi_mat *R1, mi_mat *flowx, mi_mat *flowy, mi_mat *M5out,
                         int ksize, int gaussian, int update, void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    MI_TRY(check_f32(M5, "M")); MI_TRY(check_f32(R0, "R0")); MI_TRY(check_f32(R1, "R1")); MI_TRY(check_f32(flowx, "flowx")); MI_TRY(check_f32(flowy, "flowy"));
    MI_TRY(check_f32(M5out, "Mout"));
    const int w = flowx->cols, hh = flowx->rows;
    MI_REQUIRE(flowy->rows == hh && flowy->cols == w && M5->rows == 5 * hh && R0->rows == 5 * hh && R1->rows == 5 * hh && M5out->rows == 5 * hh &&
               M5->cols == w && R0->cols == w && R1->cols == w && M5out->cols == w, MI_ERR_BAD_SIZE, "size mismatch");
    MI_REQUIRE(M5->data != M5out->data, MI_ERR_BAD_ARG, "Mout must not alias M");
    const Plane g = plane_of(w, hh);
    Taps K;
    MI_TRY(make_win_taps(ksize, &K));
    DevTmp S;
    float *m, *r0, *r1, *fx, *fy, *mo;
    MI_TRY(S.alloc(&fx, (size_t)g.ld * hh)); MI_TRY(S.alloc(&fy, (size_t)g.ld * hh)); MI_TRY(S.alloc(&mo, (size_t)g.ld * hh * 5));
    MI_TRY(stage_in(S, M5, g.ld, &m, st)); MI_TRY(stage_in(S, R0, g.ld, &r0, st)); MI_TRY(stage_in(S, R1, g.ld, &r1, st));
    MI_HIP_TRY(hipMemsetAsync(mo, 0, sizeof(float) * (size_t)g.ld * hh * 5, st));
    MI_TRY(iterate(m, r0, r1, fx, fy, mo, g, ksize, gaussian ? &K : nullptr, update != 0, st));
    MI_TRY(stage_out(fx, g.ld, flowx, st)); MI_TRY(stage_out(fy, g.ld, flowy, st)); MI_TRY(stage_out(mo, g.ld, M5out, st));
    MI_HIP_TRY(hipStreamSynchronize(st));
    return MI_OK;
}

int mi_farneback_gaussian_blur(const mi_mat *src, mi_mat *dst, int ksize, double sigma, int border, void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    MI_TRY(check_f32(src, "src")); MI_TRY(check_f32(dst, "dst"));
    MI_REQUIRE(dst->rows == src->rows && dst->cols == src->cols, MI_ERR_BAD_SIZE, "size mismatch");
    MI_REQUIRE(ksize >= 1 && (ksize & 1) && ksize / 2 <= MI_FB_MAX_KSIZE_HALF, MI_ERR_BAD_ARG, "ksize must be odd and <= 201");
    const Plane g = plane_of(src->cols, src->rows);
    const Taps K = half_taps(ksize, sigma);
    DevTmp S;
    float *in, *out;
    MI_TRY(S.alloc(&out, (size_t)g.ld * g.h));
    MI_TRY(stage_in(S, src, g.ld, &in, st));
    MI_TRY(gaussian_blur(in, out, g, ksize / 2, K, border, st));
    MI_TRY(stage_out(out, g.ld, dst, st));
    MI_HIP_TRY(hipStreamSynchronize(st));
    return MI_OK;
}

int mi_pyr_down(const mi_mat *src, mi_mat *dst, void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    MI_TRY(check_f32(src, "src")); MI_TRY(check_f32(dst, "dst"));
    MI_REQUIRE(dst->rows == (src->rows + 1) / 2 && dst->cols == (src->cols + 1) / 2, MI_ERR_BAD_SIZE, "dst must be ((rows+1)/2, (cols+1)/2)");
    const Plane gs = plane_of(src->cols, src->rows), gd = plane_of(dst->cols, dst->rows);
    DevTmp S;
    float *in, *out;
    MI_TRY(S.alloc(&out, (size_t)gd.ld * gd.h));
    MI_TRY(stage_in(S, src, gs.ld, &in, st));
    MI_TRY(pyr_down(in, gs, out, gd, st));
    MI_TRY(stage_out(out, gd.ld, dst, st));
    MI_HIP_TRY(hipStreamSynchronize(st));
    return MI_OK;
}

}  // extern "C"

// ------------------------------------------------------------------ one named launch form per call (test hooks, mi_selftest.h)
extern "C" {

int miflow_selftest_farneback_iterate(int form, const mi_mat *M5, const mi_mat *R0, const mi_mat *R1, mi_mat *flowx, mi_mat *flowy, mi_mat *M5out,
                                      mi_mat *merged, int ksize, int gaussian, int update, void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    MI_REQUIRE(form >= MI_FB_ITER_ROW && form <= MI_FB_ITER_PAIR, MI_ERR_BAD_ARG, "unknown iterate form %d", form);
    MI_TRY(check_f32(M5, "M")); MI_TRY(check_f32(R0, "R0")); MI_TRY(check_f32(R1, "R1")); MI_TRY(check_f32(flowx, "flowx")); MI_TRY(check_f32(flowy, "flowy"));
    MI_TRY(check_f32(M5out, "Mout"));
    const int w = flowx->cols, hh = flowx->rows;
    MI_REQUIRE(flowy->rows == hh && flowy->cols == w && M5->rows == 5 * hh && R0->rows == 5 * hh && R1->rows == 5 * hh && M5out->rows == 5 * hh &&
               M5->cols == w && R0->cols == w && R1->cols == w && M5out->cols == w, MI_ERR_BAD_SIZE, "size mismatch");
    MI_REQUIRE(M5->data != M5out->data, MI_ERR_BAD_ARG, "Mout must not alias M");
    if (merged) {
        MI_REQUIRE(merged->data && merged->type == MI_32FC2 && merged->rows == hh && merged->cols == w, MI_ERR_BAD_SIZE, "merged must be CV_32FC2 of the flow size");
        MI_REQUIRE(merged->step >= (size_t)w * 8 && merged->step % 8 == 0 && ((uintptr_t)merged->data % 8) == 0, MI_ERR_BAD_ARG, "merged must be 8-byte aligned");
    }
    const Plane g = plane_of(w, hh);
    Taps K;
    MI_TRY(make_win_taps(ksize, &K));
    DevTmp S;
    float *m, *r0, *r1, *fx, *fy, *mo;
    MI_TRY(S.alloc(&fx, (size_t)g.ld * hh)); MI_TRY(S.alloc(&fy, (size_t)g.ld * hh));
    MI_TRY(stage_in(S, M5, g.ld, &m, st)); MI_TRY(stage_in(S, R0, g.ld, &r0, st)); MI_TRY(stage_in(S, R1, g.ld, &r1, st));
    MI_TRY(stage_in(S, M5out, g.ld, &mo, st));
    void *const mg = merged ? merged->data : nullptr;
    const long long mstep = merged ? (long long)merged->step : 0;
    int rc;   // (a form that cannot write the merged flow is the launcher's MI_ERR_BAD_ARG)
    if (form == MI_FB_ITER_PAIR) rc = iterate2(m, r0, r1, fx, fy, mo, g, ksize, gaussian ? &K : nullptr, update != 0, st, mg, mstep);
    else rc = iterate(m, r0, r1, fx, fy, mo, g, ksize, gaussian ? &K : nullptr, update != 0, st, mg, mstep, (IterForm)form);
    if (rc == MI_OK) rc = stage_out(fx, g.ld, flowx, st);
    if (rc == MI_OK) rc = stage_out(fy, g.ld, flowy, st);
    if (rc == MI_OK) rc = stage_out(mo, g.ld, M5out, st);
    MI_HIP_TRY(hipStreamSynchronize(st));   // also on an error return: the staging copies read the caller's matrices
    return rc;
}

int miflow_selftest_farneback_poly_exp(int form, const mi_mat *src, mi_mat *dst5, int poly_n, double poly_sigma, void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    MI_REQUIRE(form >= MI_FB_POLY_ROW && form <= MI_FB_POLY_RESIZED, MI_ERR_BAD_ARG, "unknown poly_exp form %d", form);
    MI_TRY(check_f32(src, "src")); MI_TRY(check_f32(dst5, "dst"));
    MI_REQUIRE(dst5->rows % 5 == 0, MI_ERR_BAD_SIZE, "dst must be 5 stacked planes");
    const bool rs = form == MI_FB_POLY_RESIZED;
    const bool same = dst5->rows == 5 * src->rows && dst5->cols == src->cols;
    MI_REQUIRE(rs || same, MI_ERR_BAD_SIZE, "dst must be 5*rows x cols");
    MI_REQUIRE(!rs || !same, MI_ERR_BAD_SIZE, "the resized form takes a source of another size");
    MI_REQUIRE(poly_n == 5 || poly_n == 7, MI_ERR_BAD_ARG, "polyN must be 5 or 7");
    const Plane gs = plane_of(src->cols, src->rows), g = plane_of(dst5->cols, dst5->rows / 5);
    DevTmp S;
    float *in = nullptr, *out;
    MI_TRY(S.alloc(&out, (size_t)g.ld * g.h * 5));
    MI_TRY(stage_in(S, src, gs.ld, &in, st));
    PolyC C;
    MI_TRY(prepare_gaussian(poly_n, poly_sigma, &C));
    int rc = poly_exp(in, out, g, poly_n, C, st, 1, 0, 0, rs ? &gs : nullptr, form == MI_FB_POLY_TILED ? POLY_TILED : POLY_ROW);
    if (rc == MI_OK) rc = stage_out(out, g.ld, dst5, st);
    MI_HIP_TRY(hipStreamSynchronize(st));
    return rc;
}

int miflow_selftest_farneback_update_matrices(int form, const mi_mat *prevx, const mi_mat *prevy, float alpha, mi_mat *flowx, mi_mat *flowy,
                                              const mi_mat *R0, const mi_mat *R1, mi_mat *M5, void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    MI_REQUIRE(form >= MI_FB_UM_PLAIN && form <= MI_FB_UM_RESIZED, MI_ERR_BAD_ARG, "unknown update_matrices form %d", form);
    MI_TRY(check_f32(R0, "R0")); MI_TRY(check_f32(R1, "R1")); MI_TRY(check_f32(M5, "M"));
    MI_REQUIRE(M5->rows % 5 == 0, MI_ERR_BAD_SIZE, "M must be 5 stacked planes");
    const int w = M5->cols, hh = M5->rows / 5;
    MI_REQUIRE(R0->rows == 5 * hh && R1->rows == 5 * hh && R0->cols == w && R1->cols == w, MI_ERR_BAD_SIZE, "size mismatch");
    if (form != MI_FB_UM_ZERO) {
        MI_TRY(check_f32(flowx, "flowx")); MI_TRY(check_f32(flowy, "flowy"));
        MI_REQUIRE(flowx->rows == hh && flowx->cols == w && flowy->rows == hh && flowy->cols == w, MI_ERR_BAD_SIZE, "size mismatch");
    }
    const Plane g = plane_of(w, hh);
    DevTmp S;
    float *fx = nullptr, *fy = nullptr, *r0, *r1, *m;
    MI_TRY(S.alloc(&m, (size_t)g.ld * hh * 5));
    MI_TRY(stage_in(S, R0, g.ld, &r0, st)); MI_TRY(stage_in(S, R1, g.ld, &r1, st));
    int rc;
    if (form == MI_FB_UM_RESIZED) {
        MI_TRY(check_f32(prevx, "prevx")); MI_TRY(check_f32(prevy, "prevy"));
        MI_REQUIRE(prevy->rows == prevx->rows && prevy->cols == prevx->cols, MI_ERR_BAD_SIZE, "size mismatch");
        const Plane gp = plane_of(prevx->cols, prevx->rows);
        float *px, *py;
        MI_TRY(stage_in(S, prevx, gp.ld, &px, st)); MI_TRY(stage_in(S, prevy, gp.ld, &py, st));
        MI_TRY(S.alloc(&fx, (size_t)g.ld * hh)); MI_TRY(S.alloc(&fy, (size_t)g.ld * hh));
        rc = update_matrices_resized(px, py, gp, alpha, fx, fy, r0, r1, m, g, st);
        if (rc == MI_OK) rc = stage_out(fx, g.ld, flowx, st);
        if (rc == MI_OK) rc = stage_out(fy, g.ld, flowy, st);
    } else {
        if (form == MI_FB_UM_PLAIN) { MI_TRY(stage_in(S, flowx, g.ld, &fx, st)); MI_TRY(stage_in(S, flowy, g.ld, &fy, st)); }
        rc = update_matrices(fx, fy, r0, r1, m, g, st);
    }
    if (rc == MI_OK) rc = stage_out(m, g.ld, M5, st);
    MI_HIP_TRY(hipStreamSynchronize(st));
    return rc;
}

int miflow_selftest_farneback_gaussian_blur(int form, const mi_mat *src0, const mi_mat *src1, mi_mat *dst0, mi_mat *dst1, int ksize, double sigma,
                                            int border, void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    MI_REQUIRE(form >= MI_FB_BLUR_GENERIC_FAST && form <= MI_FB_BLUR_TABLE, MI_ERR_BAD_ARG, "unknown blur form %d", form);
    MI_REQUIRE(ksize >= 1 && (ksize & 1) && ksize / 2 <= MI_FB_MAX_KSIZE_HALF, MI_ERR_BAD_ARG, "ksize must be odd and <= 201");
    MI_TRY(check_f32(dst0, "dst"));
    const Plane g = plane_of(dst0->cols, dst0->rows);
    const size_t pn = (size_t)g.ld * g.h;
    const Taps K = half_taps(ksize, sigma);
    DevTmp S;
    float *in, *out;
    MI_TRY(S.alloc(&out, pn * 2));
    int rc;
    if (form == MI_FB_BLUR_TABLE) {
        MI_TRY(check_f32(dst1, "dst1"));
        MI_REQUIRE(src0 && src1 && src0->data && src1->data, MI_ERR_BAD_ARG, "null matrix");
        MI_REQUIRE((src0->type == MI_8UC1 || src0->type == MI_32FC1) && src1->type == src0->type, MI_ERR_BAD_TYPE, "sources must be CV_8UC1 or CV_32FC1, same type");
        MI_REQUIRE(src0->rows == g.h && src0->cols == g.w && src1->rows == g.h && src1->cols == g.w && dst1->rows == g.h && dst1->cols == g.w, MI_ERR_BAD_SIZE, "size mismatch");
        if (src0->type == MI_32FC1) MI_REQUIRE(src0->step % 4 == 0 && src1->step % 4 == 0, MI_ERR_BAD_ARG, "float sources must be 4-byte aligned");
        MI_REQUIRE(border == MI_BORDER_REFLECT101, MI_ERR_BAD_ARG, "the direct-source blur is REFLECT101 only");
        FmtTab T;
        memset(&T, 0, sizeof(T));
        T.a[0] = src0->data; T.sa[0] = (long long)src0->step;
        T.b[0] = src1->data; T.sb[0] = (long long)src1->step;
        rc = gaussian_blur_tab(T, src0->type, out, g, ksize / 2, K, st, (long long)pn);
        if (rc == MI_OK) rc = stage_out(out + pn, g.ld, dst1, st);
    } else {
        MI_TRY(check_f32(src0, "src"));
        MI_REQUIRE(src0->rows == g.h && src0->cols == g.w, MI_ERR_BAD_SIZE, "size mismatch");
        MI_TRY(stage_in(S, src0, g.ld, &in, st));
        rc = gaussian_blur(in, out, g, ksize / 2, K, border, st, 1, 0,
                           form == MI_FB_BLUR_TILED ? BLUR_TILED : form == MI_FB_BLUR_GENERIC_FULL ? BLUR_GENERIC_FULL : BLUR_GENERIC_FAST);
    }
    if (rc == MI_OK) rc = stage_out(out, g.ld, dst0, st);
    MI_HIP_TRY(hipStreamSynchronize(st));
    return rc;
}

}  // extern "C"
