// BTV-L1 super-resolution behind the C-ABI (include/miflow/c_api.h): handle, scratch arena, host tables and the launch sequence of
// cv::superres::BTVL1_CUDA_Base::process (superres/src/btv_l1_cuda.cpp:306-400).  Kernels: btvl1_kernels.hip.
#include <cmath>
#include <cstdlib>
#include "btvl1_dev.h"
#include "mi_selftest.h"

using namespace mi;
using namespace mi::btvl1;

struct mi_btvl1 {
    mi_btvl1_params P;
    DevBuf<unsigned char> arena;      // every scratch plane of the last geometry (layout()); grown lazily, freed with the handle
    TimingEvent ev1, ev0;             // around the last process (mi_btvl1_get_profile)
    long long launches = 0;
    bool timed = false;
};

namespace {

// getGaussianKernel(n, sigma, CV_32F) (main repo imgproc; cudafilters/src/filtering.cpp:573): fixed tables for sigma <= 0 and odd
// n <= 7, else sigma = 0.3 ((n - 1) / 2 - 1) + 0.8; exp and the normalisation in double, stored f32.
void gaussian_taps(int n, double sigma, float *out)
{
    static const float small[4][7] = {{1.f}, {0.25f, 0.5f, 0.25f}, {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f},
                                      {0.03125f, 0.109375f, 0.21875f, 0.28125f, 0.21875f, 0.109375f, 0.03125f}};
    for (int i = 0; i < MAX_TAPS; ++i) out[i] = 0.f;
    if (sigma <= 0 && n % 2 == 1 && n <= 7) {
        for (int i = 0; i < n; ++i) out[i] = small[n >> 1][i];
        return;
    }
    const double s = sigma > 0 ? sigma : ((n - 1) * 0.5 - 1) * 0.3 + 0.8;
    const double scale2x = -0.5 / (s * s);
    double t[MAX_TAPS], sum = 0.0;
    for (int i = 0; i < n; ++i) {
        const double x = i - (n - 1) * 0.5;
        t[i] = std::exp(scale2x * x * x);
        sum += t[i];
    }
    const double inv = 1.0 / sum;
    for (int i = 0; i < n; ++i) out[i] = (float)(t[i] * inv);
}

// calcBtvWeights (btv_l1_cuda.cpp:171-187): std::pow(float, int) evaluates in double
void btv_weights(int btv_kernel_size, double alpha, float *out)
{
    for (int i = 0; i < MAX_WEIGHTS; ++i) out[i] = 0.f;
    const int ksize = (btv_kernel_size - 1) / 2;
    const float alpha_f = (float)alpha;
    for (int m = 0, ind = 0; m <= ksize; ++m)
        for (int l = ksize; l + m >= 0; --l, ++ind) out[ind] = (float)std::pow((double)alpha_f, (double)(std::abs(m) + std::abs(l)));
}

size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

// Arena layout for geometry g; returns the bytes needed.  Every block starts 256-byte aligned.
size_t layout(const Geo &g, unsigned char *base, Planes *p)
{
    const size_t lpx = (size_t)g.lw * g.lh, hpx = (size_t)g.hw * g.hh, K = (size_t)g.K;
    size_t off = 0;
    auto take = [&](size_t bytes) { unsigned char *q = base + off; off += up256(bytes); return q; };
    float *src = (float *)take(K * lpx * g.cn * 4);
    float *mot[4], *rel[4];
    for (int q = 0; q < 4; ++q) mot[q] = (float *)take(K * lpx * 4);
    for (int q = 0; q < 4; ++q) rel[q] = (float *)take(K * lpx * 4);
    unsigned *fidx = (unsigned *)take(K * hpx * 4), *bidx = (unsigned *)take(K * hpx * 4);
    float *X0 = (float *)take(hpx * g.cn * 4), *X1 = (float *)take(hpx * g.cn * 4);
    signed char *sgn = (signed char *)take(K * lpx * g.cn);
    if (p) {
        p->src = src;
        for (int q = 0; q < 4; ++q) { p->mot[q] = mot[q]; p->rel[q] = rel[q]; }
        p->fidx = fidx; p->bidx = bidx; p->X[0] = X0; p->X[1] = X1; p->sgn = sgn;
    }
    return off;
}

int check_params(const mi_btvl1_params &P)
{
    // CV_Asserts of process (btv_l1_cuda.cpp:310-316), of createGaussianFilter (filtering.cpp:568) and of the linear filters (:441)
    MI_REQUIRE(P.scale > 1, MI_ERR_BAD_ARG, "btvl1: scale > 1");
    MI_REQUIRE(P.iterations > 0, MI_ERR_BAD_ARG, "btvl1: iterations > 0");
    MI_REQUIRE(P.tau > 0.0 && P.alpha > 0.0, MI_ERR_BAD_ARG, "btvl1: tau > 0 && alpha > 0");
    MI_REQUIRE(P.btv_kernel_size > 0 && P.btv_kernel_size <= 16, MI_ERR_BAD_ARG, "btvl1: btvKernelSize > 0 && btvKernelSize <= 16");
    MI_REQUIRE(P.blur_kernel_size > 0 && P.blur_kernel_size % 2 == 1 && P.blur_kernel_size < MAX_TAPS, MI_ERR_BAD_ARG,
               "btvl1: blurKernelSize odd, 1 .. 31");
    MI_REQUIRE(P.blur_sigma >= 0.0, MI_ERR_BAD_ARG, "btvl1: blurSigma >= 0");
    return MI_OK;
}

// Validation + arena + input copies + the three set-up launches.  maps_f: see launch_maps.
int prepare(mi_btvl1 *h, int n, const mi_mat *frames, const mi_mat *fwd_x, const mi_mat *fwd_y, const mi_mat *bwd_x, const mi_mat *bwd_y,
            int base_idx, float *maps_f, IterArgs *A, hipStream_t st)
{
    MI_REQUIRE(h && frames && n >= 1, MI_ERR_BAD_ARG, "btvl1: null handle / frames or n < 1");
    MI_REQUIRE(base_idx >= 0 && base_idx < n, MI_ERR_BAD_ARG, "btvl1: 0 <= baseIdx < n");
    MI_REQUIRE(n == 1 || (fwd_x && fwd_y && bwd_x && bwd_y), MI_ERR_BAD_ARG, "btvl1: null motions");
    if (const int rc = check_params(h->P)) return rc;
    const mi_btvl1_params &P = h->P;
    const int type = frames[0].type;
    MI_REQUIRE(type == MI_32FC1 || type == MI_32FC3 || type == MI_32FC4, MI_ERR_BAD_TYPE, "btvl1: frames must be CV_32FC1 / C3 / C4");
    Geo g;
    g.cn = type == MI_32FC1 ? 1 : type == MI_32FC3 ? 3 : 4;
    g.lw = frames[0].cols; g.lh = frames[0].rows; g.K = n; g.scale = P.scale;
    MI_REQUIRE(g.lw > 0 && g.lh > 0, MI_ERR_BAD_SIZE, "btvl1: empty frame");
    const long long hw = (long long)g.lw * P.scale, hh = (long long)g.lh * P.scale;
    // map positions are packed 16 : 16, and v / scale is taken as __umulhi(v, ceil(2^32 / scale)), exact while (v + scale) scale < 2^32
    MI_REQUIRE(hw <= 65535 && hh <= 65535 && P.scale < 32768, MI_ERR_BAD_SIZE, "btvl1: high-res size above 65535");
    MI_REQUIRE(hw > 2LL * P.btv_kernel_size && hh > 2LL * P.btv_kernel_size, MI_ERR_BAD_SIZE,
               "btvl1: high-res frame not larger than the cropped border of btvKernelSize pixels");
    g.hw = (int)hw; g.hh = (int)hh;
    g.inv_scale = (unsigned)(((1ULL << 32) + (unsigned)P.scale - 1) / (unsigned)P.scale);
    for (int i = 0; i < n; ++i) {
        MI_REQUIRE(frames[i].data, MI_ERR_BAD_ARG, "btvl1: null frame data");
        MI_REQUIRE(frames[i].type == type, MI_ERR_BAD_TYPE, "btvl1: frames of different types");
        MI_REQUIRE(frames[i].rows == g.lh && frames[i].cols == g.lw, MI_ERR_BAD_SIZE, "btvl1: frames of different sizes");
        // forward[i] is read for i < n - 1, backward[i] for i > 0 (calcRelativeMotions, btv_l1_cuda.cpp:98-114)
        const mi_mat *used[4] = {i < n - 1 ? &fwd_x[i] : nullptr, i < n - 1 ? &fwd_y[i] : nullptr, i > 0 ? &bwd_x[i] : nullptr,
                                 i > 0 ? &bwd_y[i] : nullptr};
        for (const mi_mat *m : used) {
            if (!m) continue;
            MI_REQUIRE(m->data, MI_ERR_BAD_ARG, "btvl1: null motion data");
            MI_REQUIRE(m->type == MI_32FC1, MI_ERR_BAD_TYPE, "btvl1: motions must be CV_32FC1");
            MI_REQUIRE(m->rows == g.lh && m->cols == g.lw, MI_ERR_BAD_SIZE, "btvl1: motion size != frame size");
        }
    }
    const size_t need = layout(g, nullptr, nullptr);
    if (need > h->arena.n && h->arena.p) MI_HIP_TRY(hipStreamSynchronize(st));
    MI_TRY(h->arena.ensure(need));
    IterArgs &a = *A;
    a.g = g;
    layout(g, h->arena.p, &a.p);
    gaussian_taps(P.blur_kernel_size, P.blur_sigma, a.t.g);
    btv_weights(P.btv_kernel_size, P.alpha, a.t.w);
    a.kb = P.blur_kernel_size; a.ks = (P.btv_kernel_size - 1) / 2; a.cur = 0;
    a.use_btv = P.lambda > 0 ? 1 : 0;
    a.data_lds = data_lds_bytes(P.blur_kernel_size, P.scale) <= DATA_LDS_MAX ? 1 : 0;
    a.beta = (float)(-P.tau * P.lambda); a.tau = (float)P.tau;   // addWeighted casts its double scalars to f32 (add_weighted.cu:91-93)
    a.dst = nullptr; a.dstep = 0; a.crop = P.btv_kernel_size;

    const size_t lpx = (size_t)g.lw * g.lh, row = (size_t)g.lw * 4;
    for (int i = 0; i < n; ++i) {
        MI_HIP_TRY(hipMemcpy2DAsync((void *)(a.p.src + i * lpx * g.cn), row * g.cn, frames[i].data, frames[i].step, row * g.cn, g.lh,
                                    hipMemcpyDeviceToDevice, st));
        const mi_mat *m[4] = {i < n - 1 ? &fwd_x[i] : nullptr, i < n - 1 ? &fwd_y[i] : nullptr, i > 0 ? &bwd_x[i] : nullptr,
                              i > 0 ? &bwd_y[i] : nullptr};
        for (int q = 0; q < 4; ++q)
            if (m[q])
                MI_HIP_TRY(hipMemcpy2DAsync((void *)(a.p.mot[q] + i * lpx), row, m[q]->data, m[q]->step, row, g.lh, hipMemcpyDeviceToDevice, st));
    }
    launch_rel_motions(g, a.p, base_idx, st);
    launch_maps(g, a.p, maps_f, st);
    launch_init(g, a.p, base_idx, st);
    MI_HIP_TRY(hipGetLastError());
    h->launches = 3;
    return MI_OK;
}

}  // namespace

extern "C" {

void mi_btvl1_default_params(mi_btvl1_params *p)
{
    if (!p) return;
    // BTVL1_CUDA_Base::BTVL1_CUDA_Base, btv_l1_cuda.cpp:280-289
    p->scale = 4; p->iterations = 180; p->tau = 1.3; p->lambda = 0.03; p->alpha = 0.7;
    p->btv_kernel_size = 7; p->blur_kernel_size = 5; p->blur_sigma = 0.0;
}

int mi_btvl1_create(const mi_btvl1_params *p, mi_btvl1 **out)
{
    MI_REQUIRE(out, MI_ERR_BAD_ARG, "null out");
    *out = nullptr;
    mi_btvl1_params d;
    if (!p) { mi_btvl1_default_params(&d); p = &d; }
    MI_TRY(require_device());
    mi_btvl1 *h = new mi_btvl1();
    h->P = *p;   // validated at process(), like the reference (CV_Assert inside process)
    int rc = h->ev0.ensure();
    if (rc || (rc = h->ev1.ensure())) { delete h; return rc; }
    *out = h;
    return MI_OK;
}

int mi_btvl1_set_params(mi_btvl1 *h, const mi_btvl1_params *p)
{
    MI_REQUIRE(h && p, MI_ERR_BAD_ARG, "null argument");
    h->P = *p;
    return MI_OK;
}

int mi_btvl1_get_params(const mi_btvl1 *h, mi_btvl1_params *p)
{
    MI_REQUIRE(h && p, MI_ERR_BAD_ARG, "null argument");
    *p = h->P;
    return MI_OK;
}

void mi_btvl1_destroy(mi_btvl1 *h) { delete h; }

int mi_btvl1_process(mi_btvl1 *h, int n, const mi_mat *frames, const mi_mat *fwd_x, const mi_mat *fwd_y, const mi_mat *bwd_x,
                     const mi_mat *bwd_y, int base_idx, mi_mat *dst, void *stream)
{
    MI_REQUIRE(h && frames && dst && dst->data, MI_ERR_BAD_ARG, "mi_btvl1_process: null argument");
    MI_REQUIRE(n >= 1, MI_ERR_BAD_ARG, "mi_btvl1_process: n >= 1");
    if (const int rc = check_params(h->P)) return rc;
    const int b = h->P.btv_kernel_size, s = h->P.scale;
    MI_REQUIRE(dst->type == frames[0].type, MI_ERR_BAD_TYPE, "mi_btvl1_process: dst.type() == src[0].type()");
    MI_REQUIRE((long long)dst->rows == (long long)frames[0].rows * s - 2 * b && (long long)dst->cols == (long long)frames[0].cols * s - 2 * b,
               MI_ERR_BAD_SIZE, "mi_btvl1_process: dst must be the high-res size less a border of btvKernelSize pixels");
    hipStream_t st = (hipStream_t)stream;
    IterArgs A;
    h->timed = false;
    MI_HIP_TRY(hipEventRecord(h->ev0.get(), st));
    if (const int rc = prepare(h, n, frames, fwd_x, fwd_y, bwd_x, bwd_y, base_idx, nullptr, &A, st)) return rc;
    // two launches per iteration, no host wait in between; iteration i reads X[i & 1] and writes the other
    for (int i = 0; i < h->P.iterations; ++i) {
        A.cur = i & 1;
        if (i == h->P.iterations - 1) { A.dst = (unsigned char *)dst->data; A.dstep = dst->step; }
        launch_data(A, st);
        launch_update(A, st);
    }
    MI_HIP_TRY(hipGetLastError());
    h->launches += 2LL * h->P.iterations;
    MI_HIP_TRY(hipEventRecord(h->ev1.get(), st));
    h->timed = true;
    return MI_OK;
}

int mi_btvl1_get_profile(mi_btvl1 *h, double *ms, long long *launches)
{
    MI_REQUIRE(h && ms && launches, MI_ERR_BAD_ARG, "mi_btvl1_get_profile: null argument");
    MI_REQUIRE(h->timed, MI_ERR_BAD_ARG, "mi_btvl1_get_profile: no completed process call");
    MI_HIP_TRY(hipEventSynchronize(h->ev1.get()));
    float t = 0.f;
    MI_HIP_TRY(hipEventElapsedTime(&t, h->ev0.get(), h->ev1.get()));
    *ms = t;
    *launches = h->launches;
    return MI_OK;
}

int mi_btvl1_stage(mi_btvl1 *h, int n, const mi_mat *frames, const mi_mat *fwd_x, const mi_mat *fwd_y, const mi_mat *bwd_x,
                   const mi_mat *bwd_y, int base_idx, mi_mat *maps, mi_mat *initial, float *taps_host, float *weights_host, void *stream)
{
    MI_REQUIRE(h && frames && maps && initial && initial->data && taps_host && weights_host, MI_ERR_BAD_ARG, "mi_btvl1_stage: null argument");
    MI_REQUIRE(n >= 1, MI_ERR_BAD_ARG, "mi_btvl1_stage: n >= 1");
    if (const int rc = check_params(h->P)) return rc;
    const long long hw = (long long)frames[0].cols * h->P.scale, hh = (long long)frames[0].rows * h->P.scale;
    MI_REQUIRE(initial->type == frames[0].type, MI_ERR_BAD_TYPE, "mi_btvl1_stage: initial.type() == src[0].type()");
    MI_REQUIRE(initial->rows == hh && initial->cols == hw, MI_ERR_BAD_SIZE, "mi_btvl1_stage: initial must have the high-res size");
    for (int i = 0; i < 4 * n; ++i) {
        MI_REQUIRE(maps[i].data && maps[i].type == MI_32FC1, MI_ERR_BAD_TYPE, "mi_btvl1_stage: maps must be CV_32FC1");
        MI_REQUIRE(maps[i].rows == hh && maps[i].cols == hw, MI_ERR_BAD_SIZE, "mi_btvl1_stage: maps must have the high-res size");
    }
    hipStream_t st = (hipStream_t)stream;
    h->timed = false;
    DevTmp tmp;
    float *maps_f = nullptr;
    MI_TRY(tmp.alloc(&maps_f, (size_t)n * 4 * (size_t)hw * (size_t)hh));
    IterArgs A;
    if (const int rc = prepare(h, n, frames, fwd_x, fwd_y, bwd_x, bwd_y, base_idx, maps_f, &A, st)) return rc;
    const size_t hpx = (size_t)hw * hh;
    for (int i = 0; i < 4 * n; ++i)
        MI_HIP_TRY(hipMemcpy2DAsync(maps[i].data, maps[i].step, maps_f + i * hpx, (size_t)hw * 4, (size_t)hw * 4, (size_t)hh, hipMemcpyDeviceToDevice, st));
    const size_t rowb = (size_t)hw * A.g.cn * 4;
    MI_HIP_TRY(hipMemcpy2DAsync(initial->data, initial->step, A.p.X[0], rowb, rowb, (size_t)hh, hipMemcpyDeviceToDevice, st));
    MI_HIP_TRY(hipStreamSynchronize(st));   // tmp is freed on return
    memcpy(taps_host, A.t.g, sizeof(float) * MAX_TAPS);
    for (int i = 0; i < 256; ++i) weights_host[i] = i < MAX_WEIGHTS ? A.t.w[i] : 0.f;
    return MI_OK;
}

int mi_btvl1_convert(const mi_mat *src, mi_mat *dst, void *stream)
{
    MI_REQUIRE(src && dst && src->data && dst->data, MI_ERR_BAD_ARG, "mi_btvl1_convert: null matrix");
    const int sd = src->type & 7, dd = dst->type & 7, cn = ((src->type >> 3) & 63) + 1;
    MI_REQUIRE((sd == 0 || sd == 5) && (dd == 0 || dd == 5), MI_ERR_BAD_TYPE, "mi_btvl1_convert: depths CV_8U / CV_32F");
    MI_REQUIRE((cn == 1 || cn == 3 || cn == 4) && (dst->type >> 3) == (src->type >> 3), MI_ERR_BAD_TYPE,
               "mi_btvl1_convert: 1, 3 or 4 channels, the same on both sides");
    MI_REQUIRE(src->rows > 0 && src->cols > 0 && dst->rows == src->rows && dst->cols == src->cols, MI_ERR_BAD_SIZE, "mi_btvl1_convert: size mismatch");
    int ndev = 0;
    MI_REQUIRE(hipGetDeviceCount(&ndev) == hipSuccess && ndev > 0, MI_ERR_NO_DEVICE, "no HIP device");
    launch_convert(sd, dd, src->data, src->step, dst->data, dst->step, src->rows, src->cols * cn, (hipStream_t)stream);
    MI_HIP_TRY(hipGetLastError());
    return MI_OK;
}

int miflow_selftest_btvl1_poison(mi_btvl1 *h, void *stream)
{
    MI_REQUIRE(h && h->arena.p, MI_ERR_BAD_ARG, "no arena yet: run a process first");
    MI_HIP_TRY(hipMemsetAsync(h->arena.p, 0xff, h->arena.n, (hipStream_t)stream));
    return MI_OK;
}

}  // extern "C"
