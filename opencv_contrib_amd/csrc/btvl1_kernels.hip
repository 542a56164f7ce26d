// Device side of BTV-L1 super-resolution (cv::superres::BTVL1_CUDA_Base::process, superres/src/btv_l1_cuda.cpp:306-400).
//
// The reference runs an iteration as ~11 K + 3 launches over full high-res planes (per frame: remap, two-pass blur, nearest resize,
// diffSign, fill, zero-stuffing, two-pass blur, remap; then fill, BTV, K + 1 addWeighted).  Here it is two:
//   k_data    low-res pixel (y, x) of frame k: the blur is evaluated only where the nearest decimation samples it, (y s, x s);
//             its kb x kb taps are gathered from X through backwardMap_k (reflect-101 of the tap position, then the map, then
//             the replicate clamp), row sums first and then their combination, in the reference's order.
//   k_update  high-res pixel: BTV term of the old X from an LDS tile, then for k = 0 .. K-1 the blur of the ZERO-STUFFED sign field
//             at forwardMap_k(y, x).  Taps on a stuffed zero add +0 * g to a sum that is never -0 (it starts at +0 and a sign
//             sample is +-1 or +0), i.e. they leave every bit of it alone, and are skipped; the taps that reach a sign sample are
//             added in the reference's order, row sums first.
// Every value is the reference's sequence of separately rounded f32 operations (the library is built with -ffp-contract=off).
#include "btvl1_dev.h"

namespace mi {
namespace btvl1 {

// BrdReflect101::idx_col (main repo core/cuda/border_interpolate.hpp): idx_low(idx_high(i))
__device__ __forceinline__ int reflect101(int i, int n)
{
    if ((unsigned)i < (unsigned)n) return i;
    const int last = n - 1;
    const int hi = abs(last - abs(last - i)) % n;
    return abs(hi) % n;
}

// CubicFilter::bicubicCoeff == tvl1flow.cu:89-104 (Keys, a = -0.5)
__device__ __forceinline__ float bicubic_coeff(float x_)
{
    const float x = fabsf(x_);
    if (x <= 1.0f) return x * x * (1.5f * x - 2.5f) + 1.0f;
    else if (x < 2.0f) return x * (x * (-0.5f * x + 2.5f) - 4.0f) + 2.0f;
    return 0.0f;
}

// CubicFilter<BrdReplicate> at (sy, sx) of N values per position (main repo core/cuda/filters.hpp; the same gather is spelled out
// in-tree at tvl1flow.cu:118-148): taps ceil(s - 2) .. floor(s + 2), sum += w v, wsum += w, result sum / wsum.
template <int N, class Fetch>
__device__ __forceinline__ void cubic_at(float sy, float sx, int H, int W, Fetch fetch, float (&out)[N])
{
    const float xmin = ceilf(sx - 2.0f), xmax = floorf(sx + 2.0f);
    const float ymin = ceilf(sy - 2.0f), ymax = floorf(sy + 2.0f);
    float sum[N], wsum = 0.0f;
#pragma unroll
    for (int q = 0; q < N; ++q) sum[q] = 0.0f;
    for (float cy = ymin; cy <= ymax; cy += 1.0f) {
        const int iy = min(max((int)floorf(cy), 0), H - 1);
        const float wy = bicubic_coeff(sy - cy);
        for (float cx = xmin; cx <= xmax; cx += 1.0f) {
            const int ix = min(max((int)floorf(cx), 0), W - 1);
            const float w = bicubic_coeff(sx - cx) * wy;
            float v[N];
            fetch(iy, ix, v);
#pragma unroll
            for (int q = 0; q < N; ++q) sum[q] = sum[q] + w * v[q];
            wsum += w;
        }
    }
#pragma unroll
    for (int q = 0; q < N; ++q) out[q] = (wsum == 0.0f) ? 0.0f : sum[q] / wsum;
}

// calcRelativeMotions (btv_l1_cuda.cpp:80-115): running sums away from the base frame, in the reference's order.
__global__ __launch_bounds__(256) void k_rel_motions(Geo g, Planes p, int base)
{
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= g.lw || y >= g.lh) return;
    const size_t plane = (size_t)g.lw * g.lh, o = (size_t)y * g.lw + x;
    const float *fx = p.mot[0], *fy = p.mot[1], *bx = p.mot[2], *by = p.mot[3];
#pragma unroll
    for (int q = 0; q < 4; ++q) p.rel[q][base * plane + o] = 0.0f;
    float a[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int i = base - 1; i >= 0; --i) {
        a[0] = a[0] + fx[i * plane + o];
        a[1] = a[1] + fy[i * plane + o];
        a[2] = a[2] + bx[(i + 1) * plane + o];
        a[3] = a[3] + by[(i + 1) * plane + o];
#pragma unroll
        for (int q = 0; q < 4; ++q) p.rel[q][i * plane + o] = a[q];
    }
    a[0] = a[1] = a[2] = a[3] = 0.0f;
    for (int i = base + 1; i < g.K; ++i) {
        a[0] = a[0] + bx[i * plane + o];
        a[1] = a[1] + by[i * plane + o];
        a[2] = a[2] + fx[(i - 1) * plane + o];
        a[3] = a[3] + fy[(i - 1) * plane + o];
#pragma unroll
        for (int q = 0; q < 4; ++q) p.rel[q][i * plane + o] = a[q];
    }
}

// PointFilter + BrdReplicate of cuda::remap (remap.cu:57-69,256-260): truncate toward zero, then clamp; packed row << 16 | column
__device__ __forceinline__ unsigned map_pos(float mx, float my, int W, int H)
{
    const int ix = min(max((int)mx, 0), W - 1);   // v_cvt_i32_f32: toward zero, saturating
    const int iy = min(max((int)my, 0), H - 1);
    return ((unsigned)iy << 16) | (unsigned)ix;
}

// upscaleMotions + buildMotionMaps (btv_l1_cuda.cpp:117-144, btv_l1_gpu.cu:73-95) of frame blockIdx.z: the four relative-motion
// planes sampled by cuda::resize(INTER_CUBIC) at dst * float(1 / scale) (resize.cu:278-281), x scale, + pixel position.
// forwardMap is built from the BACKWARD motion and vice versa, as the reference does.
__global__ __launch_bounds__(256) void k_maps(Geo g, Planes p, float inv, float *maps_f)
{
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    const int k = blockIdx.z;
    if (x >= g.hw || y >= g.hh) return;
    const size_t lplane = (size_t)g.lw * g.lh, hplane = (size_t)g.hw * g.hh;
    const float *r0 = p.rel[0] + k * lplane, *r1 = p.rel[1] + k * lplane, *r2 = p.rel[2] + k * lplane, *r3 = p.rel[3] + k * lplane;
    const int lw = g.lw;
    float m[4];
    cubic_at<4>((float)y * inv, (float)x * inv, g.lh, g.lw,
                [&](int iy, int ix, float (&v)[4]) {
                    const size_t o = (size_t)iy * lw + ix;
                    v[0] = r0[o]; v[1] = r1[o]; v[2] = r2[o]; v[3] = r3[o];
                }, m);
    const float sc = (float)g.scale;
    const float fx = m[0] * sc, fy = m[1] * sc, bx = m[2] * sc, by = m[3] * sc;
    const float fmx = (float)x + bx, fmy = (float)y + by;   // forwardMap  = pixel + backward motion
    const float bmx = (float)x + fx, bmy = (float)y + fy;   // backwardMap = pixel + forward motion
    const size_t o = (size_t)y * g.hw + x;
    p.fidx[k * hplane + o] = map_pos(fmx, fmy, g.hw, g.hh);
    p.bidx[k * hplane + o] = map_pos(bmx, bmy, g.hw, g.hh);
    if (maps_f) {
        float *mf = maps_f + (size_t)k * 4 * hplane + o;
        mf[0] = fmx; mf[hplane] = fmy; mf[2 * hplane] = bmx; mf[3 * hplane] = bmy;
    }
}

// Initial estimate: cuda::resize(src[baseIdx], highResSize, INTER_CUBIC)  (btv_l1_cuda.cpp:354)
template <int CN>
__global__ __launch_bounds__(256) void k_init(Geo g, Planes p, float inv, int base)
{
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= g.hw || y >= g.hh) return;
    const float *S = p.src + (size_t)base * g.lw * g.lh * CN;
    const int lw = g.lw;
    float v[CN];
    cubic_at<CN>((float)y * inv, (float)x * inv, g.lh, g.lw,
                 [&](int iy, int ix, float (&t)[CN]) {
                     const float *q = S + ((size_t)iy * lw + ix) * CN;
#pragma unroll
                     for (int c = 0; c < CN; ++c) t[c] = q[c];
                 }, v);
    float *X = p.X[0] + ((size_t)y * g.hw + x) * CN;
#pragma unroll
    for (int c = 0; c < CN; ++c) X[c] = v[c];
}

// sign(src_k - resize_nearest(Gauss(remap(X, backwardMap_k))))  (btv_l1_cuda.cpp:369-375): the blur only at the decimated position
template <int CN>
__global__ __launch_bounds__(256) void k_data(IterArgs A)
{
    __shared__ float s_g[MAX_TAPS];
    extern __shared__ unsigned s_pos[];   // A.data_lds: per wave kb rows of the map positions its taps can reach
    if (threadIdx.x < MAX_TAPS) s_g[threadIdx.x] = A.t.g[threadIdx.x];
    const Geo &g = A.g;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int x = blockIdx.x * 64 + lane;
    const int y = blockIdx.y * 4 + wave;
    const int k = blockIdx.z;
    const int kb = A.kb, r = kb >> 1, hw = g.hw, hh = g.hh;
    // resize(INTER_NEAREST) down by an integer scale: src(trunc(y scale), trunc(x scale)), exactly (resize.cu:227-230)
    const int Y = y * g.scale, X = x * g.scale;
    const float *Xc = A.p.X[A.cur];
    const unsigned *bi = A.p.bidx + (size_t)k * hw * hh;
    // The tap positions of a wave (one low-res row, 64 pixels) form kb rows of one contiguous column span: the wave reads the packed
    // map positions there with consecutive lanes on consecutive columns and hands them out through LDS.  Read per tap, lanes are
    // `scale` columns apart and each of the kb loads of a row touches every cache line of the span again.
    const int span = 64 * g.scale + kb - 1;
    const unsigned *mine = s_pos + (size_t)wave * kb * span;
    if (A.data_lds && y < g.lh) {
        unsigned *w = s_pos + (size_t)wave * kb * span;
        const int c0 = blockIdx.x * 64 * g.scale - r;
        for (int j = 0; j < kb; ++j) {
            const size_t row = (size_t)reflect101(Y + j - r, hh) * hw;
            for (int c = lane; c < span; c += 64) w[j * span + c] = bi[row + reflect101(c0 + c, hw)];
        }
    }
    __syncthreads();
    if (x >= g.lw || y >= g.lh) return;
    // The kb x kb taps in chunks of TC: all map positions of a chunk are loaded first, then all values of X, then the sums are formed
    // tap by tap in the reference's order (a row sum is finished and folded into the column sum when its last tap has been added).
    // Walking the taps one at a time made every tap wait for two dependent loads in turn.
    constexpr int TC = CN == 1 ? 16 : 8;
    const int ntaps = kb * kb;
    float col[CN], rs[CN];
#pragma unroll
    for (int c = 0; c < CN; ++c) col[c] = rs[c] = 0.0f;
    int li = 0, lj = 0;   // tap whose position is loaded next
    int ai = 0, aj = 0;   // tap that is added next
    for (int t0 = 0; t0 < ntaps; t0 += TC) {
        unsigned q[TC];
#pragma unroll
        for (int u = 0; u < TC; ++u) {
            // taps past the last one yield a valid position too (reflect101 maps any index into the image); they are never added
            if (A.data_lds) {
                q[u] = mine[min(lj, kb - 1) * span + lane * g.scale + li];
            } else {
                const int ty = reflect101(Y + lj - r, hh), tx = reflect101(X + li - r, hw);
                q[u] = bi[(size_t)ty * hw + tx];
            }
            if (++li == kb) { li = 0; ++lj; }
        }
        float val[TC][CN];
#pragma unroll
        for (int u = 0; u < TC; ++u) {
            const float *px = Xc + ((size_t)(q[u] >> 16) * hw + (q[u] & 0xffffu)) * CN;
#pragma unroll
            for (int c = 0; c < CN; ++c) val[u][c] = px[c];
        }
#pragma unroll
        for (int u = 0; u < TC; ++u) {
            if (t0 + u < ntaps) {
                const float gi = s_g[ai];
#pragma unroll
                for (int c = 0; c < CN; ++c) rs[c] = rs[c] + val[u][c] * gi;
                if (++ai == kb) {
                    const float gj = s_g[aj];
#pragma unroll
                    for (int c = 0; c < CN; ++c) { col[c] = col[c] + rs[c] * gj; rs[c] = 0.0f; }
                    ai = 0; ++aj;
                }
            }
        }
    }
    const size_t o = (((size_t)k * g.lh + y) * g.lw + x) * CN;
#pragma unroll
    for (int c = 0; c < CN; ++c) {
        const float a = A.p.src[o + c], b = col[c];
        A.p.sgn[o + c] = a > b ? 1 : a < b ? -1 : 0;   // diffSign on reshape(1): every channel alike (btv_l1_cuda.cpp:168)
    }
}

__device__ __forceinline__ float diff_sign(float a, float b) { return a > b ? 1.0f : a < b ? -1.0f : 0.0f; }

// Blur of the zero-stuffed sign field S of one frame at high-res position (py, px), for any kernel length and scale: the loops over
// the taps that reach a sign sample (see the head of this file).  Returned by value: the sums stay in registers across the call.
template <int CN> struct Px { float c[CN]; };
template <int CN>
__device__ __noinline__ Px<CN> frame_term_loops(const signed char *S, const float *s_g, int py, int px, int kb, int s, unsigned inv, int lw, int hw,
                                                int hh)
{
    const int r = kb >> 1;
    float col[CN];
#pragma unroll
    for (int c = 0; c < CN; ++c) col[c] = 0.0f;
    if (py - r >= 0 && py + r < hh && px - r >= 0 && px + r < hw) {
        // no tap is reflected: walk the sign samples inside the window, i.e. the multiples of the scale
        const int wy0 = py - r, wx0 = px - r;
        const int qy = (int)__umulhi((unsigned)(wy0 + s - 1), inv), qx = (int)__umulhi((unsigned)(wx0 + s - 1), inv);
        for (int sy = qy, ty = qy * s; ty <= py + r; ++sy, ty += s) {
            float rs[CN];
#pragma unroll
            for (int c = 0; c < CN; ++c) rs[c] = 0.0f;
            for (int sx = qx, tx = qx * s; tx <= px + r; ++sx, tx += s) {
                const float gi = s_g[tx - wx0];
                const signed char *e = S + ((size_t)sy * lw + sx) * CN;
#pragma unroll
                for (int c = 0; c < CN; ++c) rs[c] = rs[c] + (float)e[c] * gi;
            }
            const float gj = s_g[ty - wy0];
#pragma unroll
            for (int c = 0; c < CN; ++c) col[c] = col[c] + rs[c] * gj;
        }
    } else {
        for (int j = 0; j < kb; ++j) {
            const int ty = reflect101(py + j - r, hh);
            const int sy = (int)__umulhi((unsigned)ty, inv);
            if (sy * s != ty) continue;   // a stuffed row: its row sum is +0
            float rs[CN];
#pragma unroll
            for (int c = 0; c < CN; ++c) rs[c] = 0.0f;
            for (int i = 0; i < kb; ++i) {
                const int tx = reflect101(px + i - r, hw);
                const int sx = (int)__umulhi((unsigned)tx, inv);
                if (sx * s != tx) continue;
                const float gi = s_g[i];
                const signed char *e = S + ((size_t)sy * lw + sx) * CN;
#pragma unroll
                for (int c = 0; c < CN; ++c) rs[c] = rs[c] + (float)e[c] * gi;
            }
            const float gj = s_g[j];
#pragma unroll
            for (int c = 0; c < CN; ++c) col[c] = col[c] + rs[c] * gj;
        }
    }
    Px<CN> out;
#pragma unroll
    for (int c = 0; c < CN; ++c) out.c[c] = col[c];
    return out;
}

enum { UT_W = 32, UT_H = 8, UT_HALO = 7 };   // update tile; BTV radius <= (16 - 1) / 2

// One iteration's update of the estimate (btv_l1_cuda.cpp:378-395): X' = X + (-tau lambda) BTV(X) + tau sum_k diffTerm_k, the
// terms added in the reference's order, each as addWeighted's a * alpha + b * beta + gamma (add_weighted.cu:69).
// NW = (kb - 1) / scale + 1, the sign samples a blur window can reach per axis, where that is at most 3 (class defaults: 2); 0 = any.
template <int CN, int NW>
__global__ __launch_bounds__(256) void k_update(IterArgs A)
{
    __shared__ float s_g[MAX_TAPS];
    __shared__ float s_x[(UT_H + 2 * UT_HALO) * (UT_W + 2 * UT_HALO) * CN];
    const Geo &g = A.g;
    const int hw = g.hw, hh = g.hh, ks = A.ks;
    const float *Xc = A.p.X[A.cur];
    if (threadIdx.x < MAX_TAPS) s_g[threadIdx.x] = A.t.g[threadIdx.x];
    const int tw = UT_W + 2 * ks, th = UT_H + 2 * ks;
    const int x0 = blockIdx.x * UT_W - ks, y0 = blockIdx.y * UT_H - ks;
    if (A.use_btv) {
        // tile of the old X with a halo of the BTV radius; positions outside the image are clamped (never used: pixels closer
        // than the radius to the border keep a zero term)
        for (int e = threadIdx.x; e < tw * th; e += 256) {
            const int ty = e / tw, tx = e - ty * tw;
            const int sy = min(max(y0 + ty, 0), hh - 1), sx = min(max(x0 + tx, 0), hw - 1);
            const float *q = Xc + ((size_t)sy * hw + sx) * CN;
#pragma unroll
            for (int c = 0; c < CN; ++c) s_x[e * CN + c] = q[c];
        }
    }
    __syncthreads();
    const int lx = threadIdx.x & 31, ly = threadIdx.x >> 5;
    const int x = blockIdx.x * UT_W + lx, y = blockIdx.y * UT_H + ly;
    if (x >= hw || y >= hh) return;
    const size_t o = ((size_t)y * hw + x) * CN;
    float v[CN];
#pragma unroll
    for (int c = 0; c < CN; ++c) v[c] = Xc[o + c];

    if (A.use_btv) {
        // calcBtvRegularizationKernel (btv_l1_gpu.cu:194-214); the four-channel diffSign yields 0 in the fourth channel (:157-165)
        float reg[CN];
#pragma unroll
        for (int c = 0; c < CN; ++c) reg[c] = 0.0f;
        if (y >= ks && y < hh - ks && x >= ks && x < hw - ks) {
            const float *ctr = s_x + ((ly + ks) * tw + (lx + ks)) * CN;
            int count = 0;
            for (int m = 0; m <= ks; ++m)
                for (int l = ks; l + m >= 0; --l, ++count) {
                    const float wgt = A.t.w[count];
                    const float *pp = ctr + (m * tw + l) * CN, *qq = ctr - (m * tw + l) * CN;
#pragma unroll
                    for (int c = 0; c < (CN == 4 ? 3 : CN); ++c)
                        reg[c] = reg[c] + wgt * (diff_sign(ctr[c], pp[c]) - diff_sign(qq[c], ctr[c]));
                }
        }
#pragma unroll
        for (int c = 0; c < CN; ++c) v[c] = (v[c] * 1.0f + reg[c] * A.beta) + 0.0f;
    }

    // diffTerm_k = remap(Gauss(upscale(sign_k)), forwardMap_k)  (btv_l1_cuda.cpp:378-382), k ascending.  Frames go in chunks of KC: the
    // KC map positions are loaded together, then (NW > 0) the NW x NW sign samples each window can reach, then the sums are formed
    // -- a chunk waits for two rounds of loads instead of two or more per frame.
    const int kb = A.kb, r = kb >> 1, s = g.scale, lw = g.lw, lh = g.lh;
    const unsigned inv = g.inv_scale;
    const size_t hplane = (size_t)hw * hh, lplane = (size_t)lw * lh * CN, pix = (size_t)y * hw + x;
    constexpr int KC = NW == 0 ? 3 : (NW * NW * CN <= 12 ? 3 : (NW * NW * CN <= 18 ? 2 : 1));
    for (int k0 = 0; k0 < g.K; k0 += KC) {
        unsigned q[KC];
#pragma unroll
        for (int u = 0; u < KC; ++u) q[u] = A.p.fidx[(size_t)min(k0 + u, g.K - 1) * hplane + pix];
        float e[KC][NW > 0 ? NW * NW : 1][CN];
        if (NW > 0) {
#pragma unroll
            for (int u = 0; u < KC; ++u) {
                const signed char *S = A.p.sgn + (size_t)min(k0 + u, g.K - 1) * lplane;
                const int py = (int)(q[u] >> 16), px = (int)(q[u] & 0xffffu);
                const int qy = (int)__umulhi((unsigned)(max(py - r, 0) + s - 1), inv), qx = (int)__umulhi((unsigned)(max(px - r, 0) + s - 1), inv);
#pragma unroll
                for (int a = 0; a < NW; ++a)
#pragma unroll
                    for (int b = 0; b < NW; ++b) {
                        // samples past the window are loaded from a clamped position and not added
                        const signed char *p = S + ((size_t)min(qy + a, lh - 1) * lw + min(qx + b, lw - 1)) * CN;
#pragma unroll
                        for (int c = 0; c < CN; ++c) e[u][NW > 0 ? a * NW + b : 0][c] = (float)p[c];
                    }
            }
        }
#pragma unroll
        for (int u = 0; u < KC; ++u) {
            if (k0 + u < g.K) {
                const int py = (int)(q[u] >> 16), px = (int)(q[u] & 0xffffu);
                float col[CN];
#pragma unroll
                for (int c = 0; c < CN; ++c) col[c] = 0.0f;
                const bool interior = py - r >= 0 && py + r < hh && px - r >= 0 && px + r < hw;
                if (NW > 0 && interior) {
                    // no tap is reflected: the window reaches at most NW x NW sign samples, the multiples of the scale inside it
                    const int wy0 = py - r, wx0 = px - r;
                    const int qy = (int)__umulhi((unsigned)(wy0 + s - 1), inv), qx = (int)__umulhi((unsigned)(wx0 + s - 1), inv);
#pragma unroll
                    for (int a = 0; a < NW; ++a) {
                        const int ty = (qy + a) * s;
                        float rs[CN];
#pragma unroll
                        for (int c = 0; c < CN; ++c) rs[c] = 0.0f;
#pragma unroll
                        for (int b = 0; b < NW; ++b) {
                            const int tx = (qx + b) * s;
                            const bool ok = tx <= px + r;
                            const float gi = s_g[(tx - wx0) & (MAX_TAPS - 1)];
#pragma unroll
                            for (int c = 0; c < CN; ++c) {
                                const float n = rs[c] + e[u][NW > 0 ? a * NW + b : 0][c] * gi;
                                rs[c] = ok ? n : rs[c];
                            }
                        }
                        const bool ok = ty <= py + r;
                        const float gj = s_g[(ty - wy0) & (MAX_TAPS - 1)];
#pragma unroll
                        for (int c = 0; c < CN; ++c) {
                            const float n = col[c] + rs[c] * gj;
                            col[c] = ok ? n : col[c];
                        }
                    }
                } else {
                    const Px<CN> t = frame_term_loops<CN>(A.p.sgn + (size_t)(k0 + u) * lplane, s_g, py, px, kb, s, inv, lw, hw, hh);
#pragma unroll
                    for (int c = 0; c < CN; ++c) col[c] = t.c[c];
                }
#pragma unroll
                for (int c = 0; c < CN; ++c) v[c] = (v[c] * 1.0f + col[c] * A.tau) + 0.0f;
            }
        }
    }

    float *Xn = A.p.X[A.cur ^ 1] + o;
#pragma unroll
    for (int c = 0; c < CN; ++c) Xn[c] = v[c];
    if (A.dst) {
        // highRes_(inner).copyTo(dst): without a border of btvKernelSize pixels (btv_l1_cuda.cpp:398-399)
        const int b = A.crop;
        if (y >= b && y < hh - b && x >= b && x < hw - b) {
            float *d = reinterpret_cast<float *>(A.dst + (size_t)(y - b) * A.dstep) + (size_t)(x - b) * CN;
#pragma unroll
            for (int c = 0; c < CN; ++c) d[c] = v[c];
        }
    }
}

// GpuMat::convertTo between CV_8U and CV_32F over `n` scalars per row (saturate_cast: round to nearest even, clamp), or a copy
template <class S, class D>
__global__ __launch_bounds__(256) void k_convert(const unsigned char *src, size_t sstep, unsigned char *dst, size_t dstep, int rows, int n)
{
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= n || y >= rows) return;
    const S v = reinterpret_cast<const S *>(src + (size_t)y * sstep)[x];
    D *d = reinterpret_cast<D *>(dst + (size_t)y * dstep) + x;
    if (sizeof(S) == 4 && sizeof(D) == 1) *d = (D)min(max(__float2int_rn((float)v), 0), 255);
    else *d = (D)v;
}

void launch_convert(int sdepth, int ddepth, const void *src, size_t sstep, void *dst, size_t dstep, int rows, int n, hipStream_t st)
{
    const dim3 grid(div_up(n, 64), div_up(rows, 4));
    const unsigned char *s = (const unsigned char *)src;
    unsigned char *d = (unsigned char *)dst;
    if (sdepth == 0 && ddepth == 5) hipLaunchKernelGGL((k_convert<unsigned char, float>), grid, dim3(256), 0, st, s, sstep, d, dstep, rows, n);
    else if (sdepth == 5 && ddepth == 0) hipLaunchKernelGGL((k_convert<float, unsigned char>), grid, dim3(256), 0, st, s, sstep, d, dstep, rows, n);
    else if (sdepth == 5) hipLaunchKernelGGL((k_convert<float, float>), grid, dim3(256), 0, st, s, sstep, d, dstep, rows, n);
    else hipLaunchKernelGGL((k_convert<unsigned char, unsigned char>), grid, dim3(256), 0, st, s, sstep, d, dstep, rows, n);
}

static dim3 grid64x4(int w, int h, int z) { return dim3(div_up(w, 64), div_up(h, 4), z); }
// cuda::resize upwards by (scale, scale): the kernels receive float(1.0 / fx) (resize.cpp:105), inexact for scale 3
static float up_factor(const Geo &g) { return (float)(1.0 / (double)g.scale); }

void launch_rel_motions(const Geo &g, const Planes &p, int base_idx, hipStream_t st)
{
    hipLaunchKernelGGL(k_rel_motions, grid64x4(g.lw, g.lh, 1), dim3(256), 0, st, g, p, base_idx);
}

void launch_maps(const Geo &g, const Planes &p, float *maps_f, hipStream_t st)
{
    hipLaunchKernelGGL(k_maps, grid64x4(g.hw, g.hh, g.K), dim3(256), 0, st, g, p, up_factor(g), maps_f);
}

void launch_init(const Geo &g, const Planes &p, int base_idx, hipStream_t st)
{
    const dim3 grid = grid64x4(g.hw, g.hh, 1);
    if (g.cn == 1) hipLaunchKernelGGL((k_init<1>), grid, dim3(256), 0, st, g, p, up_factor(g), base_idx);
    else if (g.cn == 3) hipLaunchKernelGGL((k_init<3>), grid, dim3(256), 0, st, g, p, up_factor(g), base_idx);
    else hipLaunchKernelGGL((k_init<4>), grid, dim3(256), 0, st, g, p, up_factor(g), base_idx);
}

void launch_data(const IterArgs &A, hipStream_t st)
{
    const dim3 grid = grid64x4(A.g.lw, A.g.lh, A.g.K);
    const size_t lds = A.data_lds ? data_lds_bytes(A.kb, A.g.scale) : 0;
    if (A.g.cn == 1) hipLaunchKernelGGL((k_data<1>), grid, dim3(256), lds, st, A);
    else if (A.g.cn == 3) hipLaunchKernelGGL((k_data<3>), grid, dim3(256), lds, st, A);
    else hipLaunchKernelGGL((k_data<4>), grid, dim3(256), lds, st, A);
}

template <int CN>
static void launch_update_cn(const IterArgs &A, dim3 grid, hipStream_t st)
{
    const int nw = (A.kb - 1) / A.g.scale + 1;
    if (nw == 1) hipLaunchKernelGGL((k_update<CN, 1>), grid, dim3(256), 0, st, A);
    else if (nw == 2) hipLaunchKernelGGL((k_update<CN, 2>), grid, dim3(256), 0, st, A);
    else if (nw == 3) hipLaunchKernelGGL((k_update<CN, 3>), grid, dim3(256), 0, st, A);
    else hipLaunchKernelGGL((k_update<CN, 0>), grid, dim3(256), 0, st, A);
}

void launch_update(const IterArgs &A, hipStream_t st)
{
    const dim3 grid(div_up(A.g.hw, UT_W), div_up(A.g.hh, UT_H));
    if (A.g.cn == 1) launch_update_cn<1>(A, grid, st);
    else if (A.g.cn == 3) launch_update_cn<3>(A, grid, st);
    else launch_update_cn<4>(A, grid, st);
}

}  // namespace btvl1
}  // namespace mi
