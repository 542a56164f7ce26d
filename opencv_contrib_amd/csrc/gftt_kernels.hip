// cv::cuda::CornernessCriteria and cv::cuda::CornersDetector for gfx950 (wave64).  Replaces the separable Sobel of cudafilters
// (row_filter.hpp, column_filter.hpp), cornerHarris_kernel / cornerMinEigenVal_kernel of cudaimgproc/src/cuda/corners.cu and findCorners /
// sortCorners_gpu of cuda/gftt.cu.
//
// The reference writes Dx and Dy to memory through two filters of two launches each, reads them back through textures, finds the maximum
// with cuda::minMax and a read-back, appends with atomicAdd in arrival order and sorts with thrust.  Here (gftt_plan.h has the list):
//   - the response is ONE launch: the source tile and a halo go to LDS, Dx and Dy of the tile plus the window's halo are computed there
//     and never leave it.  A halo position outside the image holds Dx / Dy AT THE BORDER-MAPPED COORDINATE, which is what the reference's
//     window reads; it is not the derivative of an extended image;
//   - every float operation is the reference's in its order: each pixel adds its blockSize^2 products, rows outer, columns inner;
//   - sqrtf is taken in binary64 of the exactly converted argument and rounded once, which is correctly rounded for binary32;
//   - the threshold is computed on the device; ballots over row segments and a two-level scan give row-major order without atomics;
//   - the sort is a bitonic network on 64-bit keys {~ordered(response), linear index}: response descending, then (y, x) ascending.
// No __constant__ memory, no textures, no environment switches.
#include "gftt_dev.h"

namespace mi {
namespace gftt {

namespace {

// ---- index maps of border_interpolate.hpp (main repository) as the reference's kernels use them; n = the length of the axis
__device__ __forceinline__ int brd_low(int i, int n, int border)
{
    if (border == GFTT_BORDER_REPLICATE) return max(i, 0);
    if (border == GFTT_BORDER_REFLECT101) return abs(i) % n;
    return (abs(i) - (i < 0)) % n;
}
__device__ __forceinline__ int brd_high(int i, int n, int border)
{
    if (border == GFTT_BORDER_REPLICATE) return min(i, n - 1);
    if (border == GFTT_BORDER_REFLECT101) return abs((n - 1) - abs((n - 1) - i)) % n;
    return abs((n - 1) - abs((n - 1) - i) + (i > n - 1)) % n;
}
// the window's read: BrdRow* / BrdCol*::idx_col / idx_row, and the texture's clamp for BORDER_REPLICATE (corners.cu:114-121,150)
__device__ __forceinline__ int brd_window(int i, int n, int border) { return brd_low(brd_high(i, n, border), n, border); }
// the filter's read of p = (a pixel of the image) +- 1: at_low left of the image, at_high right of it (row_filter.hpp:83-121);
// -1: a position no output depends on
__device__ __forceinline__ int brd_filter(int p, int n, int border)
{
    if (p >= 0 && p < n) return p;
    if (p == -1) return brd_low(p, n, border);
    if (p == n) return brd_high(p, n, border);
    return -1;
}

__device__ __forceinline__ float load_src(const GfttImage &im, int y, int x)
{
    const unsigned char *row = im.data + (long long)y * im.step;
    return im.type == MI_8UC1 ? (float)row[x] : ((const float *)row)[x];   // saturate_cast<float>
}

// sum = 0; sum = sum + v[k] * kernel[k], k = 0, 1, 2 (row_filter.hpp:132-136)
__device__ __forceinline__ float taps3(float v0, float v1, float v2, const float (&k)[3])
{
    float sum = 0.f;
    sum = sum + v0 * k[0];
    sum = sum + v1 * k[1];
    sum = sum + v2 * k[2];
    return sum;
}

__device__ __forceinline__ float sqrt_rn(float v) { return (float)sqrt((double)v); }

// corners.cu:91 and :193-196
__device__ __forceinline__ float criterion(float a, float b, float c, int harris, float k)
{
    if (harris) return a * c - b * b - k * (a + c) * (a + c);
    a *= 0.5f;
    c *= 0.5f;
    return (a + c) - sqrt_rn((a - c) * (a - c) + b * b);
}

__device__ __forceinline__ float wave_max(float m)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    return m;
}

// the maximum of the workgroup's 4 waves -> wgmax[tile]
__device__ __forceinline__ void tile_max(float m, float *wgmax)
{
    __shared__ float wm[GFTT_BLOCK / 64];
    m = wave_max(m);
    if ((threadIdx.x & 63) == 0) wm[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) wgmax[blockIdx.y * gridDim.x + blockIdx.x] = fmaxf(fmaxf(wm[0], wm[1]), fmaxf(wm[2], wm[3]));
}

__global__ __launch_bounds__(GFTT_BLOCK) void k_gftt_response(GfttImage im, GfttCorner cp, int sw, int sh, int dw, int dh, GfttPlane dst,
                                                              float *wgmax)
{
    extern __shared__ float lds[];
    float *S = lds, *DX = S + sw * sh, *DY = DX + dw * dh;
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * GFTT_TILE_W, y0 = blockIdx.y * GFTT_TILE_H;
    const int lo = cp.block_size / 2;
    const int sx0 = x0 - lo - 1, sy0 = y0 - lo - 1;   // the image position of S[0]
    // the source of the tile, the window's halo and the filter's one pixel around both; positions outside the image hold what the
    // filters read there.  Only rows [0, rows) and columns [0, cols) of the caller's view are touched.
    for (int it = tid; it < sw * sh; it += GFTT_BLOCK) {
        const int r = it / sw, c = it - r * sw;
        const int gy = brd_filter(sy0 + r, im.rows, cp.border), gx = brd_filter(sx0 + c, im.cols, cp.border);
        S[it] = gy >= 0 && gx >= 0 ? load_src(im, gy, gx) : 0.f;
    }
    __syncthreads();
    for (int it = tid; it < dw * dh; it += GFTT_BLOCK) {
        const int r = it / dw, c = it - r * dw;
        const int my = brd_window(y0 - lo + r, im.rows, cp.border), mx = brd_window(x0 - lo + c, im.cols, cp.border);
        const int ly = my - sy0, lx = mx - sx0;
        float dx = 0.f, dy = 0.f;
        if (ly >= 1 && ly <= sh - 2 && lx >= 1 && lx <= sw - 2) {   // every position a pixel of this tile reads is (gftt_plan.h)
            const float *s = S + (ly - 1) * sw + lx - 1;
            const float d0 = taps3(s[0], s[1], s[2], cp.deriv), m0 = taps3(s[0], s[1], s[2], cp.smooth);
            s += sw;
            const float d1 = taps3(s[0], s[1], s[2], cp.deriv), m1 = taps3(s[0], s[1], s[2], cp.smooth);
            s += sw;
            const float d2 = taps3(s[0], s[1], s[2], cp.deriv), m2 = taps3(s[0], s[1], s[2], cp.smooth);
            dx = taps3(d0, d1, d2, cp.smooth);   // rows [-1 0 1], columns [1 2 1] * scale
            dy = taps3(m0, m1, m2, cp.deriv);    // rows [1 2 1] * scale, columns [-1 0 1]
        }
        DX[it] = dx; DY[it] = dy;
    }
    __syncthreads();
    const int lane = tid & 63, wave = tid >> 6;
    const int x = x0 + lane;
    float best = -INFINITY;
    for (int q = 0; q < GFTT_TILE_H / 4; ++q) {
        const int ry = wave * (GFTT_TILE_H / 4) + q, y = y0 + ry;
        if (y >= im.rows || x >= im.cols) continue;
        float a = 0.f, b = 0.f, c = 0.f;
        for (int i = 0; i < cp.block_size; ++i) {
            const float *px = DX + (ry + i) * dw + lane, *py = DY + (ry + i) * dw + lane;
            for (int j = 0; j < cp.block_size; ++j) {
                const float dx = px[j], dy = py[j];
                a += dx * dx;
                b += dx * dy;
                c += dy * dy;
            }
        }
        const float v = criterion(a, b, c, cp.harris, cp.k);
        *(float *)((char *)dst.data + (long long)y * dst.step + 4ll * x) = v;
        best = fmaxf(best, v);
    }
    tile_max(best, wgmax);
}

__global__ __launch_bounds__(GFTT_BLOCK) void k_gftt_deriv(GfttImage im, GfttCorner cp, float *pdx, float *pdy)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int x = blockIdx.x * GFTT_TILE_W + lane;
    if (x >= im.cols) return;
    const int xs[3] = {brd_filter(x - 1, im.cols, cp.border), x, brd_filter(x + 1, im.cols, cp.border)};
    for (int q = 0; q < GFTT_TILE_H / 4; ++q) {
        const int y = blockIdx.y * GFTT_TILE_H + wave * (GFTT_TILE_H / 4) + q;
        if (y >= im.rows) return;
        float d[3], m[3];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const int gy = r == 1 ? y : brd_filter(y - 1 + r, im.rows, cp.border);
            const float s0 = load_src(im, gy, xs[0]), s1 = load_src(im, gy, xs[1]), s2 = load_src(im, gy, xs[2]);
            d[r] = taps3(s0, s1, s2, cp.deriv);
            m[r] = taps3(s0, s1, s2, cp.smooth);
        }
        pdx[(long long)y * im.cols + x] = taps3(d[0], d[1], d[2], cp.smooth);
        pdy[(long long)y * im.cols + x] = taps3(m[0], m[1], m[2], cp.deriv);
    }
}

__global__ __launch_bounds__(GFTT_BLOCK) void k_gftt_window(const float *pdx, const float *pdy, int rows, int cols, GfttCorner cp, GfttPlane dst,
                                                            float *wgmax)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int x = blockIdx.x * GFTT_TILE_W + lane;
    const int lo = cp.block_size / 2;
    float best = -INFINITY;
    for (int q = 0; q < GFTT_TILE_H / 4; ++q) {
        const int y = blockIdx.y * GFTT_TILE_H + wave * (GFTT_TILE_H / 4) + q;
        if (y >= rows || x >= cols) continue;
        float a = 0.f, b = 0.f, c = 0.f;
        for (int i = 0; i < cp.block_size; ++i) {
            const long long row = (long long)brd_window(y - lo + i, rows, cp.border) * cols;
            for (int j = 0; j < cp.block_size; ++j) {
                const long long at = row + brd_window(x - lo + j, cols, cp.border);
                const float dx = pdx[at], dy = pdy[at];
                a += dx * dx;
                b += dx * dy;
                c += dy * dy;
            }
        }
        const float v = criterion(a, b, c, cp.harris, cp.k);
        *(float *)((char *)dst.data + (long long)y * dst.step + 4ll * x) = v;
        best = fmaxf(best, v);
    }
    tile_max(best, wgmax);
}

__global__ __launch_bounds__(GFTT_SCAN_THREADS) void k_gftt_threshold(const float *wgmax, int n, double quality, int *ctl)
{
    __shared__ float sh[GFTT_SCAN_THREADS / 64];
    float m = -INFINITY;
    for (int i = threadIdx.x; i < n; i += GFTT_SCAN_THREADS) m = fmaxf(m, wgmax[i]);
    m = wave_max(m);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int i = 1; i < GFTT_SCAN_THREADS / 64; ++i) m = fmaxf(m, sh[i]);
        ctl[GFTT_CTL_THRESHOLD] = __float_as_int((float)((double)m * quality));   // gftt.cpp:124
    }
}

__device__ __forceinline__ float plane_at(const GfttPlane &p, int y, int x) { return *(const float *)((const char *)p.data + (long long)y * p.step + 4ll * x); }

__global__ __launch_bounds__(GFTT_BLOCK) void k_gftt_find(GfttPlane resp, int rows, int cols, GfttMask mask, const int *thr_dev, float thr_host,
                                                          unsigned long long *masks, int segs_x, int nseg, int *bcount)
{
    __shared__ int wc[GFTT_BLOCK / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float threshold = thr_dev ? __int_as_float(thr_dev[GFTT_CTL_THRESHOLD]) : thr_host;
    int cnt = 0;
    for (int s = 0; s < GFTT_FIND_SEGS / 4; ++s) {
        const int seg = blockIdx.x * GFTT_FIND_SEGS + wave * (GFTT_FIND_SEGS / 4) + s;
        if (seg >= nseg) break;   // wave-uniform
        const int i = seg / segs_x, j = (seg - i * segs_x) * GFTT_SEG + lane;
        bool ok = i > 0 && i < rows - 1 && j > 0 && j < cols - 1;
        if (ok && mask.data) ok = mask.data[(long long)i * mask.step + j] != 0;
        if (ok) {
            const float val = plane_at(resp, i, j);
            ok = val > threshold;
            if (ok) {
                float mx = val;
                mx = fmaxf(plane_at(resp, i - 1, j - 1), mx);
                mx = fmaxf(plane_at(resp, i - 1, j), mx);
                mx = fmaxf(plane_at(resp, i - 1, j + 1), mx);
                mx = fmaxf(plane_at(resp, i, j - 1), mx);
                mx = fmaxf(plane_at(resp, i, j + 1), mx);
                mx = fmaxf(plane_at(resp, i + 1, j - 1), mx);
                mx = fmaxf(plane_at(resp, i + 1, j), mx);
                mx = fmaxf(plane_at(resp, i + 1, j + 1), mx);
                ok = val == mx;
            }
        }
        const unsigned long long bits = __ballot(ok);
        if (lane == 0) masks[seg] = bits;
        cnt += __popcll(bits);
    }
    if (lane == 0) wc[wave] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) bcount[blockIdx.x] = wc[0] + wc[1] + wc[2] + wc[3];
}

// ONE workgroup over the FIND workgroups' counts: thread t owns a contiguous run, so bases are row-major
__global__ __launch_bounds__(GFTT_SCAN_THREADS) void k_gftt_scan(const int *bcount, int *bbase, int nfind, int capacity, int *ctl)
{
    __shared__ int sh[GFTT_SCAN_THREADS];
    const int t = threadIdx.x;
    const int chunk = (nfind + GFTT_SCAN_THREADS - 1) / GFTT_SCAN_THREADS;
    const int lo = min(nfind, t * chunk), hi = min(nfind, lo + chunk);
    int n = 0;
    for (int i = lo; i < hi; ++i) n += bcount[i];
    sh[t] = n;
    __syncthreads();
    for (int o = 1; o < GFTT_SCAN_THREADS; o <<= 1) {
        const int add = t >= o ? sh[t - o] : 0;
        __syncthreads();
        sh[t] += add;
        __syncthreads();
    }
    int base = sh[t] - n;
    for (int i = lo; i < hi; ++i) {
        bbase[i] = base;
        base += bcount[i];
    }
    if (t == 0) {
        const int found = sh[GFTT_SCAN_THREADS - 1], count = min(found, capacity);   // gftt.cu:111
        int npad = 0;
        if (count > 0) for (npad = GFTT_SORT_TILE; npad < count; npad <<= 1) {}
        ctl[GFTT_CTL_FOUND] = found; ctl[GFTT_CTL_COUNT] = count; ctl[GFTT_CTL_NPAD] = npad;
    }
}

// ascending keys are response descending, then linear index ascending; -0 and +0 are one response (EigGreater compares with >)
__device__ __forceinline__ unsigned long long make_key(float r, int idx)
{
    if (r == 0.f) r = 0.f;
    const unsigned u = (unsigned)__float_as_int(r);
    const unsigned ordered = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return ((unsigned long long)~ordered << 32) | (unsigned)idx;
}

__global__ __launch_bounds__(GFTT_BLOCK) void k_gftt_emit(GfttPlane resp, int cols, const unsigned long long *masks, int segs_x, int nseg,
                                                          const int *bbase, int capacity, unsigned long long *keys, float2 *pts)
{
    __shared__ int pre[GFTT_FIND_SEGS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int seg0 = blockIdx.x * GFTT_FIND_SEGS;
    if (wave == 0) {   // exclusive prefix of the workgroup's 64 segment counts
        const int c = seg0 + lane < nseg ? __popcll(masks[seg0 + lane]) : 0;
        int incl = c;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int up = __shfl_up(incl, o);
            if (lane >= o) incl += up;
        }
        pre[lane] = incl - c;
    }
    __syncthreads();
    const int base = bbase[blockIdx.x];
    for (int s = 0; s < GFTT_FIND_SEGS / 4; ++s) {
        const int ls = wave * (GFTT_FIND_SEGS / 4) + s, seg = seg0 + ls;
        if (seg >= nseg) break;
        const unsigned long long m = masks[seg];
        if (!((m >> lane) & 1)) continue;
        const int at = base + pre[ls] + __popcll(m & ((1ull << lane) - 1));
        if (at >= capacity) continue;   // the first `capacity` in row-major order stay
        const int y = seg / segs_x, x = (seg - y * segs_x) * GFTT_SEG + lane;
        if (keys) keys[at] = make_key(plane_at(resp, y, x), y * cols + x);
        if (pts) pts[at] = make_float2((float)x, (float)y);   // gftt.cu:84
    }
}

__global__ __launch_bounds__(GFTT_BLOCK) void k_gftt_make_keys(GfttPlane resp, int cols, const float2 *pts, int n, unsigned long long *keys, int *ctl)
{
    const int i = blockIdx.x * GFTT_BLOCK + threadIdx.x;
    if (i == 0) {
        int npad = 0;
        if (n > 0) for (npad = GFTT_SORT_TILE; npad < n; npad <<= 1) {}
        ctl[GFTT_CTL_FOUND] = n; ctl[GFTT_CTL_COUNT] = n; ctl[GFTT_CTL_NPAD] = npad;
    }
    if (i >= n) return;
    const int x = (int)pts[i].x, y = (int)pts[i].y;   // tex(a.y, a.x), gftt.cu:119
    keys[i] = make_key(plane_at(resp, y, x), y * cols + x);
}

__device__ __forceinline__ void compare_swap(unsigned long long &a, unsigned long long &b, bool ascending)
{
    if ((a > b) == ascending) { const unsigned long long t = a; a = b; b = t; }
}

// steps j = from .. 1 of the merge of length-k sequences inside one LDS tile; the direction is that of the GLOBAL network
__device__ __forceinline__ void tile_steps(unsigned long long *t, int base, int k, int from)
{
    for (int j = from; j >= 1; j >>= 1) {
#pragma unroll
        for (int q = 0; q < GFTT_SORT_TILE / 2 / GFTT_SORT_THREADS; ++q) {
            const int p = threadIdx.x + q * GFTT_SORT_THREADS;
            const int i = ((p & ~(j - 1)) << 1) | (p & (j - 1));
            unsigned long long a = t[i], b = t[i | j];
            compare_swap(a, b, ((base + i) & k) == 0);
            t[i] = a; t[i | j] = b;
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(GFTT_SORT_THREADS) void k_gftt_sort_local(unsigned long long *keys, const int *ctl)
{
    __shared__ unsigned long long t[GFTT_SORT_TILE];
    const int base = blockIdx.x * GFTT_SORT_TILE, count = ctl[GFTT_CTL_COUNT];
    if (base >= ctl[GFTT_CTL_NPAD]) return;   // uniform
    for (int i = threadIdx.x; i < GFTT_SORT_TILE; i += GFTT_SORT_THREADS) t[i] = base + i < count ? keys[base + i] : ~0ull;
    __syncthreads();
    for (int k = 2; k <= GFTT_SORT_TILE; k <<= 1) tile_steps(t, base, k, k / 2);
    for (int i = threadIdx.x; i < GFTT_SORT_TILE; i += GFTT_SORT_THREADS) keys[base + i] = t[i];
}

__global__ __launch_bounds__(GFTT_SORT_THREADS) void k_gftt_sort_global(unsigned long long *keys, const int *ctl, int k, int j)
{
    const int npad = ctl[GFTT_CTL_NPAD];
    const int p = blockIdx.x * GFTT_SORT_THREADS + threadIdx.x;
    if (k > npad || p >= npad / 2) return;
    const int i = ((p & ~(j - 1)) << 1) | (p & (j - 1));
    unsigned long long a = keys[i], b = keys[i | j];
    compare_swap(a, b, (i & k) == 0);
    keys[i] = a; keys[i | j] = b;
}

__global__ __launch_bounds__(GFTT_SORT_THREADS) void k_gftt_sort_merge(unsigned long long *keys, const int *ctl, int k)
{
    __shared__ unsigned long long t[GFTT_SORT_TILE];
    const int base = blockIdx.x * GFTT_SORT_TILE, npad = ctl[GFTT_CTL_NPAD];
    if (k > npad || base >= npad) return;   // uniform
    for (int i = threadIdx.x; i < GFTT_SORT_TILE; i += GFTT_SORT_THREADS) t[i] = keys[base + i];
    __syncthreads();
    tile_steps(t, base, k, GFTT_SORT_TILE / 2);
    for (int i = threadIdx.x; i < GFTT_SORT_TILE; i += GFTT_SORT_THREADS) keys[base + i] = t[i];
}

__global__ __launch_bounds__(GFTT_BLOCK) void k_gftt_points(const unsigned long long *keys, int cols, int limit, float2 *out, int *ctl)
{
    const int count = ctl[GFTT_CTL_COUNT];
    const int nout = limit > 0 ? min(limit, count) : count;   // gftt.cpp:136
    const int i = blockIdx.x * GFTT_BLOCK + threadIdx.x;
    if (i == 0) ctl[GFTT_CTL_NOUT] = nout;
    if (i >= nout) return;
    const int idx = (int)(unsigned)keys[i];
    const int y = idx / cols;
    out[i] = make_float2((float)(idx - y * cols), (float)y);
}

}  // namespace

int response_fused(const GfttLaunch &k, const GfttResponsePlan &p, const GfttImage &im, const GfttCorner &c, const GfttPlane &dst, float *wgmax,
                   hipStream_t st)
{
    hipLaunchKernelGGL(k_gftt_response, dim3(k.grid_x, k.grid_y), dim3(k.block), k.lds, st, im, c, p.sw, p.sh, p.dw, p.dh, dst, wgmax);
    MI_HIP_TRY(hipGetLastError());
    return MI_OK;
}

int response_deriv(const GfttLaunch &k, const GfttImage &im, const GfttCorner &c, float *dx, float *dy, hipStream_t st)
{
    hipLaunchKernelGGL(k_gftt_deriv, dim3(k.grid_x, k.grid_y), dim3(k.block), 0, st, im, c, dx, dy);
    MI_HIP_TRY(hipGetLastError());
    return MI_OK;
}

int response_window(const GfttLaunch &k, const GfttResponsePlan &p, const GfttCorner &c, const float *dx, const float *dy, const GfttPlane &dst,
                    float *wgmax, hipStream_t st)
{
    hipLaunchKernelGGL(k_gftt_window, dim3(k.grid_x, k.grid_y), dim3(k.block), 0, st, dx, dy, p.rows, p.cols, c, dst, wgmax);
    MI_HIP_TRY(hipGetLastError());
    return MI_OK;
}

int threshold(const GfttLaunch &k, const float *wgmax, int n, double quality, int *ctl, hipStream_t st)
{
    hipLaunchKernelGGL(k_gftt_threshold, dim3(k.grid_x), dim3(k.block), 0, st, wgmax, n, quality, ctl);
    MI_HIP_TRY(hipGetLastError());
    return MI_OK;
}

int find(const GfttLaunch &k, const GfttPlane &resp, int rows, int cols, const GfttMask &mask, const int *thr_dev, float thr_host,
         unsigned long long *masks, int segs_x, int nseg, int *bcount, hipStream_t st)
{
    hipLaunchKernelGGL(k_gftt_find, dim3(k.grid_x), dim3(k.block), 0, st, resp, rows, cols, mask, thr_dev, thr_host, masks, segs_x, nseg, bcount);
    MI_HIP_TRY(hipGetLastError());
    return MI_OK;
}

int scan(const GfttLaunch &k, const int *bcount, int *bbase, int nfind, int capacity, int *ctl, hipStream_t st)
{
    hipLaunchKernelGGL(k_gftt_scan, dim3(k.grid_x), dim3(k.block), 0, st, bcount, bbase, nfind, capacity, ctl);
    MI_HIP_TRY(hipGetLastError());
    return MI_OK;
}

int emit(const GfttLaunch &k, const GfttPlane &resp, int cols, const unsigned long long *masks, int segs_x, int nseg, const int *bbase,
         int capacity, unsigned long long *keys, float *pts, hipStream_t st)
{
    hipLaunchKernelGGL(k_gftt_emit, dim3(k.grid_x), dim3(k.block), 0, st, resp, cols, masks, segs_x, nseg, bbase, capacity, keys, (float2 *)pts);
    MI_HIP_TRY(hipGetLastError());
    return MI_OK;
}

int make_keys(const GfttPlane &resp, int cols, const float *pts, int n, unsigned long long *keys, int *ctl, hipStream_t st)
{
    hipLaunchKernelGGL(k_gftt_make_keys, dim3(div_up(n > 0 ? n : 1, GFTT_BLOCK)), dim3(GFTT_BLOCK), 0, st, resp, cols, (const float2 *)pts, n, keys,
                       ctl);
    MI_HIP_TRY(hipGetLastError());
    return MI_OK;
}

int sort_step(const GfttLaunch &k, unsigned long long *keys, const int *ctl, hipStream_t st)
{
    if (k.kernel == GFTT_K_SORT_LOCAL) hipLaunchKernelGGL(k_gftt_sort_local, dim3(k.grid_x), dim3(k.block), 0, st, keys, ctl);
    else if (k.kernel == GFTT_K_SORT_GLOBAL) hipLaunchKernelGGL(k_gftt_sort_global, dim3(k.grid_x), dim3(k.block), 0, st, keys, ctl, k.k, k.j);
    else hipLaunchKernelGGL(k_gftt_sort_merge, dim3(k.grid_x), dim3(k.block), 0, st, keys, ctl, k.k);
    MI_HIP_TRY(hipGetLastError());
    return MI_OK;
}

int points(const GfttLaunch &k, const unsigned long long *keys, int cols, int limit, float *out, int *ctl, hipStream_t st)
{
    hipLaunchKernelGGL(k_gftt_points, dim3(k.grid_x), dim3(k.block), 0, st, keys, cols, limit, (float2 *)out, ctl);
    MI_HIP_TRY(hipGetLastError());
    return MI_OK;
}

}  // namespace gftt
}  // namespace mi
