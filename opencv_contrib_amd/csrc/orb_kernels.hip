// cv::cuda::ORB for gfx950 (wave64).  Replaces the kernels of cudafeatures2d/src/cuda/orb.cu and what orb.cpp calls around them
// (cuda::resize, threshold, bitwise_and, the Gaussian filter, thrust::sort_by_key).  orb_plan.h has the launch list.
//
//   - every integer and f32 operation is the reference's, in its order, uncontracted; the three transcendental places are defined in
//     double and rounded once: angle = (float)atan2((double)m_01, (double)m_10), sina / cosa = (float)sin / cos((double)ar);
//   - the cull is a SELECT and a RANK, not a sort of all candidates: the total order is (response descending, index ascending) on an
//     order-preserving integer key with -0 == +0; histograms are integer sums, so no result depends on the arrival order of an atomic;
//   - Harris, angle and descriptors run one wave per keypoint and reduce with cross-lane moves; grids are sized by capacities and the
//     kernels read the keypoint counts on the device, so the host never waits between stages;
//   - no __constant__ memory (u_max is an argument), no textures, no environment switches.
#include "orb_dev.h"

namespace mi {
namespace orb {

namespace {

constexpr float ORB_PI_F = 3.14159265f;      // CV_PI_F, opencv2/core/cuda/common.hpp
constexpr float ORB_HARRIS_K = 0.04f;        // orb.cpp: HARRIS_K

__device__ __forceinline__ int wave_sum(int v)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// saturate_cast<uchar>(float): round to nearest even, saturated
__device__ __forceinline__ unsigned char sat_u8(float v)
{
    const int i = __float2int_rn(v);
    return (unsigned char)min(max(i, 0), 255);
}

__device__ __forceinline__ short2 as_loc(int v) { return make_short2((short)(v & 0xffff), (short)(v >> 16)); }

// resize_linear<uchar>'s arithmetic for one destination pixel (resize.cu:243-267).  x1 / y1 are clamped into the source: they are inside
// wherever the reference reads inside
__device__ __forceinline__ unsigned char resize_px(const OrbPlaneSrc &s, int dst_x, int dst_y, float fx, float fy)
{
    const float src_x = dst_x * fx, src_y = dst_y * fy;
    float out = 0.0f;
    const int x1 = __float2int_rd(src_x), y1 = __float2int_rd(src_y);
    const int x2 = x1 + 1, y2 = y1 + 1;
    const int x1r = min(max(x1, 0), s.cols - 1), y1r = min(max(y1, 0), s.rows - 1);
    const int x2r = min(x2, s.cols - 1), y2r = min(y2, s.rows - 1);
    const unsigned char *r1 = s.data + (long long)y1r * s.step, *r2 = s.data + (long long)y2r * s.step;
    out = out + r1[x1r] * ((x2 - src_x) * (y2 - src_y));
    out = out + r1[x2r] * ((src_x - x1) * (y2 - src_y));
    out = out + r2[x1r] * ((x2 - src_x) * (src_y - y1));
    out = out + r2[x2r] * ((src_x - x1) * (src_y - y1));
    return sat_u8(out);
}

__global__ __launch_bounds__(ORB_BLOCK) void k_orb_level(OrbPlaneSrc src, OrbPlaneSrc msrc, int mask_mode, float fx, float fy, int edge,
                                                          unsigned char *dimg, long long ipitch, unsigned char *dmask, long long mpitch, int rows,
                                                          int cols)
{
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= cols || y >= rows) return;
    dimg[y * ipitch + x] = resize_px(src, x, y, fx, fy);
    if (!dmask) return;
    unsigned char m = 255;   // maskPyr_[level].setTo(255), orb.cpp:680
    if (msrc.data) {
        if (mask_mode == 0) {
            m = msrc.data[(long long)y * msrc.step + x];
        } else {
            m = resize_px(msrc, x, y, fx, fy);
            if (mask_mode == 2) m = m > 254 ? m : 0;   // THRESH_TOZERO
        }
    }
    const bool inner = x >= edge && x < cols - edge && y >= edge && y < rows - edge;
    dmask[y * mpitch + x] = inner ? m : 0;
}

// ---------------------------------------------------------------------------------------------------------------- cull

// ascending in the response, -0 and +0 on one key
__device__ __forceinline__ unsigned order_key(float r)
{
    unsigned b = __float_as_uint(r);
    if (b == 0x80000000u) b = 0;
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

__device__ __forceinline__ int cull_target(const OrbLevelDev &v, int ncull, int c) { return ncull == 2 && c == 0 ? 2 * v.quota : v.quota; }
__device__ __forceinline__ size_t hist_at(int c, int level, int d) { return (((size_t)c * ORB_MAX_LEVELS + level) * ORB_DIGITS + d) * ORB_BINS; }
__device__ __forceinline__ size_t state_at(int c, int level, int d) { return (((size_t)c * ORB_MAX_LEVELS + level) * (ORB_DIGITS + 1) + d) * 2; }

// The select's step after digit d - 1 was counted: from {prefix, k} ("the k-th largest of the keys that start with prefix") and that
// digit's histogram to the next {prefix, k}.  The whole workgroup (256 threads) calls it; every workgroup finds the same pair.
__device__ void select_digit(const int *h, int d_prev, unsigned *prefix, unsigned *k, int *sh, unsigned *res)
{
    const int t = threadIdx.x;
    const int mine = h[ORB_BINS - 1 - t];   // descending bins
    sh[t] = mine;
    __syncthreads();
    for (int o = 1; o < ORB_BINS; o <<= 1) {
        const int add = t >= o ? sh[t - o] : 0;
        __syncthreads();
        sh[t] += add;
        __syncthreads();
    }
    const unsigned incl = (unsigned)sh[t], excl = incl - (unsigned)mine;
    if (incl >= *k && excl < *k) { res[0] = (unsigned)(ORB_BINS - 1 - t); res[1] = *k - excl; }
    __syncthreads();
    *prefix |= res[0] << (24 - 8 * d_prev);
    *k = res[1];
    __syncthreads();
}

// {prefix, k} before digit d is counted; workgroup (0, level) records it
__device__ void select_state(const int *hist, unsigned *state, int c, int level, int d, int n, unsigned *prefix, unsigned *k, int *sh, unsigned *res)
{
    *prefix = 0; *k = (unsigned)n;
    if (d == 0) return;
    if (d > 1) { *prefix = state[state_at(c, level, d - 1)]; *k = state[state_at(c, level, d - 1) + 1]; }
    select_digit(hist + hist_at(c, level, d - 1), d - 1, prefix, k, sh, res);
    if (blockIdx.x == 0 && threadIdx.x == 0) { state[state_at(c, level, d)] = *prefix; state[state_at(c, level, d) + 1] = *k; }
}

__global__ __launch_bounds__(ORB_BLOCK) void k_orb_hist(const OrbLevelDev *tab, int *hist, unsigned *state, int ncull, int c, int d)
{
    __shared__ int sh[ORB_BINS];
    __shared__ unsigned res[2];
    const int level = blockIdx.y;
    const OrbLevelDev &v = tab[level];
    const int in = orb_cull_in(ncull, c);
    const int count = v.counts[1 + in], n = cull_target(v, ncull, c);
    if (count <= n || n == 0 || (int)(blockIdx.x * ORB_BLOCK) >= count) return;   // uniform: no cull (orb.cpp:727-733), or no keypoint here
    unsigned prefix, k;
    select_state(hist, state, c, level, d, n, &prefix, &k, sh, res);
    sh[threadIdx.x] = 0;
    __syncthreads();
    const int i = blockIdx.x * ORB_BLOCK + threadIdx.x;
    if (i < count) {
        unsigned key;
        if (d == 0) { key = order_key(v.resp[in][i]); v.keys[i] = key; }
        else key = v.keys[i];
        const bool in_race = d == 0 || (key >> (32 - 8 * d)) == (prefix >> (32 - 8 * d));
        if (in_race) atomicAdd(&sh[(key >> (24 - 8 * d)) & 255u], 1);
    }
    __syncthreads();
    if (sh[threadIdx.x]) atomicAdd(&hist[hist_at(c, level, d) + threadIdx.x], sh[threadIdx.x]);
}

__global__ __launch_bounds__(ORB_BLOCK) void k_orb_rank(const OrbLevelDev *tab, const int *hist, unsigned *state, int ncull, int c)
{
    __shared__ int sh[ORB_BINS];
    __shared__ unsigned res[2];
    const int level = blockIdx.y;
    const OrbLevelDev &v = tab[level];
    const int in = orb_cull_in(ncull, c), out = orb_cull_out(ncull, c);
    const int count = v.counts[1 + in], n = cull_target(v, ncull, c);
    const int i = blockIdx.x * ORB_BLOCK + threadIdx.x;
    if (count <= n || n == 0) {
        // no sort: the order stays (orb.cpp:727).  n == 0 with keypoints: the level gives none (the reference reads a released matrix)
        const int kept = count <= n ? count : 0;
        if (i == 0) v.counts[1 + out] = kept;
        if (i < kept && v.loc[out] != v.loc[in]) { v.loc[out][i] = v.loc[in][i]; v.resp[out][i] = v.resp[in][i]; }
        return;
    }
    if (i == 0) v.counts[1 + out] = n;
    if ((int)(blockIdx.x * ORB_BLOCK) >= count) return;
    unsigned T, kT;
    select_state(hist, state, c, level, ORB_DIGITS, n, &T, &kT, sh, res);   // T: the n-th largest key
    const int lane = threadIdx.x & 63;
    const unsigned ki = i < count ? v.keys[i] : 0u;
    if (!__any(i < count && ki >= T)) return;   // wave-uniform: nobody here can be kept
    // "j stands in front of i": key larger, or equal and index smaller = one 64-bit compare of {key, ~index}
    const unsigned long long ci = ((unsigned long long)ki << 32) | (unsigned)~i;
    int rank = 0;
    for (int j0 = 0; j0 < count; j0 += 64) {
        const int jl = j0 + lane;
        const unsigned kv = jl < count ? v.keys[jl] : 0u;   // past the end: {0, ~j} stands in front of nobody (j > i)
#pragma unroll
        for (int l = 0; l < 64; ++l) {
            const unsigned kj = (unsigned)__builtin_amdgcn_readlane((int)kv, l);
            const unsigned long long cj = ((unsigned long long)kj << 32) | (unsigned)~(j0 + l);
            rank += cj > ci;
        }
    }
    if (i < count && rank < n) { v.loc[out][rank] = v.loc[in][i]; v.resp[out][rank] = v.resp[in][i]; }
}

// ---------------------------------------------------------------------------------------------------------------- per keypoint

__global__ __launch_bounds__(ORB_BLOCK) void k_orb_harris(const OrbLevelDev *tab, int area)
{
    const OrbLevelDev &v = tab[blockIdx.y];
    const int lane = threadIdx.x & 63, pt = blockIdx.x * ORB_KP_PER_BLOCK + (threadIdx.x >> 6);
    if (pt >= v.counts[1 + area]) return;   // wave-uniform
    const short2 loc = as_loc(v.loc[area][pt]);
    constexpr int bs = ORB_HARRIS_BLOCK, r = bs / 2;
    int a = 0, b = 0, c = 0;
    if (lane < bs * bs) {
        const int i = lane / bs, j = lane % bs;
        const unsigned char *p = v.img + (long long)(loc.y - r + i) * v.pitch + (loc.x - r + j);
        const int P = v.pitch;
        const int Ix = (p[1] - p[-1]) * 2 + (p[-P + 1] - p[-P - 1]) + (p[P + 1] - p[P - 1]);
        const int Iy = (p[P] - p[-P]) * 2 + (p[P - 1] - p[-P - 1]) + (p[P + 1] - p[-P + 1]);
        a = Ix * Ix; b = Iy * Iy; c = Ix * Iy;
    }
    a = wave_sum(a); b = wave_sum(b); c = wave_sum(c);
    if (lane == 0) {
        float scale = (1 << 2) * bs * 255.0f;
        scale = 1.0f / scale;
        const float scale_sq_sq = scale * scale * scale * scale;
        v.resp[area][pt] = ((float)a * b - (float)c * c - ORB_HARRIS_K * ((float)a + b) * ((float)a + b)) * scale_sq_sq;
    }
}

__global__ __launch_bounds__(ORB_BLOCK) void k_orb_angle(const OrbLevelDev *tab, const int *u_max, int half_k, int *m01_out, int *m10_out)
{
    const OrbLevelDev &v = tab[blockIdx.y];
    const int lane = threadIdx.x & 63, pt = blockIdx.x * ORB_KP_PER_BLOCK + (threadIdx.x >> 6);
    if (pt >= v.counts[3]) return;   // wave-uniform
    const short2 loc = as_loc(v.loc[2][pt]);
    const unsigned char *p = v.img + (long long)loc.y * v.pitch + loc.x;
    int m_01 = 0, m_10 = 0;
    // a row of the disc is at most 2 * 29 + 1 = 59 pixels (u_max.size() < 32): one lane per pixel
    { const int u = lane - half_k; if (u <= half_k) m_10 += u * p[u]; }
    for (int vv = 1; vv <= half_k; ++vv) {
        const int d = u_max[vv], u = lane - d;
        if (u <= d) {
            const int val_plus = p[(long long)vv * v.pitch + u], val_minus = p[-(long long)vv * v.pitch + u];
            m_01 += vv * (val_plus - val_minus);
            m_10 += u * (val_plus + val_minus);
        }
    }
    m_01 = wave_sum(m_01); m_10 = wave_sum(m_10);
    if (lane == 0) {
        float kp_dir = (float)atan2((double)m_01, (double)m_10);
        kp_dir += (kp_dir < 0) * (2.0f * ORB_PI_F);
        kp_dir *= 180.0f / ORB_PI_F;
        v.angle[pt] = kp_dir;
        if (m01_out && blockIdx.y == 0) { m01_out[pt] = m_01; m10_out[pt] = m_10; }
    }
}

// rows of the levels in front of `level` in the merged outputs
__device__ __forceinline__ int merged_offset(const OrbLevelDev *tab, int level)
{
    int o = 0;
    for (int l = 0; l < level; ++l) o += tab[l].counts[3];
    return o;
}

struct Sampler {
    const unsigned char *p; int pitch; const int *px, *py; float sina, cosa;
    // GET_VALUE, orb.cu:250-252
    __device__ __forceinline__ int operator()(int idx) const
    {
        const int dy = __float2int_rn(px[idx] * sina + py[idx] * cosa), dx = __float2int_rn(px[idx] * cosa - py[idx] * sina);
        return p[(long long)dy * pitch + dx];
    }
};

// group g of a descriptor byte: one bit with WTA_K 2, two bits with 3 and 4 (the three calc bodies, orb.cu:254-360)
template <int WTA_K> __device__ __forceinline__ int wta_group(const Sampler &s, int g)
{
    if (WTA_K == 2) {
        const int t0 = s(2 * g), t1 = s(2 * g + 1);
        return (t0 < t1) << g;
    } else if (WTA_K == 3) {
        const int t0 = s(3 * g), t1 = s(3 * g + 1), t2 = s(3 * g + 2);
        return (t2 > t1 ? (t2 > t0 ? 2 : 0) : (t1 > t0)) << (2 * g);
    } else {
        int t0 = s(4 * g), t1 = s(4 * g + 1), t2 = s(4 * g + 2), t3 = s(4 * g + 3);
        int a = 0, b = 2;
        if (t1 > t0) t0 = t1, a = 1;
        if (t3 > t2) t2 = t3, b = 3;
        return (t0 > t2 ? a : b) << (2 * g);
    }
}

// one wave per keypoint, two lanes per descriptor byte: each takes half of the byte's groups
template <int WTA_K> __global__ __launch_bounds__(ORB_BLOCK) void k_orb_desc(const OrbLevelDev *tab, const int *pattern, int pattern_cols,
                                                                             unsigned char *desc, long long dstep, int dcap)
{
    const OrbLevelDev &v = tab[blockIdx.y];
    const int lane = threadIdx.x & 63, pt = blockIdx.x * ORB_KP_PER_BLOCK + (threadIdx.x >> 6);
    if (pt >= v.counts[3]) return;   // wave-uniform
    const int row = merged_offset(tab, blockIdx.y) + pt;
    if (row >= dcap) return;
    const short2 loc = as_loc(v.loc[2][pt]);
    float ar = v.angle[pt];
    ar *= (float)(ORB_PI_F / 180.f);
    const float sina = (float)sin((double)ar), cosa = (float)cos((double)ar);
    constexpr int per_byte = WTA_K == 3 ? 12 : 16, groups = WTA_K == 2 ? 8 : 4;
    const int byte = lane >> 1, half = lane & 1;
    const Sampler s = {v.dimg + (long long)loc.y * v.pitch + loc.x, v.pitch, pattern + per_byte * byte, pattern + pattern_cols + per_byte * byte, sina, cosa};
    int val = 0;
#pragma unroll
    for (int g = 0; g < groups / 2; ++g) val |= wta_group<WTA_K>(s, half * (groups / 2) + g);
    val |= __shfl_xor(val, 1);
    if (half == 0) desc[(long long)row * dstep + byte] = (unsigned char)val;
}

__global__ __launch_bounds__(ORB_BLOCK) void k_orb_merge(const OrbLevelDev *tab, unsigned char *kp, long long kstep, int kcap)
{
    const OrbLevelDev &v = tab[blockIdx.y];
    const int i = blockIdx.x * ORB_BLOCK + threadIdx.x;
    if (i >= v.counts[3]) return;
    const int col = merged_offset(tab, blockIdx.y) + i;
    if (col >= kcap) return;
    const short2 loc = as_loc(v.loc[2][i]);
    auto at = [&](int r) -> float & { return *(float *)(kp + r * kstep + 4ll * col); };
    at(0) = loc.x * v.loc_scale;
    at(1) = loc.y * v.loc_scale;
    at(2) = v.resp[2][i];
    at(3) = v.angle[i];
    at(4) = (float)blockIdx.y;
    at(5) = v.size;
}

// ---------------------------------------------------------------------------------------------------------------- blur

__device__ __forceinline__ int reflect101(int i, int n)
{
    if (n == 1) return 0;
    while (i < 0 || i >= n) i = i < 0 ? -i : 2 * n - 2 - i;
    return i;
}

// Row pass into LDS (f32, taps summed in ascending order), column pass out of it: the intermediate is the value the reference stores
__global__ __launch_bounds__(ORB_BLOCK) void k_orb_blur(const unsigned char *src, long long spitch, unsigned char *dst, long long dpitch, int rows, int cols,
                                                         OrbTaps taps)
{
    constexpr int T = ORB_BLUR_TILE, H = 3, TH = T + 2 * H;
    __shared__ unsigned char tile[TH][TH + 2];
    __shared__ float rowp[TH][T];
    const int x0 = blockIdx.x * T, y0 = blockIdx.y * T;
    for (int it = threadIdx.x; it < TH * TH; it += ORB_BLOCK) {
        const int r = it / TH, c = it - r * TH;
        tile[r][c] = src[reflect101(y0 - H + r, rows) * spitch + reflect101(x0 - H + c, cols)];
    }
    __syncthreads();
    for (int it = threadIdx.x; it < TH * T; it += ORB_BLOCK) {
        const int r = it / T, c = it - r * T;
        float sum = 0.0f;
#pragma unroll
        for (int k = 0; k < 7; ++k) sum = sum + (float)tile[r][c + k] * taps.k[k];
        rowp[r][c] = sum;
    }
    __syncthreads();
    const int c = threadIdx.x % T, r = threadIdx.x / T;
    if (x0 + c < cols && y0 + r < rows) {
        float sum = 0.0f;
#pragma unroll
        for (int k = 0; k < 7; ++k) sum = sum + rowp[r + k][c] * taps.k[k];
        dst[(y0 + r) * dpitch + x0 + c] = sat_u8(sum);
    }
}

}  // namespace

int level(const OrbLaunch &k, const OrbPlaneSrc &src, const OrbPlaneSrc &msrc, int mask_mode, float fx, float fy, int edge, unsigned char *dimg,
          long long ipitch, unsigned char *dmask, long long mpitch, int rows, int cols, hipStream_t st)
{
    hipLaunchKernelGGL(k_orb_level, dim3(k.grid_x, k.grid_y), dim3(k.block), 0, st, src, msrc, mask_mode, fx, fy, edge, dimg, ipitch, dmask, mpitch, rows,
                       cols);
    MI_HIP_TRY(hipGetLastError());
    return MI_OK;
}

int hist(const OrbLaunch &k, const OrbLevelDev *tab, int *hist, unsigned *state, int ncull, hipStream_t st)
{
    hipLaunchKernelGGL(k_orb_hist, dim3(k.grid_x, k.grid_y), dim3(k.block), 0, st, tab, hist, state, ncull, k.arg / ORB_DIGITS, k.arg % ORB_DIGITS);
    MI_HIP_TRY(hipGetLastError());
    return MI_OK;
}

int rank(const OrbLaunch &k, const OrbLevelDev *tab, const int *hist, unsigned *state, int ncull, hipStream_t st)
{
    hipLaunchKernelGGL(k_orb_rank, dim3(k.grid_x, k.grid_y), dim3(k.block), 0, st, tab, hist, state, ncull, k.arg);
    MI_HIP_TRY(hipGetLastError());
    return MI_OK;
}

int harris(const OrbLaunch &k, const OrbLevelDev *tab, int area, hipStream_t st)
{
    hipLaunchKernelGGL(k_orb_harris, dim3(k.grid_x, k.grid_y), dim3(k.block), 0, st, tab, area);
    MI_HIP_TRY(hipGetLastError());
    return MI_OK;
}

int angle(const OrbLaunch &k, const OrbLevelDev *tab, const int *u_max, int half_k, int *m01, int *m10, hipStream_t st)
{
    hipLaunchKernelGGL(k_orb_angle, dim3(k.grid_x, k.grid_y), dim3(k.block), 0, st, tab, u_max, half_k, m01, m10);
    MI_HIP_TRY(hipGetLastError());
    return MI_OK;
}

int blur(const OrbLaunch &k, const unsigned char *src, long long spitch, unsigned char *dst, long long dpitch, int rows, int cols, const OrbTaps &taps,
         hipStream_t st)
{
    hipLaunchKernelGGL(k_orb_blur, dim3(k.grid_x, k.grid_y), dim3(k.block), 0, st, src, spitch, dst, dpitch, rows, cols, taps);
    MI_HIP_TRY(hipGetLastError());
    return MI_OK;
}

int descriptors(const OrbLaunch &k, const OrbLevelDev *tab, const int *pattern, int pattern_cols, int wta_k, unsigned char *desc, long long dstep,
                int dcap, hipStream_t st)
{
    const dim3 g(k.grid_x, k.grid_y), b(k.block);
    if (wta_k == 2) hipLaunchKernelGGL(k_orb_desc<2>, g, b, 0, st, tab, pattern, pattern_cols, desc, dstep, dcap);
    else if (wta_k == 3) hipLaunchKernelGGL(k_orb_desc<3>, g, b, 0, st, tab, pattern, pattern_cols, desc, dstep, dcap);
    else hipLaunchKernelGGL(k_orb_desc<4>, g, b, 0, st, tab, pattern, pattern_cols, desc, dstep, dcap);
    MI_HIP_TRY(hipGetLastError());
    return MI_OK;
}

int merge(const OrbLaunch &k, const OrbLevelDev *tab, unsigned char *kp, long long kstep, int kcap, hipStream_t st)
{
    hipLaunchKernelGGL(k_orb_merge, dim3(k.grid_x, k.grid_y), dim3(k.block), 0, st, tab, kp, kstep, kcap);
    MI_HIP_TRY(hipGetLastError());
    return MI_OK;
}

}  // namespace orb
}  // namespace mi
