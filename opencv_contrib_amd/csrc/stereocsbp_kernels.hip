// cv::cuda::StereoConstantSpaceBP: the HIP kernels.  Twin of modules/cudastereo/src/cuda/stereocsbp.cu, bit for bit: every f32 add,
// multiply, compare and the one division are separately rounded (-ffp-contract=off) in the reference's order; 16-bit messages are summed
// in int and wrap when they are narrowed to short, and every value the reference stores through short is rounded where it stores it.
// The reference's parameters travel as kernel arguments.  All kernels run 64-lane waves and read no texture.
#include <cfloat>
#include "stereocsbp_dev.h"

namespace mi {
namespace scsbp {

// saturate_cast<T>(float): short = round to nearest even, clamp (cvt.rni.sat.s16.f32); float = the value
template <class T> __device__ __forceinline__ T sat(float v);
template <> __device__ __forceinline__ float sat<float>(float v) { return v; }
template <> __device__ __forceinline__ short sat<short>(float v) { return (short)min(max(__float2int_rn(v), -32768), 32767); }
template <class T> __device__ __forceinline__ T t_max();
template <> __device__ __forceinline__ float t_max<float>() { return FLT_MAX; }
template <> __device__ __forceinline__ short t_max<short>() { return 32767; }
// T v = a + b + ...: float adds left to right; shorts are promoted to int and the sum wraps when it is narrowed
__device__ __forceinline__ float add4(float a, float b, float c, float d) { return ((a + b) + c) + d; }
__device__ __forceinline__ short add4(short a, short b, short c, short d) { return (short)((int)a + (int)b + (int)c + (int)d); }
__device__ __forceinline__ float add5(float a, float b, float c, float d, float e) { return (((a + b) + c) + d) + e; }
__device__ __forceinline__ short add5(short a, short b, short c, short d, short e) { return (short)((int)a + (int)b + (int)c + (int)d + (int)e); }
// float cost_min = minimum + max_disc_term (stereocsbp.cu:677): T + int
__device__ __forceinline__ float plus_int(float m, int k) { return m + (float)k; }
__device__ __forceinline__ float plus_int(short m, int k) { return (float)((int)m + k); }

// ---------------------------------------------------------------- pixeldiff, stereocsbp.cu:61-84
template <int CN> __device__ __forceinline__ float pixeldiff(const unsigned char *l, const unsigned char *r, float max_data_term)
{
    if (CN == 1) return fminf((float)abs((int)l[0] - (int)r[0]), max_data_term);
    const float tb = 0.114f * (float)abs((int)l[0] - (int)r[0]);
    const float tg = 0.587f * (float)abs((int)l[1] - (int)r[1]);
    const float tr = 0.299f * (float)abs((int)l[2] - (int)r[2]);
    return fminf((tr + tg) + tb, max_data_term);
}

// ---------------------------------------------------------------- init_data_cost / compute_data_cost, stereocsbp.cu:178-267, :356-447
// One launch geometry for both: an ITEM is (pixel, candidate).  The coarse levels have few pixels (640 x 480 at level 3: 80 x 60), so
// the candidates are spread over lanes and blocks next to the pixels, and every item is computed once from the images.
// A candidate whose right column would lie beyond the image (possible only with candidates the reference itself would read out of
// bounds with) is charged like one that lies before it.
template <class T>
struct CostArgs {
    const unsigned char *left, *right; long long lstep, rstep; int rows, cols;
    const T *sel; long long sel_step; int h2;
    T *out; long long ostep; int h, w, level, n;
    float max_data_term, data_weight; int min_disp;
};

template <class T> __device__ __forceinline__ int candidate(const CostArgs<T> &a, int k, int y, int x)
{
    return a.sel ? (int)a.sel[((long long)k * a.h2 + y / 2) * a.sel_step + x / 2] : k;
}

// levels 0 and 1: one running sum over the window, rows outer and columns inner
template <class T, int CN>
__global__ __launch_bounds__(64) void k_csbp_data_cost_plain(CostArgs<T> a)
{
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y, k = blockIdx.z;
    if (x >= a.w) return;
    const int d = candidate(a, k, y, x);
    const int y0 = y << a.level, yt = (y + 1) << a.level, x0 = x << a.level, xt = (x + 1) << a.level;
    float val = 0.0f;
    for (int yi = y0; yi < yt; ++yi)
        for (int xi = x0; xi < xt; ++xi) {
            const int xr = xi - d;
            if (d < a.min_disp || xr < 0 || xr >= a.cols) val += a.data_weight * a.max_data_term;
            else val += a.data_weight * pixeldiff<CN>(a.left + yi * a.lstep + xi * CN, a.right + yi * a.rstep + xr * CN, a.max_data_term);
        }
    a.out[((long long)k * a.h + y) * a.ostep + x] = sat<T>(val);
}

// reduce<W>, W <= 32, of the reference (core/cuda/reduce.hpp, WarpOptimized): lane 0 of the W-lane segment ends with the total
template <int W> __device__ __forceinline__ float tree(float v)
{
#pragma unroll
    for (int delta = W / 2; delta >= 1; delta /= 2) v += __shfl_down(v, delta, W);
    return v;
}

// levels 2 .. 7, WINSZ = 2^level: lane tid of an item sums column tid of the window, the columns are combined by the reference's tree
template <class T, int CN, int WINSZ>
__global__ __launch_bounds__(256) void k_csbp_data_cost_reduce(CostArgs<T> a, long long items)
{
    constexpr int G = 256 / WINSZ;   // items of a block
    const int tid = threadIdx.x % WINSZ;
    const long long it = (long long)blockIdx.x * G + threadIdx.x / WINSZ;
    const bool live = it < items;
    int k = 0, x_out = 0, y_out = 0;
    float val = 0.0f;
    if (live) {
        k = (int)(it % a.n);
        const long long pix = it / a.n;
        x_out = (int)(pix % a.w); y_out = (int)(pix / a.w);
        const int d = candidate(a, k, y_out, x_out);
        const int x0 = x_out << a.level, y0 = y_out << a.level;
        const int len = min(y0 + WINSZ, a.rows) - y0;
        if (x0 + tid < a.cols) {
            const int xr = x0 + tid - d;
            if (xr < 0 || d < a.min_disp || xr >= a.cols) val = a.data_weight * a.max_data_term * (float)len;
            else {
                const unsigned char *lle = a.left + y0 * a.lstep + CN * (x0 + tid), *lri = a.right + y0 * a.rstep + CN * xr;
                for (int y = 0; y < len; ++y) {
                    val += a.data_weight * pixeldiff<CN>(lle, lri, a.max_data_term);
                    lle += a.lstep; lri += a.rstep;
                }
            }
        }
    }
    if constexpr (WINSZ <= 32) val = tree<WINSZ>(val);
    else if constexpr (WINSZ == 64) {          // GenericOptimized32, M = 2: the tree of 32 in each half, then total(0) + total(1)
        val = tree<32>(val);
        val += __shfl_down(val, 32, 64);
    } else {                                   // WINSZ == 128, M = 4: (g0 + g2) + (g1 + g3)
        static_assert(WINSZ == 128, "window");
        __shared__ float part[8];
        val = tree<32>(val);
        if (threadIdx.x % 32 == 0) part[threadIdx.x / 32] = val;
        __syncthreads();
        if (tid == 0) {
            const float *g = part + threadIdx.x / 32;
            val = (g[0] + g[2]) + (g[1] + g[3]);
        }
    }
    if (live && tid == 0) a.out[((long long)k * a.h + y_out) * a.ostep + x_out] = sat<T>(val);
}

template <class T, int CN>
static int launch_data_cost(const CostArgs<T> &a, hipStream_t s)
{
    const long long items = (long long)a.w * a.h * a.n;
    const auto blocks = [&](int winsz) { return dim3((unsigned)((items + 256 / winsz - 1) / (256 / winsz))); };
    switch (a.level) {
    case 0: case 1: hipLaunchKernelGGL((k_csbp_data_cost_plain<T, CN>), dim3(div_up(a.w, 64), a.h, a.n), dim3(64), 0, s, a); break;
    case 2: hipLaunchKernelGGL((k_csbp_data_cost_reduce<T, CN, 4>), blocks(4), dim3(256), 0, s, a, items); break;
    case 3: hipLaunchKernelGGL((k_csbp_data_cost_reduce<T, CN, 8>), blocks(8), dim3(256), 0, s, a, items); break;
    case 4: hipLaunchKernelGGL((k_csbp_data_cost_reduce<T, CN, 16>), blocks(16), dim3(256), 0, s, a, items); break;
    case 5: hipLaunchKernelGGL((k_csbp_data_cost_reduce<T, CN, 32>), blocks(32), dim3(256), 0, s, a, items); break;
    case 6: hipLaunchKernelGGL((k_csbp_data_cost_reduce<T, CN, 64>), blocks(64), dim3(256), 0, s, a, items); break;
    case 7: hipLaunchKernelGGL((k_csbp_data_cost_reduce<T, CN, 128>), blocks(128), dim3(256), 0, s, a, items); break;
    default: MI_REQUIRE(false, MI_ERR_BAD_ARG, "level must be 0 .. 7");
    }
    MI_HIP_TRY(hipGetLastError());
    return MI_OK;
}

template <class T>
static int data_cost_t(const CsbpImages &im, const void *sel, long long sel_step, int h2, void *out, long long ostep, int h, int w, int level,
                       int n, const CsbpConst &c, hipStream_t s)
{
    MI_REQUIRE(h > 0 && w > 0 && n > 0 && h <= 65535 && n <= 65535, MI_ERR_BAD_SIZE, "level of %d x %d with %d candidates", h, w, n);
    MI_REQUIRE(level >= 0 && level < CSBP_MAX_LEVELS && (h << level) <= im.rows && (w << level) <= im.cols, MI_ERR_BAD_SIZE,
               "a %d x %d level %d does not fit the image", h, w, level);
    const CostArgs<T> a = {im.left, im.right, im.lstep, im.rstep, im.rows, im.cols, (const T *)sel, sel_step, h2, (T *)out, ostep, h, w, level, n,
                           c.max_data_term, c.data_weight, c.min_disp};
    switch (im.cn) {
    case 1: return launch_data_cost<T, 1>(a, s);
    case 3: return launch_data_cost<T, 3>(a, s);
    case 4: return launch_data_cost<T, 4>(a, s);
    }
    MI_REQUIRE(false, MI_ERR_BAD_TYPE, "left.type() == CV_8UC1 || left.type() == CV_8UC3 || left.type() == CV_8UC4");
}

int data_cost(int msg_type, const CsbpImages &im, const void *sel, long long sel_step, int h2, void *out, long long ostep, int h, int w,
              int level, int n, const CsbpConst &c, hipStream_t s)
{
    return msg_type == CSBP_MSG_32F ? data_cost_t<float>(im, sel, sel_step, h2, out, ostep, h, w, level, n, c, s)
                                    : data_cost_t<short>(im, sel, sel_step, h2, out, ostep, h, w, level, n, c, s);
}

// ---------------------------------------------------------------- get_first_k_initial_local / _global, stereocsbp.cu:86-176
template <class T>
__global__ __launch_bounds__(256) void k_csbp_first_k(int local, T *cost, T *sel_cost, T *sel_disp, long long step, int h, int w, int nr_plane,
                                                      int ndisp)
{
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (!(y < h && x < w)) return;
    const long long plane = step * h, off = y * step + x;
    T *sd = sel_disp + off, *sc = sel_cost + off, *dc = cost + off;
    int found = 0;
    if (local && ndisp > 2) {   // strict local minima in ascending d (:134-154); with ndisp == 2 the loop body never runs
        T prev = dc[0], cur = dc[plane], next = dc[2 * plane];
        for (int d = 1; d < ndisp - 1 && found < nr_plane; ++d) {
            if (cur < prev && cur < next) {
                sc[found * plane] = cur;
                sd[found * plane] = (T)d;
                dc[d * plane] = t_max<T>();
                ++found;
            }
            prev = cur;
            cur = next;
            next = dc[(d + 1) * plane];
        }
    }
    for (int i = found; i < nr_plane; ++i) {   // the global minima of what remains; ties to the lowest index, (max, 0) once all is spent
        T minimum = t_max<T>();
        int id = 0;
        for (int d = 0; d < ndisp; ++d) {
            const T cur = dc[d * plane];
            if (cur < minimum) { minimum = cur; id = d; }
        }
        sc[i * plane] = minimum;
        sd[i * plane] = (T)id;
        dc[id * plane] = t_max<T>();
    }
}

// The same selection with one WAVE per pixel, ndisp <= CSBP_FIRST_K_WAVE_MAX: the coarsest level has few pixels (640 x 480 at level 3:
// 4800, 75 waves if a lane is a pixel) and every one of them makes nr_plane passes over ndisp costs, so the disparities are spread over
// the lanes.  The pixel's costs are read from global memory once into LDS, twice: orig[] keeps what the local pass compares (the
// reference's prev / cur / next are all values from before any overwrite), work[] takes the overwrites with max.  A pass is a strided
// scan per lane (strict <, ascending: the lowest index of a lane's minimum) and a butterfly over the wave that prefers the smaller
// value and, for equal values, the smaller index: the first occurrence of the minimum, as the sequential scan finds it.
__device__ __forceinline__ float wave_xor(float v, int m) { return __shfl_xor(v, m, 64); }
__device__ __forceinline__ short wave_xor(short v, int m) { return (short)__shfl_xor((int)v, m, 64); }

template <class T>
__global__ __launch_bounds__(64) void k_csbp_first_k_wave(int local, const T *cost, T *sel_cost, T *sel_disp, long long step, int h, int w,
                                                          int nr_plane, int ndisp)
{
    extern __shared__ unsigned char csbp_smem[];
    T *orig = (T *)csbp_smem, *work = orig + ndisp;
    const int lane = threadIdx.x, x = blockIdx.x % w, y = blockIdx.x / w;
    const long long plane = step * h, off = y * step + x;
    for (int d = lane; d < ndisp; d += 64) orig[d] = work[d] = cost[off + d * plane];
    __syncthreads();   // one wave per block: orders the LDS writes before the reads below
    int found = 0;
    if (local && ndisp > 2) {
        // The reference's loop (:136-153) reloads next from plane d + 1 at the end of step d, the plane it already holds, so its window
        // lags from step 2 on: step 1 sees (c0, c1, c2), steps 2 and 3 see (c1, c2, c2) and (c2, c2, c3) and never hit, and step d >= 4
        // sees (c[d-2], c[d-1], c[d]).  A hit at step d stores the window's middle value with disparity d and overwrites plane d.  All
        // three values are from before any overwrite (the overwritten plane is never ahead of the loads).  The first nr_plane hits in
        // ascending d are taken.
        for (int d0 = 0; d0 < ndisp && found < nr_plane; d0 += 64) {
            const int d = d0 + lane, mid = d == 1 ? 1 : d - 1;
            const bool hit = (d == 1 || d >= 4) && d < ndisp - 1 && orig[mid] < orig[mid - 1] && orig[mid] < orig[mid + 1];
            const unsigned long long m = __ballot(hit);
            const int slot = found + __popcll(m & ((1ull << lane) - 1ull));
            if (hit && slot < nr_plane) {
                sel_cost[off + slot * plane] = orig[mid];
                sel_disp[off + slot * plane] = (T)d;
                work[d] = t_max<T>();
            }
            found = min(found + __popcll(m), nr_plane);
        }
        __syncthreads();
    }
    for (int i = found; i < nr_plane; ++i) {   // the global minima of what remains; (max, 0) once all is spent
        T best = t_max<T>();
        int id = 0x7fffffff;
        for (int d = lane; d < ndisp; d += 64) {
            const T v = work[d];
            if (v < best) { best = v; id = d; }
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            const T ob = wave_xor(best, m);
            const int oi = __shfl_xor(id, m, 64);
            if (ob < best || (ob == best && oi < id)) { best = ob; id = oi; }
        }
        if (id == 0x7fffffff) id = 0;
        if (lane == 0) {
            sel_cost[off + i * plane] = best;
            sel_disp[off + i * plane] = (T)id;
            work[id] = t_max<T>();
        }
        __syncthreads();
    }
}

template <class T>
static int first_k_t(int local, void *cost, void *sel_cost, void *sel_disp, long long step, int h, int w, int nr_plane, int ndisp, hipStream_t s)
{
    if (ndisp <= CSBP_FIRST_K_WAVE_MAX)
        hipLaunchKernelGGL(k_csbp_first_k_wave<T>, dim3((unsigned)h * (unsigned)w), dim3(64), 2 * (size_t)ndisp * sizeof(T), s, local, (const T *)cost,
                           (T *)sel_cost, (T *)sel_disp, step, h, w, nr_plane, ndisp);
    else
        hipLaunchKernelGGL(k_csbp_first_k<T>, dim3(div_up(w, 64), div_up(h, 4)), dim3(64, 4), 0, s, local, (T *)cost, (T *)sel_cost, (T *)sel_disp, step,
                           h, w, nr_plane, ndisp);
    MI_HIP_TRY(hipGetLastError());
    return MI_OK;
}

int first_k(int msg_type, int local, void *cost, void *sel_cost, void *sel_disp, long long step, int h, int w, int nr_plane, int ndisp,
            hipStream_t s)
{
    MI_REQUIRE(h > 0 && w > 0 && (long long)h * w < (1ll << 31), MI_ERR_BAD_SIZE, "level of %d x %d", h, w);
    return msg_type == CSBP_MSG_32F ? first_k_t<float>(local, cost, sel_cost, sel_disp, step, h, w, nr_plane, ndisp, s)
                                    : first_k_t<short>(local, cost, sel_cost, sel_disp, step, h, w, nr_plane, ndisp, s);
}

// ---------------------------------------------------------------- init_message, stereocsbp.cu:525-607
template <class T> struct Set { T *u, *d, *l, *r, *disp; long long step; };
template <class T> static Set<T> set_of(const CsbpSet &m) { return {(T *)m.u, (T *)m.d, (T *)m.l, (T *)m.r, (T *)m.disp, m.step}; }

template <class T>
__global__ __launch_bounds__(256) void k_csbp_init_message(T *temp, Set<T> nw, Set<T> cur, T *sel_cost, const T *data_cost, int h, int w,
                                                           int nr_plane, int h2, int w2, int nr_plane2)
{
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (!(y < h && x < w)) return;
    const long long p1 = nw.step * h, p2 = cur.step * h2, off = y * nw.step + x, off2 = (y / 2) * cur.step + x / 2;
    const T *un = cur.u + min(h2 - 1, y / 2 + 1) * cur.step + x / 2;
    const T *dn = cur.d + max(0, y / 2 - 1) * cur.step + x / 2;
    const T *ln = cur.l + (y / 2) * cur.step + min(w2 - 1, x / 2 + 1);
    const T *rn = cur.r + (y / 2) * cur.step + max(0, x / 2 - 1);
    T *sum = temp + off;
    const T *dc = data_cost + off;
    for (int d = 0; d < nr_plane2; ++d) sum[d * p1] = add5(dc[d * p1], un[d * p2], dn[d * p2], ln[d * p2], rn[d * p2]);
    // get_first_k_element_increase (:525-556): selected on the summed cost, stored is the unsummed one
    for (int i = 0; i < nr_plane; ++i) {
        T minimum = t_max<T>();
        int id = 0;
        for (int j = 0; j < nr_plane2; ++j) {
            const T c = sum[j * p1];
            if (c < minimum) { minimum = c; id = j; }
        }
        sel_cost[off + i * p1] = dc[id * p1];
        nw.disp[off + i * p1] = cur.disp[off2 + id * p2];
        nw.u[off + i * p1] = cur.u[off2 + id * p2];
        nw.d[off + i * p1] = cur.d[off2 + id * p2];
        nw.l[off + i * p1] = cur.l[off2 + id * p2];
        nw.r[off + i * p1] = cur.r[off2 + id * p2];
        sum[id * p1] = t_max<T>();
    }
}

int init_message(int msg_type, void *temp, const CsbpSet &nw, const CsbpSet &cur, void *sel_cost, const void *data_cost, int h, int w,
                 int nr_plane, int h2, int w2, int nr_plane2, hipStream_t s)
{
    const dim3 grid(div_up(w, 64), div_up(h, 4)), block(64, 4);
    if (msg_type == CSBP_MSG_32F)
        hipLaunchKernelGGL(k_csbp_init_message<float>, grid, block, 0, s, (float *)temp, set_of<float>(nw), set_of<float>(cur), (float *)sel_cost,
                           (const float *)data_cost, h, w, nr_plane, h2, w2, nr_plane2);
    else
        hipLaunchKernelGGL(k_csbp_init_message<short>, grid, block, 0, s, (short *)temp, set_of<short>(nw), set_of<short>(cur), (short *)sel_cost,
                           (const short *)data_cost, h, w, nr_plane, h2, w2, nr_plane2);
    MI_HIP_TRY(hipGetLastError());
    return MI_OK;
}

// ---------------------------------------------------------------- compute_message, stereocsbp.cu:656-716
// The pixel a lane updates in half-sweep t: x = 2 i + ((y + t) & 1), interior only; rows 1 .. h - 2 are blockIdx.y + 1.
__device__ __forceinline__ bool iter_pixel(int w, int t, int *x, int *y)
{
    *y = blockIdx.y + 1;
    *x = ((blockIdx.x * 64 + threadIdx.x) << 1) + ((*y + t) & 1);
    return *x > 0 && *x < w - 1;
}
// the three messages that enter message k (u, d, l, r) of a pixel, the neighbour whose candidates it is sent to, and where it goes
// (:711-714).  No lane reads an element another lane of the launch writes: every neighbour is of the other checkerboard colour.
template <class T>
__device__ __forceinline__ void message_ports(const Set<T> &m, long long off, int k, T **dst, const T **m1, const T **m2, const T **m3,
                                              const T **src_disp)
{
    const T *un = m.u + off + m.step, *dn = m.d + off - m.step, *ln = m.l + off + 1, *rn = m.r + off - 1, *disp = m.disp + off;
    switch (k) {
    case 0: *dst = m.u + off; *m1 = rn; *m2 = un; *m3 = ln; *src_disp = disp - m.step; break;
    case 1: *dst = m.d + off; *m1 = dn; *m2 = rn; *m3 = ln; *src_disp = disp + m.step; break;
    case 2: *dst = m.l + off; *m1 = un; *m2 = dn; *m3 = ln; *src_disp = disp - 1; break;
    default: *dst = m.r + off; *m1 = un; *m2 = dn; *m3 = rn; *src_disp = disp + 1; break;
    }
}

// General form, any nr_plane: message_per_pixel as the reference has it, the sums in the message itself and the clipped costs in temp.
template <class T>
__global__ __launch_bounds__(64) void k_csbp_message_gen(Set<T> m, const T *sel_cost, T *temp_, int h, int w, int n, int t, int max_disc_term,
                                                         float jump)
{
    int x, y;
    if (!iter_pixel(w, t, &x, &y)) return;
    const long long plane = m.step * h, off = y * m.step + x;
    const T *data = sel_cost + off, *dst_disp = m.disp + off;
    T *temp = temp_ + off;
    for (int k = 0; k < 4; ++k) {
        T *dst;
        const T *m1, *m2, *m3, *src_disp;
        message_ports(m, off, k, &dst, &m1, &m2, &m3, &src_disp);
        T minimum = t_max<T>();
        for (int d = 0; d < n; ++d) {
            const T val = add4(data[d * plane], m1[d * plane], m2[d * plane], m3[d * plane]);
            if (val < minimum) minimum = val;
            dst[d * plane] = val;
        }
        float sum = 0;
        for (int d = 0; d < n; ++d) {
            float cost_min = plus_int(minimum, max_disc_term);
            const float sd = (float)src_disp[d * plane];
            for (int d2 = 0; d2 < n; ++d2) cost_min = fminf(cost_min, (float)dst[d2 * plane] + jump * fabsf((float)dst_disp[d2 * plane] - sd));
            temp[d * plane] = sat<T>(cost_min);
            sum += cost_min;   // the unrounded one
        }
        sum /= (float)n;
        for (int d = 0; d < n; ++d) dst[d * plane] = sat<T>((float)temp[d * plane] - sum);
    }
}

// Register form, nr_plane <= CAP: the sums and the candidates' disparities of the pixel stay in VGPRs (statically indexed), the clipped
// costs of the message in a lane-private LDS column (indexed by the runtime plane), and every element of the message is written once.
template <class T, int CAP>
__global__ __launch_bounds__(64) void k_csbp_message_reg(Set<T> m, const T *sel_cost, int h, int w, int n, int t, int max_disc_term, float jump)
{
    __shared__ T clipped[CAP][64];
    int x, y;
    if (!iter_pixel(w, t, &x, &y)) return;
    const int lane = threadIdx.x;
    const long long plane = m.step * h, off = y * m.step + x;
    const T *data = sel_cost + off;
    float dd[CAP], val[CAP];
#pragma unroll
    for (int i = 0; i < CAP; ++i) dd[i] = i < n ? (float)m.disp[off + i * plane] : 0.0f;
    for (int k = 0; k < 4; ++k) {
        T *dst;
        const T *m1, *m2, *m3, *src_disp;
        message_ports(m, off, k, &dst, &m1, &m2, &m3, &src_disp);
        T minimum = t_max<T>();
#pragma unroll
        for (int i = 0; i < CAP; ++i)
            if (i < n) {
                const T v = add4(data[i * plane], m1[i * plane], m2[i * plane], m3[i * plane]);
                if (v < minimum) minimum = v;
                val[i] = (float)v;
            }
        const float ceiling = plus_int(minimum, max_disc_term);
        float sum = 0;
        for (int d = 0; d < n; ++d) {
            float cost_min = ceiling;
            const float sd = (float)src_disp[d * plane];
#pragma unroll
            for (int i = 0; i < CAP; ++i)
                if (i < n) cost_min = fminf(cost_min, val[i] + jump * fabsf(dd[i] - sd));
            clipped[d][lane] = sat<T>(cost_min);
            sum += cost_min;
        }
        sum /= (float)n;
        for (int d = 0; d < n; ++d) dst[d * plane] = sat<T>((float)clipped[d][lane] - sum);
    }
}

template <class T>
static int launch_iterate(int form, int cap, const CsbpSet &ms, const void *sel_cost, void *temp, int h, int w, int n, int t, const CsbpConst &c,
                          hipStream_t s)
{
    MI_REQUIRE(n > 0, MI_ERR_BAD_ARG, "nr_plane > 0");
    if (h < 3 || w < 3) return MI_OK;   // no interior pixel
    MI_REQUIRE(h - 2 <= 65535, MI_ERR_BAD_SIZE, "too many rows");
    const dim3 grid(div_up(div_up(w, 2), 64), h - 2), block(64);
    const Set<T> m = set_of<T>(ms);
    const T *sc = (const T *)sel_cost;
    const int k = c.max_disc_term;
    const float j = c.disc_single_jump;
    if (form == CSBP_FORM_GEN) {
        MI_REQUIRE(temp, MI_ERR_BAD_ARG, "the general form needs its temp plane");
        hipLaunchKernelGGL(k_csbp_message_gen<T>, grid, block, 0, s, m, sc, (T *)temp, h, w, n, t, k, j);
    }
    else if (form == CSBP_FORM_REG && cap == 4 && n <= 4) hipLaunchKernelGGL((k_csbp_message_reg<T, 4>), grid, block, 0, s, m, sc, h, w, n, t, k, j);
    else if (form == CSBP_FORM_REG && cap == 8 && n <= 8) hipLaunchKernelGGL((k_csbp_message_reg<T, 8>), grid, block, 0, s, m, sc, h, w, n, t, k, j);
    else if (form == CSBP_FORM_REG && cap == 16 && n <= 16) hipLaunchKernelGGL((k_csbp_message_reg<T, 16>), grid, block, 0, s, m, sc, h, w, n, t, k, j);
    else if (form == CSBP_FORM_REG && cap == 32 && n <= 32) hipLaunchKernelGGL((k_csbp_message_reg<T, 32>), grid, block, 0, s, m, sc, h, w, n, t, k, j);
    else if (form == CSBP_FORM_REG && cap == 64 && n <= 64) hipLaunchKernelGGL((k_csbp_message_reg<T, 64>), grid, block, 0, s, m, sc, h, w, n, t, k, j);
    else MI_REQUIRE(false, MI_ERR_BAD_ARG, "no iteration kernel of form %d, capacity %d for %d planes", form, cap, n);
    MI_HIP_TRY(hipGetLastError());
    return MI_OK;
}

int iterate(int msg_type, int form, int cap, const CsbpSet &m, const void *sel_cost, void *temp, int h, int w, int nr_plane, int t,
            const CsbpConst &c, hipStream_t s)
{
    return msg_type == CSBP_MSG_32F ? launch_iterate<float>(form, cap, m, sel_cost, temp, h, w, nr_plane, t, c, s)
                                    : launch_iterate<short>(form, cap, m, sel_cost, temp, h, w, nr_plane, t, c, s);
}

// ---------------------------------------------------------------- compute_disp, stereocsbp.cu:752-804, with the border fill and the conversion
// saturate_cast<O>(short) of convertTo
template <class O> __device__ __forceinline__ O out_cast(short best) { return (O)best; }
template <> __device__ __forceinline__ unsigned char out_cast<unsigned char>(short best) { return (unsigned char)min(max((int)best, 0), 255); }

template <class T, class O>
__global__ __launch_bounds__(256) void k_csbp_disp(Set<T> m, const T *sel_cost, int rows, int cols, int n, O *disp, long long ostep)
{
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (!(x < cols && y < rows)) return;
    O *o = (O *)((char *)disp + y * ostep) + x;
    if (!(y > 0 && y < rows - 1 && x > 0 && x < cols - 1)) { *o = (O)0; return; }   // out.setTo(0)  stereocsbp.cpp:314
    const long long plane = m.step * rows, off = y * m.step + x;
    const T *data = sel_cost + off, *ds = m.disp + off;
    const T *u = m.u + off + m.step, *d = m.d + off - m.step, *l = m.l + off + 1, *r = m.r + off - 1;
    short best = 0;
    T best_val = t_max<T>();
    for (int i = 0; i < n; ++i) {
        const T val = add5(data[i * plane], u[i * plane], d[i * plane], l[i * plane], r[i * plane]);
        if (val < best_val) { best_val = val; best = sat<short>((float)ds[i * plane]); }
    }
    *o = out_cast<O>(best);
}

template <class T, class O>
static int launch_disp(const CsbpSet &m, const void *sel_cost, int rows, int cols, int n, void *disp, long long ostep, hipStream_t s)
{
    hipLaunchKernelGGL((k_csbp_disp<T, O>), dim3(div_up(cols, 64), div_up(rows, 4)), dim3(64, 4), 0, s, set_of<T>(m), (const T *)sel_cost, rows, cols,
                       n, (O *)disp, ostep);
    MI_HIP_TRY(hipGetLastError());
    return MI_OK;
}
template <class T>
static int disp_t(const CsbpSet &m, const void *sel_cost, int rows, int cols, int n, void *disp, long long ostep, int out_type, hipStream_t s)
{
    switch (out_type) {
    case MI_16SC1: return launch_disp<T, short>(m, sel_cost, rows, cols, n, disp, ostep, s);
    case MI_8UC1: return launch_disp<T, unsigned char>(m, sel_cost, rows, cols, n, disp, ostep, s);
    case MI_32SC1: return launch_disp<T, int>(m, sel_cost, rows, cols, n, disp, ostep, s);
    case MI_32FC1: return launch_disp<T, float>(m, sel_cost, rows, cols, n, disp, ostep, s);
    }
    MI_REQUIRE(false, MI_ERR_BAD_TYPE, "disparity: must be CV_16SC1, CV_8UC1, CV_32SC1 or CV_32FC1");
}

int compute_disp(int msg_type, const CsbpSet &m, const void *sel_cost, int rows, int cols, int nr_plane, void *disp, long long ostep,
                 int out_type, hipStream_t s)
{
    return msg_type == CSBP_MSG_32F ? disp_t<float>(m, sel_cost, rows, cols, nr_plane, disp, ostep, out_type, s)
                                    : disp_t<short>(m, sel_cost, rows, cols, nr_plane, disp, ostep, out_type, s);
}

}  // namespace scsbp
}  // namespace mi
