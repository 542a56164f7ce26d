// cv::cuda::StereoBeliefPropagation: the HIP kernels.  Twin of modules/cudastereo/src/cuda/stereobp.cu, bit for bit: every f32
// add, multiply, compare and the one division are separately rounded (-ffp-contract=off) in the reference's order, and for 16-bit
// messages every value the reference stores through short is rounded where it stores it.  The reference's constants travel as kernel
// arguments.  All kernels run 64-lane waves and read no texture.
#include <cfloat>
#include "stereobp_dev.h"

namespace mi {
namespace sbp {

// saturate_cast<T>(float): short = round to nearest even, clamp (cvt.rni.sat.s16.f32); float = the value
template <class T> __device__ __forceinline__ T sat(float v);
template <> __device__ __forceinline__ float sat<float>(float v) { return v; }
template <> __device__ __forceinline__ short sat<short>(float v) { return (short)min(max(__float2int_rn(v), -32768), 32767); }
// the value a store through T leaves for the next read
template <class T> __device__ __forceinline__ float thru(float v) { return (float)sat<T>(v); }
// dst[i] -= sum (stereobp.cu:425): for short the usual arithmetic conversions, float -> short truncating toward zero
template <class T> __device__ __forceinline__ T sub(float v, float sum);
template <> __device__ __forceinline__ float sub<float>(float v, float sum) { return v - sum; }
template <> __device__ __forceinline__ short sub<short>(float v, float sum) { return (short)(int)(v - sum); }

// ---------------------------------------------------------------- comp_data, stereobp.cu:76-161
template <int CN> __device__ __forceinline__ float pix_diff(const unsigned char *l, const unsigned char *r)
{
    if (CN == 1) return (float)abs((int)l[0] - (int)r[0]);
    const float tr = 0.299f, tg = 0.587f, tb = 0.114f;
    float val = tb * (float)abs((int)l[0] - (int)r[0]);
    val += tg * (float)abs((int)l[1] - (int)r[1]);
    val += tr * (float)abs((int)l[2] - (int)r[2]);
    return val;
}

template <int CN, class T>
__global__ __launch_bounds__(256) void k_sbp_comp_data(const unsigned char *left, long long lstep, const unsigned char *right, long long rstep,
                                                       T *data, long long dstep, int rows, int cols, BpConst c)
{
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (!(y > 0 && y < rows - 1 && x > 0 && x < cols - 1)) return;   // border elements are not written
    const unsigned char *ls = left + y * lstep + x * CN, *rs = right + y * rstep + x * CN;
    T *ds = data + y * dstep + x;
    const long long plane = dstep * rows;
    const float cap = c.data_weight * c.max_data_term;
    for (int disp = 0; disp < c.ndisp; ++disp) {
        float v = cap;
        if (x - disp >= 1) v = fminf(c.data_weight * pix_diff<CN>(ls, rs - disp * CN), cap);
        ds[disp * plane] = sat<T>(v);
    }
}

template <int CN, class T>
static int launch_comp_data(const unsigned char *left, long long lstep, const unsigned char *right, long long rstep, void *data,
                            long long dstep, int rows, int cols, const BpConst &c, hipStream_t s)
{
    hipLaunchKernelGGL((k_sbp_comp_data<CN, T>), dim3(div_up(cols, 64), div_up(rows, 4)), dim3(64, 4), 0, s, left, lstep, right, rstep,
                       (T *)data, dstep, rows, cols, c);
    MI_HIP_TRY(hipGetLastError());
    return MI_OK;
}

int comp_data(int msg_type, int cn, const unsigned char *left, long long lstep, const unsigned char *right, long long rstep,
              void *data, long long dstep, int rows, int cols, const BpConst &c, hipStream_t s)
{
    const bool f = msg_type == SBP_MSG_32F;
    switch (cn) {
    case 1: return f ? launch_comp_data<1, float>(left, lstep, right, rstep, data, dstep, rows, cols, c, s)
                     : launch_comp_data<1, short>(left, lstep, right, rstep, data, dstep, rows, cols, c, s);
    case 3: return f ? launch_comp_data<3, float>(left, lstep, right, rstep, data, dstep, rows, cols, c, s)
                     : launch_comp_data<3, short>(left, lstep, right, rstep, data, dstep, rows, cols, c, s);
    case 4: return f ? launch_comp_data<4, float>(left, lstep, right, rstep, data, dstep, rows, cols, c, s)
                     : launch_comp_data<4, short>(left, lstep, right, rstep, data, dstep, rows, cols, c, s);
    }
    MI_REQUIRE(false, MI_ERR_BAD_TYPE, "left.type() == CV_8UC1 || left.type() == CV_8UC3 || left.type() == CV_8UC4");
}

// ---------------------------------------------------------------- data_step_down, stereobp.cu:257-280
template <class T>
__global__ __launch_bounds__(256) void k_sbp_step_down(const T *src, long long sstep, int src_rows, int src_cols, T *dst, long long dstep,
                                                       int dst_rows, int dst_cols, int ndisp)
{
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (!(x < dst_cols && y < dst_rows)) return;
    const int x0 = 2 * x, x1 = min(x0 + 1, src_cols - 1), y0 = 2 * y, y1 = min(y0 + 1, src_rows - 1);
    for (int d = 0; d < ndisp; ++d) {
        const T *p0 = src + ((long long)d * src_rows + y0) * sstep, *p1 = src + ((long long)d * src_rows + y1) * sstep;
        float v = (float)p0[x0];
        v += (float)p1[x0];
        v += (float)p0[x1];
        v += (float)p1[x1];
        dst[((long long)d * dst_rows + y) * dstep + x] = sat<T>(v);
    }
}

int data_step_down(int msg_type, const void *src, long long sstep, int src_rows, int src_cols, void *dst, long long dstep,
                   int dst_rows, int dst_cols, int ndisp, hipStream_t s)
{
    const dim3 grid(div_up(dst_cols, 64), div_up(dst_rows, 4)), block(64, 4);
    if (msg_type == SBP_MSG_32F)
        hipLaunchKernelGGL(k_sbp_step_down<float>, grid, block, 0, s, (const float *)src, sstep, src_rows, src_cols, (float *)dst, dstep, dst_rows, dst_cols, ndisp);
    else
        hipLaunchKernelGGL(k_sbp_step_down<short>, grid, block, 0, s, (const short *)src, sstep, src_rows, src_cols, (short *)dst, dstep, dst_rows, dst_cols, ndisp);
    MI_HIP_TRY(hipGetLastError());
    return MI_OK;
}

// ---------------------------------------------------------------- level_up_message, stereobp.cu:305-322; blockIdx.z = u, d, l, r
template <class T> struct Msgs { T *u, *d, *l, *r; long long step; };
template <class T> static Msgs<T> msgs_of(const BpMsgs &m) { return {(T *)m.u, (T *)m.d, (T *)m.l, (T *)m.r, m.step}; }

template <class T>
__global__ __launch_bounds__(256) void k_sbp_level_up(Msgs<T> src, int src_rows, Msgs<T> dst, int dst_rows, int dst_cols, int ndisp)
{
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y, m = blockIdx.z;
    if (!(x < dst_cols && y < dst_rows)) return;
    const T *sp = m == 0 ? src.u : m == 1 ? src.d : m == 2 ? src.l : src.r;
    T *dp = m == 0 ? dst.u : m == 1 ? dst.d : m == 2 ? dst.l : dst.r;
    sp += (y / 2) * src.step + x / 2;
    dp += y * dst.step + x;
    const long long splane = src.step * src_rows, dplane = dst.step * dst_rows;
    for (int d = 0; d < ndisp; ++d) dp[d * dplane] = sp[d * splane];
}

int level_up(int msg_type, const BpMsgs &src, int src_rows, const BpMsgs &dst, int dst_rows, int dst_cols, int ndisp, hipStream_t s)
{
    const dim3 grid(div_up(dst_cols, 64), div_up(dst_rows, 4), 4), block(64, 4);
    if (msg_type == SBP_MSG_32F)
        hipLaunchKernelGGL(k_sbp_level_up<float>, grid, block, 0, s, msgs_of<float>(src), src_rows, msgs_of<float>(dst), dst_rows, dst_cols, ndisp);
    else
        hipLaunchKernelGGL(k_sbp_level_up<short>, grid, block, 0, s, msgs_of<short>(src), src_rows, msgs_of<short>(dst), dst_rows, dst_cols, ndisp);
    MI_HIP_TRY(hipGetLastError());
    return MI_OK;
}

// ---------------------------------------------------------------- one_iteration, stereobp.cu:358-450
// The pixel a lane updates in half-sweep t: x = 2 i + ((y + t) & 1), interior only; rows 1 .. rows - 2 are blockIdx.y + 1.
__device__ __forceinline__ bool iter_pixel(int rows, int cols, int t, int *x, int *y)
{
    *y = blockIdx.y + 1;
    *x = ((blockIdx.x * 64 + threadIdx.x) << 1) + ((*y + t) & 1);
    return *x > 0 && *x < cols - 1;
}

// message() from its sums on, all in registers.  s[i], i < n: the f32 sum ((m1 + m2) + m3) + data of disparity i.  Every
// "store through T, read back" of the reference is thru<T>() at the place of that store; the value is written once, at the end.
template <class T, int CAP>
__device__ __forceinline__ void message_reg(float (&s)[CAP], int n, T *dst, long long plane, float max_disc_term, float jump)
{
    float minimum = FLT_MAX;
#pragma unroll
    for (int i = 0; i < CAP; ++i)
        if (i < n) {
            if (s[i] < minimum) minimum = s[i];   // of the unstored sums (:401-404)
            s[i] = thru<T>(s[i]);
        }
    // calc_min_linear_penalty (:358-387): prev carries the unrounded value, the element the rounded one
    float prev = s[0];
#pragma unroll
    for (int i = 1; i < CAP; ++i)
        if (i < n) {
            prev += jump;
            float cur = s[i];
            if (prev < cur) { cur = prev; s[i] = thru<T>(prev); }
            prev = cur;
        }
#pragma unroll
    for (int i = CAP - 1; i >= 0; --i) {
        if (i == n - 1) prev = s[i];
        else if (i < n - 1) {
            prev += jump;
            float cur = s[i];
            if (prev < cur) { cur = prev; s[i] = thru<T>(prev); }
            prev = cur;
        }
    }
    minimum += max_disc_term;
    float sum = 0;
#pragma unroll
    for (int i = 0; i < CAP; ++i)
        if (i < n) {
            float v = s[i];
            if (v > minimum) { v = minimum; s[i] = thru<T>(minimum); }
            sum += v;
        }
    sum /= (float)n;   // IEEE division (hipcc's default for f32 '/')
#pragma unroll
    for (int i = 0; i < CAP; ++i)
        if (i < n) dst[i * plane] = sub<T>(s[i], sum);
}

// Register form.  f32: the five inputs of a pixel are read once per disparity and feed the four sums, 4 x CAP values per lane (343
// VGPRs at CAP 64: one wave per SIMD).  16-bit: two passes of two sums each (u, d; then r, l -- the second pass reads the five inputs
// again, from the cache): 166 VGPRs, three waves per SIMD, 0.138 ms against 0.253 ms per 640 x 480 x 64 half-sweep; for f32 the two
// passes (228 VGPRs, two waves) measured no faster at level 0 (0.297 / 0.294 ms) and 7 % slower over a whole compute.
template <class T, int CAP>
__global__ __launch_bounds__(64) void k_sbp_iterate_reg(Msgs<T> m, const T *data, long long dstep, int rows, int cols, int t, BpConst c)
{
    int x, y;
    if (!iter_pixel(rows, cols, t, &x, &y)) return;
    const int n = c.ndisp;
    const long long plane = m.step * rows, dplane = dstep * rows, off = y * m.step + x;
    const T *ub = m.u + off + m.step, *db = m.d + off - m.step, *lb = m.l + off + 1, *rb = m.r + off - 1, *dt = data + y * dstep + x;
    if constexpr (sizeof(T) == 2) {
        float su[CAP], sd[CAP];
#pragma unroll
        for (int i = 0; i < CAP; ++i)
            if (i < n) {
                const float a = (float)ub[i * plane], b = (float)db[i * plane], e = (float)lb[i * plane], f = (float)rb[i * plane];
                const float g = (float)dt[i * dplane];
                su[i] = ((a + e) + f) + g;
                sd[i] = ((b + e) + f) + g;
            }
        message_reg<T, CAP>(su, n, m.u + off, plane, c.max_disc_term, c.disc_single_jump);
        message_reg<T, CAP>(sd, n, m.d + off, plane, c.max_disc_term, c.disc_single_jump);
        float sr[CAP], sl[CAP];
#pragma unroll
        for (int i = 0; i < CAP; ++i)
            if (i < n) {
                const float a = (float)ub[i * plane], b = (float)db[i * plane], e = (float)lb[i * plane], f = (float)rb[i * plane];
                const float g = (float)dt[i * dplane];
                sr[i] = ((a + b) + f) + g;
                sl[i] = ((a + b) + e) + g;
            }
        message_reg<T, CAP>(sr, n, m.r + off, plane, c.max_disc_term, c.disc_single_jump);
        message_reg<T, CAP>(sl, n, m.l + off, plane, c.max_disc_term, c.disc_single_jump);
    } else {
        float su[CAP], sd[CAP], sr[CAP], sl[CAP];
#pragma unroll
        for (int i = 0; i < CAP; ++i)
            if (i < n) {
                const float a = (float)ub[i * plane], b = (float)db[i * plane], e = (float)lb[i * plane], f = (float)rb[i * plane];
                const float g = (float)dt[i * dplane];
                su[i] = ((a + e) + f) + g;   // message(us + step, ls + 1, rs - 1, dt, us)  :445
                sd[i] = ((b + e) + f) + g;   // message(ds - step, ls + 1, rs - 1, dt, ds)  :446
                sr[i] = ((a + b) + f) + g;   // message(us + step, ds - step, rs - 1, dt, rs)  :447
                sl[i] = ((a + b) + e) + g;   // message(us + step, ds - step, ls + 1, dt, ls)  :448
            }
        message_reg<T, CAP>(su, n, m.u + off, plane, c.max_disc_term, c.disc_single_jump);
        message_reg<T, CAP>(sd, n, m.d + off, plane, c.max_disc_term, c.disc_single_jump);
        message_reg<T, CAP>(sr, n, m.r + off, plane, c.max_disc_term, c.disc_single_jump);
        message_reg<T, CAP>(sl, n, m.l + off, plane, c.max_disc_term, c.disc_single_jump);
    }
}

// General form, any ndisp: the message lives in global memory between its passes, as stereobp.cu:389-426 has it.  No lane reads an
// element another lane of the launch writes: all reads of neighbours are of the other checkerboard colour.
template <class T>
__device__ void message_gen(const T *m1, const T *m2, const T *m3, const T *data, T *dst, long long plane, long long dplane, int n,
                            float max_disc_term, float jump)
{
    float minimum = FLT_MAX;
    for (int i = 0; i < n; ++i) {
        float v = (float)m1[i * plane];
        v += (float)m2[i * plane];
        v += (float)m3[i * plane];
        v += (float)data[i * dplane];
        if (v < minimum) minimum = v;
        dst[i * plane] = sat<T>(v);
    }
    float prev = (float)dst[0];
    for (int i = 1; i < n; ++i) {
        prev += jump;
        float cur = (float)dst[i * plane];
        if (prev < cur) { cur = prev; dst[i * plane] = sat<T>(prev); }
        prev = cur;
    }
    prev = (float)dst[(n - 1) * plane];
    for (int i = n - 2; i >= 0; --i) {
        prev += jump;
        float cur = (float)dst[i * plane];
        if (prev < cur) { cur = prev; dst[i * plane] = sat<T>(prev); }
        prev = cur;
    }
    minimum += max_disc_term;
    float sum = 0;
    for (int i = 0; i < n; ++i) {
        float v = (float)dst[i * plane];
        if (v > minimum) { v = minimum; dst[i * plane] = sat<T>(minimum); }
        sum += v;
    }
    sum /= (float)n;
    for (int i = 0; i < n; ++i) dst[i * plane] = sub<T>((float)dst[i * plane], sum);
}

template <class T>
__global__ __launch_bounds__(64) void k_sbp_iterate_gen(Msgs<T> m, const T *data, long long dstep, int rows, int cols, int t, BpConst c)
{
    int x, y;
    if (!iter_pixel(rows, cols, t, &x, &y)) return;
    const long long plane = m.step * rows, dplane = dstep * rows, off = y * m.step + x;
    T *us = m.u + off, *ds = m.d + off, *ls = m.l + off, *rs = m.r + off;
    const T *dt = data + y * dstep + x;
    message_gen(us + m.step, ls + 1, rs - 1, dt, us, plane, dplane, c.ndisp, c.max_disc_term, c.disc_single_jump);
    message_gen(ds - m.step, ls + 1, rs - 1, dt, ds, plane, dplane, c.ndisp, c.max_disc_term, c.disc_single_jump);
    message_gen(us + m.step, ds - m.step, rs - 1, dt, rs, plane, dplane, c.ndisp, c.max_disc_term, c.disc_single_jump);
    message_gen(us + m.step, ds - m.step, ls + 1, dt, ls, plane, dplane, c.ndisp, c.max_disc_term, c.disc_single_jump);
}

template <class T>
static int launch_iterate(int form, int cap, const BpMsgs &m, const void *data, long long dstep, int rows, int cols, int t,
                          const BpConst &c, hipStream_t s)
{
    if (rows < 3 || cols < 3) return MI_OK;   // no interior pixel
    const dim3 grid(div_up(div_up(cols, 2), 64), rows - 2), block(64);
    const Msgs<T> mm = msgs_of<T>(m);
    const T *dt = (const T *)data;
    if (form == SBP_FORM_GEN) hipLaunchKernelGGL(k_sbp_iterate_gen<T>, grid, block, 0, s, mm, dt, dstep, rows, cols, t, c);
    else if (form == SBP_FORM_REG && cap == 16 && c.ndisp <= 16) hipLaunchKernelGGL((k_sbp_iterate_reg<T, 16>), grid, block, 0, s, mm, dt, dstep, rows, cols, t, c);
    else if (form == SBP_FORM_REG && cap == 32 && c.ndisp <= 32) hipLaunchKernelGGL((k_sbp_iterate_reg<T, 32>), grid, block, 0, s, mm, dt, dstep, rows, cols, t, c);
    else if (form == SBP_FORM_REG && cap == 64 && c.ndisp <= 64) hipLaunchKernelGGL((k_sbp_iterate_reg<T, 64>), grid, block, 0, s, mm, dt, dstep, rows, cols, t, c);
    else MI_REQUIRE(false, MI_ERR_BAD_ARG, "no iteration kernel of form %d, capacity %d for %d disparities", form, cap, c.ndisp);
    MI_HIP_TRY(hipGetLastError());
    return MI_OK;
}

int iterate(int msg_type, int form, int cap, const BpMsgs &m, const void *data, long long dstep, int rows, int cols, int t,
            const BpConst &c, hipStream_t s)
{
    return msg_type == SBP_MSG_32F ? launch_iterate<float>(form, cap, m, data, dstep, rows, cols, t, c, s)
                                   : launch_iterate<short>(form, cap, m, data, dstep, rows, cols, t, c, s);
}

// ---------------------------------------------------------------- output, stereobp.cu:481-517, with the border fill and the conversion
// saturate_cast<O>(short) of convertTo: the winner is in [0, ndisp), so only uchar can clamp
template <class O> __device__ __forceinline__ O out_cast(int best) { return (O)(short)min(best, 32767); }
template <> __device__ __forceinline__ unsigned char out_cast<unsigned char>(int best) { return (unsigned char)min((int)(short)min(best, 32767), 255); }

template <class T, class O>
__global__ __launch_bounds__(256) void k_sbp_output(Msgs<T> m, const T *data, long long dstep, int rows, int cols, int ndisp, O *disp, long long ostep)
{
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (!(x < cols && y < rows)) return;
    O *o = (O *)((char *)disp + y * ostep) + x;
    if (!(y > 0 && y < rows - 1 && x > 0 && x < cols - 1)) { *o = (O)0; return; }   // out.setTo(0)  stereobp.cpp:353
    const long long plane = m.step * rows, dplane = dstep * rows, off = y * m.step + x;
    const T *us = m.u + off + m.step, *ds = m.d + off - m.step, *ls = m.l + off + 1, *rs = m.r + off - 1, *dt = data + y * dstep + x;
    int best = 0;
    float best_val = FLT_MAX;
    for (int d = 0; d < ndisp; ++d) {
        float v = (float)us[d * plane];
        v += (float)ds[d * plane];
        v += (float)ls[d * plane];
        v += (float)rs[d * plane];
        v += (float)dt[d * dplane];
        if (v < best_val) { best_val = v; best = d; }
    }
    *o = out_cast<O>(best);
}

template <class T, class O>
static int launch_output(const BpMsgs &m, const void *data, long long dstep, int rows, int cols, int ndisp, void *disp, long long ostep, hipStream_t s)
{
    hipLaunchKernelGGL((k_sbp_output<T, O>), dim3(div_up(cols, 64), div_up(rows, 4)), dim3(64, 4), 0, s, msgs_of<T>(m), (const T *)data, dstep,
                       rows, cols, ndisp, (O *)disp, ostep);
    MI_HIP_TRY(hipGetLastError());
    return MI_OK;
}
template <class T>
static int output_t(const BpMsgs &m, const void *data, long long dstep, int rows, int cols, int ndisp, void *disp, long long ostep, int out_type, hipStream_t s)
{
    switch (out_type) {
    case MI_16SC1: return launch_output<T, short>(m, data, dstep, rows, cols, ndisp, disp, ostep, s);
    case MI_8UC1: return launch_output<T, unsigned char>(m, data, dstep, rows, cols, ndisp, disp, ostep, s);
    case MI_32SC1: return launch_output<T, int>(m, data, dstep, rows, cols, ndisp, disp, ostep, s);
    case MI_32FC1: return launch_output<T, float>(m, data, dstep, rows, cols, ndisp, disp, ostep, s);
    }
    MI_REQUIRE(false, MI_ERR_BAD_TYPE, "disparity: must be CV_16SC1, CV_8UC1, CV_32SC1 or CV_32FC1");
}

int output(int msg_type, const BpMsgs &m, const void *data, long long dstep, int rows, int cols, int ndisp, void *disp, long long ostep,
           int out_type, hipStream_t s)
{
    return msg_type == SBP_MSG_32F ? output_t<float>(m, data, dstep, rows, cols, ndisp, disp, ostep, out_type, s)
                                   : output_t<short>(m, data, dstep, rows, cols, ndisp, disp, ostep, out_type, s);
}

}  // namespace sbp
}  // namespace mi
