// cv::cuda::BroxOpticalFlow on gfx950.  Every kernel follows its reference kernel operation by operation and left to right; the file is
// compiled without contraction, and `/` and sqrtf are the correctly rounded ones.  No textures: the reference's 1-D fetches are plain
// loads, its normalised 2-D reads are tex_linear / tex_point below, which are DEFINITIONS, as is rsqrtf = 1 / sqrtf.
// Wave64: a 64 x 4 workgroup is four waves, each on one row segment, so every plane access of a wave is one contiguous 256-byte row.
#include "brox_dev.h"

namespace mi {
namespace brox {
namespace {

constexpr float EPS2 = 1e-6f;   // NCVBroxOpticalFlow.cu:78

struct Planes2 { CPlane a[2], b[2]; Plane d[2]; };

__device__ __forceinline__ float at(const CPlane &p, int y, int x) { return p.p[(long long)y * p.ld + x]; }

// cudaAddressModeMirror on normalised coordinates: periodic with period 2N
__device__ __forceinline__ int mirror_periodic(int k, int n)
{
    int m = k % (2 * n);
    if (m < 0) m += 2 * n;
    return m < n ? m : 2 * n - 1 - m;
}

// normalised, cudaFilterModeLinear, cudaAddressModeMirror: the sample point moves back by half a texel, the weights are 1.8 fixed point
__device__ __forceinline__ float tex_linear(const CPlane &t, int w, int h, float yn, float xn)
{
    const float xb = xn * (float)w - 0.5f, yb = yn * (float)h - 0.5f;
    const float fi = floorf(xb), fj = floorf(yb);
    const int i = (int)fi, j = (int)fj;
    const float a = floorf((xb - fi) * 256.0f + 0.5f) / 256.0f, b = floorf((yb - fj) * 256.0f + 0.5f) / 256.0f;
    const int i0 = mirror_periodic(i, w), i1 = mirror_periodic(i + 1, w), j0 = mirror_periodic(j, h), j1 = mirror_periodic(j + 1, h);
    return (1.0f - a) * (1.0f - b) * at(t, j0, i0) + a * (1.0f - b) * at(t, j0, i1) + (1.0f - a) * b * at(t, j1, i0) + a * b * at(t, j1, i1);
}

// load_array_element's mirror (NCVBroxOpticalFlow.cu:243-246)
__device__ __forceinline__ int mirror_sym(int i, int n)
{
    i = max(i, -i - 1);
    return min(i, n - i + n - 1);
}

// ------------------------------------------------------------------ resizeSuperSample_32f, NPP_staging.cu:2073-2149
__device__ __forceinline__ float process_line(const float *row, float xmin, float xmax, int ixmin, int ixmax, float fxmin, float cxmax)
{
    int spos = ixmin;
    float wsum = 1.0f - xmin + fxmin;
    float sum = row[spos] * (1.0f - xmin + fxmin);
    spos++;
    for (int ix = ixmin + 1; ix < ixmax; ++ix) {
        sum += row[spos];
        spos++;
        wsum += 1.0f;
    }
    sum += row[spos] * (cxmax - xmax);
    wsum += cxmax - xmax;
    return sum / wsum;
}

__global__ __launch_bounds__(256) void k_brox_resize_down(Planes2 P, int sw, int sh, int dw, int dh, float scale)
{
    const int ix = blockIdx.x * blockDim.x + threadIdx.x, iy = blockIdx.y * blockDim.y + threadIdx.y;
    if (ix >= dw || iy >= dh) return;
    const CPlane src = P.a[blockIdx.z];
    const Plane dst = P.d[blockIdx.z];
    const float rw = (float)sw, rh = (float)sh;
    const float x = scale * (float)ix, y = scale * (float)iy;
    const float xBegin = fmaxf(x - scale, 0.0f), xEnd = fminf(x + scale, rw - 1.0f);
    const float yBegin = fmaxf(y - scale, 0.0f), yEnd = fminf(y + scale, rh - 1.0f);
    const float floorXBegin = floorf(xBegin), ceilXEnd = ceilf(xEnd), floorYBegin = floorf(yBegin), ceilYEnd = ceilf(yEnd);
    // a window reads up to max(begin + 1, end); brox_resize_down_fits (brox_plan.h) holds that inside the source before any launch
    const int iXBegin = (int)floorXBegin, iXEnd = (int)ceilXEnd, iYBegin = (int)floorYBegin, iYEnd = (int)ceilYEnd;
    const float *row = src.p + (long long)iYBegin * src.ld;
    float wsum = 1.0f - yBegin + floorYBegin;
    float sum = process_line(row, xBegin, xEnd, iXBegin, iXEnd, floorXBegin, ceilXEnd) * (1.0f - yBegin + floorYBegin);
    row += src.ld;
    for (int yy = iYBegin + 1; yy < iYEnd; ++yy) {
        sum += process_line(row, xBegin, xEnd, iXBegin, iXEnd, floorXBegin, ceilXEnd);
        row += src.ld;
        wsum += 1.0f;
    }
    sum += process_line(row, xBegin, xEnd, iXBegin, iXEnd, floorXBegin, ceilXEnd) * (ceilYEnd - yEnd);
    wsum += ceilYEnd - yEnd;
    sum /= wsum;
    dst.p[(long long)iy * dst.ld + ix] = sum;
}

// ------------------------------------------------------------------ resizeBicubic, NPP_staging.cu:2152-2231
__device__ __forceinline__ float bicubic_coeff(float x_)
{
    const float x = fabsf(x_);
    if (x <= 1.0f) return x * x * (1.5f * x - 2.5f) + 1.0f;
    if (x < 2.0f) return x * (x * (-0.5f * x + 2.5f) - 4.0f) + 2.0f;
    return 0.0f;
}

__global__ __launch_bounds__(256) void k_brox_resize_up(Planes2 P, int sw, int sh, int dw, int dh, float scale, float mul)
{
    const int ix = blockIdx.x * blockDim.x + threadIdx.x, iy = blockIdx.y * blockDim.y + threadIdx.y;
    if (ix >= dw || iy >= dh) return;
    const CPlane a = P.a[blockIdx.z], b = P.b[blockIdx.z];
    const Plane dst = P.d[blockIdx.z];
    const float dx = 1.0f / sw, dy = 1.0f / sh;
    const float rw = (float)sw, rh = (float)sh;
    float x = scale * (float)ix, y = scale * (float)iy;
    float xmin = fmaxf(ceilf(x - 2.0f), 0.0f), xmax = fminf(floorf(x + 2.0f), rw - 1.0f);
    float ymin = fmaxf(ceilf(y - 2.0f), 0.0f), ymax = fminf(floorf(y + 2.0f), rh - 1.0f);
    x += 0.5f; y += 0.5f;
    xmin += 0.5f; xmax += 0.5f; ymin += 0.5f; ymax += 0.5f;
    float sum = 0.0f, wsum = 0.0f;
    for (float cy = ymin; cy <= ymax; cy += 1.0f) {
        for (float cx = xmin; cx <= xmax; cx += 1.0f) {
            const float xDist = x - cx, yDist = y - cy;
            float wx = bicubic_coeff(xDist);
            const float wy = bicubic_coeff(yDist);
            wx *= wy;
            // normalised, cudaFilterModePoint, cudaAddressModeMirror: texel floor(xn * W)
            const int tx = mirror_periodic((int)floorf(cx * dx * rw), sw), ty = mirror_periodic((int)floorf(cy * dy * rh), sh);
            float t = at(a, ty, tx);
            if (b.p) t = t + at(b, ty, tx);
            sum += wx * t;
            wsum += wx;
        }
    }
    const float r = (!wsum) ? 0.0f : sum / wsum;
    dst.p[(long long)iy * dst.ld + ix] = r * mul;
}

// ------------------------------------------------------------------ the 5-tap derivative filter, NPP_staging.cu:1433-1501
__global__ __launch_bounds__(256) void k_brox_deriv(DerivJobs J, int w, int h)
{
    const int ix = blockIdx.x * blockDim.x + threadIdx.x, iy = blockIdx.y * blockDim.y + threadIdx.y;
    if (ix >= w || iy >= h) return;
    const DerivJob job = J.j[blockIdx.z];
    const float taps[5] = {1.0f, -8.0f, 0.0f, 8.0f, -1.0f};   // NCVBroxOpticalFlow.cu:689
    const int n = job.column ? h : w, c = job.column ? iy : ix;
    float sum = 0.0f;
#pragma unroll
    for (int m = 0; m < 5; ++m) {
        int i = c + m - 2;
        if (i < 0) i = 1 - i;            // the reference's mirror is asymmetric: -1 -> 2, -2 -> 3
        if (i >= n) i = n + n - i - 1;
        sum += (job.column ? at(job.src, i, ix) : at(job.src, iy, i)) * taps[m];
    }
    job.dst.p[(long long)iy * job.dst.ld + ix] = sum * (1.0f / 12.0f);
}

__global__ __launch_bounds__(256) void k_brox_zero2(Plane a, Plane b, int w, int h)
{
    const int ix = blockIdx.x * blockDim.x + threadIdx.x, iy = blockIdx.y * blockDim.y + threadIdx.y;
    if (ix >= w || iy >= h) return;
    a.p[(long long)iy * a.ld + ix] = 0.0f;
    b.p[(long long)iy * b.ld + ix] = 0.0f;
}

// ------------------------------------------------------------------ prepare_sor_stage_1_tex, NCVBroxOpticalFlow.cu:188-227,340-406
struct Flow4 { CPlane u, v, du, dv; };

__global__ __launch_bounds__(256) void k_brox_prepare1(Flow4 F, Images I, Coeffs C, int w, int h, float alpha, float gamma)
{
    const int ig = blockIdx.x * blockDim.x + threadIdx.x, jg = blockIdx.y * blockDim.y + threadIdx.y;
    if (ig >= w || jg >= h) return;
    // the tile with its halo of load_array: the pixel, its row below (j - 1) and above (j + 1), columns i - 1 .. i + 1, mirrored
    const int xl = mirror_sym(ig - 1, w), xr = mirror_sym(ig + 1, w), yd = mirror_sym(jg - 1, h), yu = mirror_sym(jg + 1, h);
#define BROX_LOAD9(name, P) \
    const float name##_c = at(P, jg, ig), name##_l = at(P, jg, xl), name##_r = at(P, jg, xr), name##_u = at(P, yu, ig), name##_ul = at(P, yu, xl), \
                name##_d = at(P, yd, ig), name##_dl = at(P, yd, xl), name##_dr = at(P, yd, xr)
    BROX_LOAD9(u, F.u);
    BROX_LOAD9(v, F.v);
    BROX_LOAD9(du, F.du);
    BROX_LOAD9(dv, F.dv);
#undef BROX_LOAD9
    float x = (float)ig + 0.5f, y = (float)jg + 0.5f;
    const float wx = (x + u_c) / (float)w, wy = (y + v_c) / (float)h;
    x /= (float)w;
    y /= (float)h;
    const float Iz = tex_linear(I.i1, w, h, wy, wx) - tex_linear(I.i0, w, h, y, x);
    const float Ix = tex_linear(I.ix, w, h, wy, wx);
    const float Ixz = Ix - tex_linear(I.ix0, w, h, y, x);
    const float Ixy = tex_linear(I.ixy, w, h, wy, wx);
    const float Ixx = tex_linear(I.ixx, w, h, wy, wx);
    const float Iy = tex_linear(I.iy, w, h, wy, wx);
    const float Iyz = Iy - tex_linear(I.iy0, w, h, y, x);
    const float Iyy = tex_linear(I.iyy, w, h, wy, wx);
    const float q0 = Iz + Ix * du_c + Iy * dv_c;
    const float q1 = Ixz + Ixx * du_c + Ixy * dv_c;
    const float q2 = Iyz + Ixy * du_c + Iyy * dv_c;
    float data_term = 0.5f * (1.0f / sqrtf(q0 * q0 + gamma * (q1 * q1 + q2 * q2) + EPS2));   // rsqrtf(x) is DEFINED as 1 / sqrtf(x)
    data_term /= alpha;
    float sx, sy;
    {   // diffusivity_along_x
        const float u_x = u_c + du_c - u_l - du_l;
        const float v_x = v_c + dv_c - v_l - dv_l;
        const float u_y = 0.25f * (u_u + du_u + u_ul + du_ul - u_d - du_d - u_dl - du_dl);
        const float v_y = 0.25f * (v_u + dv_u + v_ul + dv_ul - v_d - dv_d - v_dl - dv_dl);
        sx = 0.5f / sqrtf(u_x * u_x + v_x * v_x + u_y * u_y + v_y * v_y + EPS2);
    }
    {   // diffusivity_along_y
        const float u_y = u_c + du_c - u_d - du_d;
        const float v_y = v_c + dv_c - v_d - dv_d;
        const float u_x = 0.25f * (u_r + u_dr + du_r + du_dr - u_l - u_dl - du_l - du_dl);
        const float v_x = 0.25f * (v_r + v_dr + dv_r + dv_dr - v_l - v_dl - dv_l - dv_dl);
        sy = 0.5f / sqrtf(u_x * u_x + v_x * v_x + u_y * u_y + v_y * v_y + EPS2);
    }
    if (ig == 0) sx = 0.0f;
    if (jg == 0) sy = 0.0f;
#define BROX_ST(P, val) P.p[(long long)jg * P.ld + ig] = (val)
    BROX_ST(C.ndudv, data_term * (Ix * Iy + gamma * Ixy * (Ixx + Iyy)));
    BROX_ST(C.nu, data_term * (Ix * Iz + gamma * (Ixx * Ixz + Ixy * Iyz)));
    BROX_ST(C.nv, data_term * (Iy * Iz + gamma * (Iyy * Iyz + Ixy * Ixz)));
    BROX_ST(C.denu, data_term * (Ix * Ix + gamma * (Ixy * Ixy + Ixx * Ixx)));
    BROX_ST(C.denv, data_term * (Iy * Iy + gamma * (Ixy * Ixy + Iyy * Iyy)));
    BROX_ST(C.diffx, sx);
    BROX_ST(C.diffy, sy);
}

// ------------------------------------------------------------------ prepare_sor_stage_2, NCVBroxOpticalFlow.cu:416-473
__global__ __launch_bounds__(256) void k_brox_prepare2(Coeffs C, int w, int h)
{
    const int ig = blockIdx.x * blockDim.x + threadIdx.x, jg = blockIdx.y * blockDim.y + threadIdx.y;
    if (ig >= w || jg >= h) return;
    const float sx = at(cp(C.diffx), jg, ig), sy = at(cp(C.diffy), jg, ig);
    const float sx_r = ig < w - 1 ? at(cp(C.diffx), jg, ig + 1) : 0.0f;
    const float sy_u = jg < h - 1 ? at(cp(C.diffy), jg + 1, ig) : 0.0f;
    const float diffusivity_sum = sx + sx_r + sy + sy_u;
    float denom_u = at(cp(C.denu), jg, ig), denom_v = at(cp(C.denv), jg, ig);
    denom_u += diffusivity_sum;
    denom_v += diffusivity_sum;
    BROX_ST(C.denu, 1.0f / denom_u);
    BROX_ST(C.denv, 1.0f / denom_v);
}
#undef BROX_ST

// ------------------------------------------------------------------ sor_pass, NCVBroxOpticalFlow.cu:479-554
// one pixel's update from its four neighbours' u + du, v + dv: the arithmetic both forms share
struct SorNb { float u_l, u_r, u_d, u_u, u, v_l, v_r, v_d, v_u, v, du_l, du_r, du_d, du_u, dv_l, dv_r, dv_d, dv_u;
               float s_left, s_down, s_right, s_up, idenu, idenv, nu, nv, ndudv; };

__device__ __forceinline__ void sor_update(const SorNb &n, float &du, float &dv)
{
    const float omega = 1.99f;
    const float numerator_u = (n.s_left * (n.u_l + n.du_l) + n.s_up * (n.u_u + n.du_u) + n.s_right * (n.u_r + n.du_r) + n.s_down * (n.u_d + n.du_d) -
                               n.u * (n.s_left + n.s_right + n.s_up + n.s_down) - n.nu - n.ndudv * dv);
    du = (1.0f - omega) * du + omega * n.idenu * numerator_u;
    const float numerator_v = (n.s_left * (n.v_l + n.dv_l) + n.s_up * (n.v_u + n.dv_u) + n.s_right * (n.v_r + n.dv_r) + n.s_down * (n.v_d + n.dv_d) -
                               n.v * (n.s_left + n.s_right + n.s_up + n.s_down) - n.nv - n.ndudv * du);
    dv = (1.0f - omega) * dv + omega * n.idenv * numerator_v;
}

__global__ __launch_bounds__(256) void k_brox_sor_plain(SorArgs A, int colour)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x, j = blockIdx.y * blockDim.y + threadIdx.y;
    if (i >= A.w || j >= A.h) return;
    float du = at(A.du, j, i), dv = at(A.dv, j, i);
    if ((i + j) % 2 == colour) {
        const int ir = i < A.w - 1 ? i + 1 : i, il = i > 0 ? i - 1 : i, ju = j < A.h - 1 ? j + 1 : j, jd = j > 0 ? j - 1 : j;
        SorNb n;
        n.s_left = at(A.diffx, j, i);
        n.s_down = at(A.diffy, j, i);
        n.s_right = i < A.w - 1 ? at(A.diffx, j, ir) : 0.0f;   // Neumann
        n.s_up = j < A.h - 1 ? at(A.diffy, ju, i) : 0.0f;
        n.u_l = at(A.u, j, il); n.u_r = at(A.u, j, ir); n.u_d = at(A.u, jd, i); n.u_u = at(A.u, ju, i); n.u = at(A.u, j, i);
        n.v_l = at(A.v, j, il); n.v_r = at(A.v, j, ir); n.v_d = at(A.v, jd, i); n.v_u = at(A.v, ju, i); n.v = at(A.v, j, i);
        n.du_l = at(A.du, j, il); n.du_r = at(A.du, j, ir); n.du_d = at(A.du, jd, i); n.du_u = at(A.du, ju, i);
        n.dv_l = at(A.dv, j, il); n.dv_r = at(A.dv, j, ir); n.dv_d = at(A.dv, jd, i); n.dv_u = at(A.dv, ju, i);
        n.idenu = at(A.idenu, j, i); n.idenv = at(A.idenv, j, i); n.nu = at(A.nu, j, i); n.nv = at(A.nv, j, i); n.ndudv = at(A.ndudv, j, i);
        sor_update(n, du, dv);
    }
    A.du_new.p[(long long)j * A.du_new.ld + i] = du;
    A.dv_new.p[(long long)j * A.dv_new.ld + i] = dv;
}

// The blocked form.  A workgroup holds u, v, du, dv and both diffusivities of a (64 + 8) x (16 + 8) tile in LDS and runs the 2 k
// half-passes of k <= 2 solver iterations on it.  Half-pass t (t = 0 .. 2k - 1) is valid on the tile shrunk by t + 1 pixels; a tile
// side that reaches the frame border does not shrink there, because sor_pass clamps a border pixel's neighbour to the pixel itself, so
// nothing outside the frame is read.  The two colours touch disjoint pixels and a pixel reads only the other colour, so the update
// is in place with one barrier per half-pass.  The per-pixel expression is sor_update, the plain form's: the same bits.
__global__ __launch_bounds__(BROX_SOR_THREADS) void k_brox_sor_blocked(SorArgs A, int k)
{
    constexpr int LX = BROX_SOR_LDS_X, LY = BROX_SOR_LDS_Y, N = LX * LY;
    __shared__ float s_u[N], s_v[N], s_du[N], s_dv[N], s_sx[N], s_sy[N];
    const int gx0 = blockIdx.x * BROX_SOR_TILE_X - BROX_SOR_HALO, gy0 = blockIdx.y * BROX_SOR_TILE_Y - BROX_SOR_HALO;
    const int gx1 = gx0 + LX - 1, gy1 = gy0 + LY - 1;
    const int tid = threadIdx.x;
    for (int idx = tid; idx < N; idx += BROX_SOR_THREADS) {
        const int ly = idx / LX, lx = idx - ly * LX, gx = gx0 + lx, gy = gy0 + ly;
        const bool in = gx >= 0 && gx < A.w && gy >= 0 && gy < A.h;
        s_u[idx] = in ? at(A.u, gy, gx) : 0.0f;
        s_v[idx] = in ? at(A.v, gy, gx) : 0.0f;
        s_du[idx] = in ? at(A.du, gy, gx) : 0.0f;
        s_dv[idx] = in ? at(A.dv, gy, gx) : 0.0f;
        s_sx[idx] = in ? at(A.diffx, gy, gx) : 0.0f;
        s_sy[idx] = in ? at(A.diffy, gy, gx) : 0.0f;
    }
    __syncthreads();
    for (int t = 0; t < 2 * k; ++t) {
        const int colour = t & 1;
        const int lox = gx0 < 0 ? 0 : gx0 + t + 1, hix = gx1 >= A.w - 1 ? A.w - 1 : gx1 - (t + 1);
        const int loy = gy0 < 0 ? 0 : gy0 + t + 1, hiy = gy1 >= A.h - 1 ? A.h - 1 : gy1 - (t + 1);
        for (int idx = tid; idx < N; idx += BROX_SOR_THREADS) {
            const int ly = idx / LX, lx = idx - ly * LX, i = gx0 + lx, j = gy0 + ly;
            if (i < lox || i > hix || j < loy || j > hiy || ((i + j) & 1) != colour) continue;
            const int pr = i < A.w - 1 ? idx + 1 : idx, pl = i > 0 ? idx - 1 : idx, pu = j < A.h - 1 ? idx + LX : idx, pd = j > 0 ? idx - LX : idx;
            SorNb n;
            n.s_left = s_sx[idx];
            n.s_down = s_sy[idx];
            n.s_right = i < A.w - 1 ? s_sx[pr] : 0.0f;
            n.s_up = j < A.h - 1 ? s_sy[pu] : 0.0f;
            n.u_l = s_u[pl]; n.u_r = s_u[pr]; n.u_d = s_u[pd]; n.u_u = s_u[pu]; n.u = s_u[idx];
            n.v_l = s_v[pl]; n.v_r = s_v[pr]; n.v_d = s_v[pd]; n.v_u = s_v[pu]; n.v = s_v[idx];
            n.du_l = s_du[pl]; n.du_r = s_du[pr]; n.du_d = s_du[pd]; n.du_u = s_du[pu];
            n.dv_l = s_dv[pl]; n.dv_r = s_dv[pr]; n.dv_d = s_dv[pd]; n.dv_u = s_dv[pu];
            n.idenu = at(A.idenu, j, i); n.idenv = at(A.idenv, j, i); n.nu = at(A.nu, j, i); n.nv = at(A.nv, j, i); n.ndudv = at(A.ndudv, j, i);
            float du = s_du[idx], dv = s_dv[idx];
            sor_update(n, du, dv);
            s_du[idx] = du;
            s_dv[idx] = dv;
        }
        __syncthreads();
    }
    for (int idx = tid; idx < BROX_SOR_TILE_X * BROX_SOR_TILE_Y; idx += BROX_SOR_THREADS) {
        const int ty = idx / BROX_SOR_TILE_X, tx = idx - ty * BROX_SOR_TILE_X;
        const int i = blockIdx.x * BROX_SOR_TILE_X + tx, j = blockIdx.y * BROX_SOR_TILE_Y + ty;
        if (i >= A.w || j >= A.h) continue;
        const int l = (ty + BROX_SOR_HALO) * LX + tx + BROX_SOR_HALO;
        A.du_new.p[(long long)j * A.du_new.ld + i] = s_du[l];
        A.dv_new.p[(long long)j * A.dv_new.ld + i] = s_dv[l];
    }
}

__global__ __launch_bounds__(256) void k_brox_add_out(CPlane u, CPlane du, CPlane v, CPlane dv, float *flow, long long flow_ld, int w, int h)
{
    const int ix = blockIdx.x * blockDim.x + threadIdx.x, iy = blockIdx.y * blockDim.y + threadIdx.y;
    if (ix >= w || iy >= h) return;
    float *o = flow + (long long)iy * flow_ld + 2 * ix;
    o[0] = at(u, iy, ix) + at(du, iy, ix);
    o[1] = at(v, iy, ix) + at(dv, iy, ix);
}

inline dim3 grid_of(const BroxLaunch &k) { return dim3(k.gx, k.gy, k.gz); }
inline dim3 block_of(const BroxLaunch &k) { return k.kernel == BROX_K_SOR_BLOCKED ? dim3(k.threads) : dim3(BROX_BLOCK_X, BROX_BLOCK_Y); }

}  // namespace

int resize_down(const BroxLaunch &k, const CPlane *src, int sw, int sh, const Plane *dst, int dw, int dh, float scale, hipStream_t st)
{
    Planes2 P = {};
    for (unsigned i = 0; i < k.gz && i < 2; ++i) { P.a[i] = src[i]; P.d[i] = dst[i]; }
    hipLaunchKernelGGL(k_brox_resize_down, grid_of(k), block_of(k), 0, st, P, sw, sh, dw, dh, scale);
    MI_HIP_TRY(hipGetLastError());
    return MI_OK;
}

int resize_up(const BroxLaunch &k, const CPlane *a, const CPlane *b, int sw, int sh, const Plane *dst, int dw, int dh, float scale, float mul,
              hipStream_t st)
{
    Planes2 P = {};
    for (unsigned i = 0; i < k.gz && i < 2; ++i) { P.a[i] = a[i]; if (b) P.b[i] = b[i]; P.d[i] = dst[i]; }
    hipLaunchKernelGGL(k_brox_resize_up, grid_of(k), block_of(k), 0, st, P, sw, sh, dw, dh, scale, mul);
    MI_HIP_TRY(hipGetLastError());
    return MI_OK;
}

int derivatives(const BroxLaunch &k, const DerivJobs &jobs, int w, int h, hipStream_t st)
{
    hipLaunchKernelGGL(k_brox_deriv, grid_of(k), block_of(k), 0, st, jobs, w, h);
    MI_HIP_TRY(hipGetLastError());
    return MI_OK;
}

int zero2(const BroxLaunch &k, const Plane &a, const Plane &b, int w, int h, hipStream_t st)
{
    hipLaunchKernelGGL(k_brox_zero2, grid_of(k), block_of(k), 0, st, a, b, w, h);
    MI_HIP_TRY(hipGetLastError());
    return MI_OK;
}

int prepare1(const BroxLaunch &k, const CPlane &u, const CPlane &v, const CPlane &du, const CPlane &dv, const Images &im, const Coeffs &c, int w,
             int h, float alpha, float gamma, hipStream_t st)
{
    const Flow4 F = {u, v, du, dv};
    hipLaunchKernelGGL(k_brox_prepare1, grid_of(k), block_of(k), 0, st, F, im, c, w, h, alpha, gamma);
    MI_HIP_TRY(hipGetLastError());
    return MI_OK;
}

int prepare2(const BroxLaunch &k, const Coeffs &c, int w, int h, hipStream_t st)
{
    hipLaunchKernelGGL(k_brox_prepare2, grid_of(k), block_of(k), 0, st, c, w, h);
    MI_HIP_TRY(hipGetLastError());
    return MI_OK;
}

int sor_plain(const BroxLaunch &k, const SorArgs &a, hipStream_t st)
{
    hipLaunchKernelGGL(k_brox_sor_plain, grid_of(k), block_of(k), 0, st, a, k.arg);
    MI_HIP_TRY(hipGetLastError());
    return MI_OK;
}

int sor_blocked(const BroxLaunch &k, const SorArgs &a, hipStream_t st)
{
    MI_REQUIRE(k.arg >= 1 && k.arg <= BROX_SOR_KMAX, MI_ERR_BAD_ARG, "a blocked launch runs 1 .. %d solver iterations", (int)BROX_SOR_KMAX);
    hipLaunchKernelGGL(k_brox_sor_blocked, grid_of(k), block_of(k), 0, st, a, k.arg);
    MI_HIP_TRY(hipGetLastError());
    return MI_OK;
}

int add_out(const BroxLaunch &k, const CPlane &u, const CPlane &du, const CPlane &v, const CPlane &dv, float *flow, long long flow_ld, int w, int h,
            hipStream_t st)
{
    hipLaunchKernelGGL(k_brox_add_out, grid_of(k), block_of(k), 0, st, u, du, v, dv, flow, flow_ld, w, h);
    MI_HIP_TRY(hipGetLastError());
    return MI_OK;
}

}  // namespace brox
}  // namespace mi
