// Internal launch API of the BroxOpticalFlow HIP kernels (brox_kernels.hip).  Not part of the C-ABI.
// Geometry (grids, tiles, forms) is the plan's (brox_plan.h); each function launches exactly one kernel.
#pragma once
#include "mi_common.h"
#include "brox_plan.h"

namespace mi {
namespace brox {

inline int brox_fail(const BroxErr &e) { MI_REQUIRE(e.code == MI_OK, e.code, "%s", e.msg); return MI_OK; }

// a float plane: row pitch in floats, any 4-byte-aligned base
struct Plane { float *p; long long ld; };
struct CPlane { const float *p; long long ld; };
__host__ __device__ inline CPlane cp(const Plane &a) { return {a.p, a.ld}; }

// the nine images of a level as prepare_sor_stage_1_tex names them (NCVBroxOpticalFlow.cu:340)
struct Images { CPlane i0, i1, ix, ixx, ix0, iy, iyy, iy0, ixy; };
// the seven coefficient planes (:341); denu / denv hold the inverse denominators after stage 2
struct Coeffs { Plane diffx, diffy, denu, denv, ndudv, nu, nv; };
struct DerivJob { CPlane src; Plane dst; int column; };
struct DerivJobs { DerivJob j[4]; };

// resizeSuperSample_32f (NPP_staging.cu:2073-2149) on n planes (gz); scale = 1 / scale_factor as the launch site forms it (:2265)
int resize_down(const BroxLaunch &k, const CPlane *src, int sw, int sh, const Plane *dst, int dw, int dh, float scale, hipStream_t st);
// resizeBicubic (:2152-2231) and scaleVector (NCVBroxOpticalFlow.cu:145-152) on n planes; the source is a + b where b is given (the
// `add` of :929-931 taken into the read: one rounding either way)
int resize_up(const BroxLaunch &k, const CPlane *a, const CPlane *b, int sw, int sh, const Plane *dst, int dw, int dh, float scale, float mul,
              hipStream_t st);
// FilterRowBorderMirror_32f_C1R / FilterColumnBorderMirror_32f_C1R (NPP_staging.cu:1433-1501), one job per gz
int derivatives(const BroxLaunch &k, const DerivJobs &jobs, int w, int h, hipStream_t st);
int zero2(const BroxLaunch &k, const Plane &a, const Plane &b, int w, int h, hipStream_t st);
// prepare_sor_stage_1_tex (NCVBroxOpticalFlow.cu:340-406) and prepare_sor_stage_2 (:416-473)
int prepare1(const BroxLaunch &k, const CPlane &u, const CPlane &v, const CPlane &du, const CPlane &dv, const Images &im, const Coeffs &c, int w,
             int h, float alpha, float gamma, hipStream_t st);
int prepare2(const BroxLaunch &k, const Coeffs &c, int w, int h, hipStream_t st);
// sor_pass<colour> (:479-554): du, dv -> du_new, dv_new
struct SorArgs { CPlane u, v, du, dv; Plane du_new, dv_new; CPlane diffx, diffy, idenu, idenv, ndudv, nu, nv; int w, h; };
int sor_plain(const BroxLaunch &k, const SorArgs &a, hipStream_t st);
// both colours of k.arg <= BROX_SOR_KMAX solver iterations over an LDS tile with a halo of 2 pixels per iteration
int sor_blocked(const BroxLaunch &k, const SorArgs &a, hipStream_t st);
// pointwise_add (:101-108) of both components and the interleave into the caller's CV_32FC2 (brox.cpp:183-185); step in floats
int add_out(const BroxLaunch &k, const CPlane &u, const CPlane &du, const CPlane &v, const CPlane &dv, float *flow, long long flow_ld, int w, int h,
            hipStream_t st);

}  // namespace brox
}  // namespace mi
