// Internal launch API of the CornernessCriteria / CornersDetector HIP kernels (gftt_kernels.hip).  Not part of the C-ABI.
// Geometry (forms, tiles, grids, LDS sizes) is the plan's (gftt_plan.h); each function launches exactly one kernel.
#pragma once
#include "mi_common.h"
#include "gftt_plan.h"

namespace mi {
namespace gftt {

inline int gftt_fail(const GfttErr &e) { MI_REQUIRE(e.code == MI_OK, e.code, "%s", e.msg); return MI_OK; }

// the caller's image: MI_8UC1 or MI_32FC1, step in bytes, any base address
struct GfttImage { const unsigned char *data; long long step; int rows, cols, type; };
// what the response depends on besides the image; deriv / smooth: the 3-tap kernels of createSobelFilter (filtering.cpp:524-545), the
// scale already in `smooth`
struct GfttCorner { float deriv[3], smooth[3]; int block_size, border, harris; float k; };
// a float plane, step in bytes
struct GfttPlane { float *data; long long step; };
struct GfttMask { const unsigned char *data; long long step; };   // data == null: none

// linearRow + linearColumn (row_filter.hpp:55-141, column_filter.hpp:55-141) and cornerHarris_kernel / cornerMinEigenVal_kernel
// (corners.cu:62-131,164-240) in one launch; wgmax[tile]: the maximum of the tile's responses
int response_fused(const GfttLaunch &k, const GfttResponsePlan &p, const GfttImage &im, const GfttCorner &c, const GfttPlane &dst, float *wgmax,
                   hipStream_t st);
// the same in two: Dx / Dy planes (dense, cols floats a row), then the windows
int response_deriv(const GfttLaunch &k, const GfttImage &im, const GfttCorner &c, float *dx, float *dy, hipStream_t st);
int response_window(const GfttLaunch &k, const GfttResponsePlan &p, const GfttCorner &c, const float *dx, const float *dy, const GfttPlane &dst,
                    float *wgmax, hipStream_t st);
// cuda::minMax's maximum and gftt.cpp:124's threshold: ctl[GFTT_CTL_THRESHOLD] = (float)((double)max * quality)
int threshold(const GfttLaunch &k, const float *wgmax, int n, double quality, int *ctl, hipStream_t st);
// findCorners' test (gftt.cu:55-88) as one ballot per segment; thr_dev (null: thr_host) is the device's threshold
int find(const GfttLaunch &k, const GfttPlane &resp, int rows, int cols, const GfttMask &mask, const int *thr_dev, float thr_host,
         unsigned long long *masks, int segs_x, int nseg, int *bcount, hipStream_t st);
// bases of the FIND workgroups, the total, the cut at capacity and the sort's padded size into ctl
int scan(const GfttLaunch &k, const int *bcount, int *bbase, int nfind, int capacity, int *ctl, hipStream_t st);
// the first `capacity` candidates in row-major order: keys (null: not wanted) and / or float2 {x, y} points (null: not wanted)
int emit(const GfttLaunch &k, const GfttPlane &resp, int cols, const unsigned long long *masks, int segs_x, int nseg, const int *bbase,
         int capacity, unsigned long long *keys, float *pts, hipStream_t st);
// keys of n float2 points (mi_gftt_sort); sets the count and the padded size in ctl
int make_keys(const GfttPlane &resp, int cols, const float *pts, int n, unsigned long long *keys, int *ctl, hipStream_t st);
// one launch of the sort's list (sortCorners_gpu, gftt.cu:124-136)
int sort_step(const GfttLaunch &k, unsigned long long *keys, const int *ctl, hipStream_t st);
// the first min(limit > 0 ? limit : all, count) keys as float2 {x, y}; the number into ctl[GFTT_CTL_NOUT]
int points(const GfttLaunch &k, const unsigned long long *keys, int cols, int limit, float *out, int *ctl, hipStream_t st);

}  // namespace gftt
}  // namespace mi
