// Internal launch API of the FastFeatureDetector HIP kernels (fast_kernels.hip).  Not part of the C-ABI.
// Geometry (tiles, segments, pitches, grids) is the plan's (fast_plan.h); these functions launch exactly one kernel each.
#pragma once
#include "mi_common.h"
#include "fast_plan.h"

namespace mi {
namespace fast {

inline int fast_fail(const FastErr &e) { MI_REQUIRE(e.code == MI_OK, e.code, "%s", e.msg); return MI_OK; }

// the caller's image and mask (mask == null: none); steps in bytes, any base address, any step >= cols
struct FastImage { const unsigned char *data; long long step; const unsigned char *mask; long long mstep; int rows, cols; };
// the frame area of the scratch
struct FastScratch { unsigned char *plane; unsigned long long *cand, *surv, *emit; int *pos; int *counts; };

// calcKeypoints<true>, fast.cu:211-275, without its atomics: plane[y * pitch + x] = 0 or score + 1, cand[y * segs_x + x / 64] = the
// ballot of the segment's candidates
int score(const FastLaunch &k, const FastFrame &f, const FastImage &im, int threshold, const FastScratch &s, hipStream_t st);
// nonmaxSuppression's test, fast.cu:318-346, for every candidate: surv = the candidates that beat their eight neighbours
int nms(const FastLaunch &k, const FastFrame &f, const FastScratch &s, hipStream_t st);
// ranks, the cut at max_npoints, output positions; counts[0] = candidates, counts[1] = emitted.  surv == cand without suppression
int scan(const FastLaunch &k, const FastFrame &f, const FastScratch &s, bool use_nms, int max_npoints, hipStream_t st);
// short2 {x, y} into loc[], float(score) or 0 into resp[], row-major
int emit(const FastLaunch &k, const FastFrame &f, const FastScratch &s, bool use_nms, void *loc, float *resp, hipStream_t st);
// the reference's CV_32SC1 plane from the byte plane: score where a candidate, 0 elsewhere; ostep in bytes
int plane_to_scores(const FastFrame &f, const unsigned char *plane, int *scores, long long ostep, hipStream_t st);
// short2 locations -> float2 points
int locations_to_points(const void *loc, int n, float *points, hipStream_t st);

}  // namespace fast
}  // namespace mi
