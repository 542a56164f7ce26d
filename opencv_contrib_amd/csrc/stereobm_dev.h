// Internal launch API of the StereoBM HIP kernels (stereobm_kernels.hip).  Not part of the C-ABI.
#pragma once
#include <cstdlib>
#include "mi_common.h"
#include "sbm_plan.h"

namespace mi {
namespace sbm {

// SSD block matching + winner-take-all (+ the uniqueness verification pass when the plan says so), as sbm_make_plan planned it.
// The images: one pair by its pointers, or (tab != null) the plan's `pairs` pairs of one size from a device table in ONE launch
// (blockIdx.z = pair): the batch supplies the parallelism, so the row bands are taller and the 2R-row start-up of a band weighs less.
// disp: zero-filled by the caller (stereobm.cu:506); minssd (rows x mstep uint32, pairs mpair elements apart): required when the plan verifies.
struct BmPair { const unsigned char *left, *right; unsigned char *disp; long long lstep, rstep, dstep; };
struct BmImages { BmPair one; const BmPair *tab; unsigned *minssd; long long mstep, mpair; int emulate_edge; };
int block_match(const BmImages &images, const BmPlan &plan, hipStream_t s);
inline BmSwitches bm_switches() { const char *e = MI_EXP_ENV("MIFLOW_SBM_ROWS"); return {tuning().sbm_wt, tuning().sbm_swz, e ? atoi(e) : 0}; }
// a validator's verdict as this library reports errors
inline int sbm_fail(const SbmErr &e) { MI_REQUIRE(e.code == MI_OK, e.code, "%s", e.msg); return MI_OK; }
int prefilter_xsobel(const unsigned char *src, long long sstep, unsigned char *dst, long long dstep, int rows, int cols,
                     int cap, hipStream_t s);
int prefilter_norm(const unsigned char *src, long long sstep, unsigned char *dst, long long dstep, int rows, int cols,
                   int cap, int winsize, hipStream_t s);
int zero_disp_batch(const BmPair *tab_dev, int pairs, int rows, int cols, hipStream_t s);   // disp := 0 of every pair, one launch
int textureness_fused(const unsigned char *img, long long istep, unsigned char *disp, long long dstep, const BmPair *tab_dev, int pairs,
                      int rows, int cols, int winsz, float avg_threshold, hipStream_t s);   // one launch, no scratch plane; bit-identical
int textureness(const unsigned char *img, long long istep, unsigned char *disp, long long dstep, int rows, int cols,
                int winsz, float avg_threshold, int *S, hipStream_t s);   // S: int scratch of textureness_scratch_dims() = sld x sh elements
int dbg_wave_min(const unsigned *in_dev, unsigned *out_dev, hipStream_t s);
int dbg_tmax16(const unsigned *in_dev /*[16][64]*/, unsigned *out_dev /*[64]*/, hipStream_t s);

}  // namespace sbm
}  // namespace mi
