// Hardware self-test hooks: NOT part of the public C-ABI (include/miflow/c_api.h does not declare them).  They run the
// cross-lane primitives the kernels rely on (DPP wave shifts / scans / reductions, ballot tie-break) on known inputs so
// that tests/ can check their semantics on the real device.  Exported under their own prefix for the ctypes tests only.
#pragma once
#include "miflow/c_api.h"

#ifdef __cplusplus
extern "C" {
#endif
/* out_host[0..63] = wave-wide min of in_host[0..63] as seen by every lane, out_host[64] = lane picked by the reference's
 * tie-break rule among the minima (StereoBM winner-take-all) */
MI_API int miflow_selftest_wave_min(const unsigned *in_host, unsigned *out_host /*[65]*/);
/* in_host[k*64 + lane] = value k of lane `lane` (k < 16); out_host[lane] = max over all lanes of value (lane & 15) */
MI_API int miflow_selftest_tmax16(const unsigned *in_host /*[1024]*/, unsigned *out_host /*[64]*/);
/* out_host[i] = inclusive prefix sum of in_host[0..i] over the 64 lanes (DPP scan of the SURF integral) */
MI_API int miflow_selftest_wave_scan(const unsigned *in_host, unsigned *out_host /*[64]*/);
/* the three libm calls of the SURF orientation and descriptor kernels on n <= 2^22 host values: atan2_host[i] = atan2f(a_host[i],
 * b_host[i]) as k_orientation compiles it, (sin_host[i], cos_host[i]) = sincos_rounded(a_host[i]) (csrc/surf_kernels.hip) */
MI_API int miflow_selftest_surf_libm(const float *a_host, const float *b_host, int n, float *atan2_host, float *sin_host, float *cos_host);
/* out_host[0..63] = value received from lane n-1, out_host[64..127] = from lane n+1 when every lane n contributes n+100
 * (DPP wave shifts of the blocked TV-L1 kernels) */
MI_API int miflow_selftest_lane_shift(int *out_host /*[128]*/);
/* Control slots of pair `pair` of the last convergence-checked calc: per launch 8 ints {scale, warp, S.x, S.y, X.x, X.y, X.z,
 * X.w} (tvl1_dev.h); returns the launch count or a negative status.  Used by tools/spec_trace.py to inspect the decisions of the
 * speculative steps; synchronises `stream`. */
/* *fault = 1 if a wave of a joined-wave blocked iteration kernel ever gave up waiting for its neighbour (never expected: the
 * results of that launch are invalid); synchronises the device */
MI_API int miflow_selftest_jw_fault(int *fault);
/* the RCCL binding of mi_tvl1_multi on one device: out_host = in_host after a grouped ncclSend / ncclRecv to self; *available = 0
 * (and nothing copied) where librccl is absent */
MI_API int miflow_selftest_rccl_self_copy(const unsigned char *in_host, unsigned char *out_host, size_t bytes, int *available);
/* fills the handle's whole scratch arena (every plane of every pair slot it was sized for) with NaNs on `stream`: a calc that reads a
 * plane it has not written first -- e.g. the coarsest level's flow, which is never cleared (zero_flow, csrc/fb_plan.h) -- then shows it.
 * MI_ERR_BAD_ARG before the handle's first calc (no arena yet). */
struct mi_farneback;
MI_API int miflow_selftest_farneback_poison(struct mi_farneback *h, void *stream);
/* the same for a BTV-L1 handle: every scratch plane of its arena (frames, motions, maps, both estimates, the sign field) */
/* ONE named launch form of a Farneback stage on the caller's planes (staged into dense planes exactly as the mi_farneback_* stage
 * entries of c_api.h stage them), where the level loop would pick the form from the grid size and the process-wide tuning: one test
 * process holds every form to the oracle and to the other forms.  A form that has no kernel for the request (two iterations per launch
 * at winSize 21, the tiled blur at half size 5, ...) returns MI_ERR_BAD_ARG and launches nothing.  All synchronise `stream`.
 *   iterate: M5out arrives holding a pattern of the caller's (update == 0 must leave it alone); PAIR runs two iterations (the first always
 *     updates; `update` is the second's) and needs M5 != M5out; `merged` (NULL, or a pitched CV_32FC2 matrix, 8-byte aligned) is written
 *     in place by the tiled and the two-iteration kernels, as the last iteration of a single-pair calc writes the caller's flow.
 *   poly_exp: RESIZED takes `src` of ANOTHER size (the blurred full-size frame); the expansion samples its cuda::resize to dst5's size.
 *   update_matrices: PLAIN reads flowx / flowy; ZERO takes them as NULL (the coarsest level's start); RESIZED reads prevx / prevy of
 *     another size and WRITES flowx / flowy = resize(prev) * alpha beside M5.
 *   gaussian_blur: src1 / dst1 only with TABLE, which blurs both (pitched CV_8UC1 or CV_32FC1, read in place; REFLECT101). */
enum { MI_FB_ITER_ROW = 1, MI_FB_ITER_TILE256 = 2, MI_FB_ITER_TILE64 = 3, MI_FB_ITER_PAIR = 4 };
enum { MI_FB_POLY_ROW = 1, MI_FB_POLY_TILED = 2, MI_FB_POLY_RESIZED = 3 };
enum { MI_FB_UM_PLAIN = 1, MI_FB_UM_ZERO = 2, MI_FB_UM_RESIZED = 3 };
enum { MI_FB_BLUR_GENERIC_FAST = 1, MI_FB_BLUR_GENERIC_FULL = 2, MI_FB_BLUR_TILED = 3, MI_FB_BLUR_TABLE = 4 };
MI_API int miflow_selftest_farneback_iterate(int form, const mi_mat *M5, const mi_mat *R0, const mi_mat *R1, mi_mat *flowx, mi_mat *flowy,
                                             mi_mat *M5out, mi_mat *merged, int ksize, int gaussian, int update, void *stream);
MI_API int miflow_selftest_farneback_poly_exp(int form, const mi_mat *src, mi_mat *dst5, int poly_n, double poly_sigma, void *stream);
MI_API int miflow_selftest_farneback_update_matrices(int form, const mi_mat *prevx, const mi_mat *prevy, float alpha, mi_mat *flowx, mi_mat *flowy,
                                                     const mi_mat *R0, const mi_mat *R1, mi_mat *M5, void *stream);
MI_API int miflow_selftest_farneback_gaussian_blur(int form, const mi_mat *src0, const mi_mat *src1, mi_mat *dst0, mi_mat *dst1, int ksize,
                                                   double sigma, int border, void *stream);
struct mi_btvl1;
MI_API int miflow_selftest_btvl1_poison(struct mi_btvl1 *h, void *stream);
struct mi_tvl1;
MI_API int miflow_selftest_tvl1_slots(struct mi_tvl1 *h, int pair, int *out_host, int cap_launches, void *stream);
#ifdef __cplusplus
}
#endif
