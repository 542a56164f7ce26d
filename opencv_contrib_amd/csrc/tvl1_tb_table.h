// The streaming blocked kernels (k_iterate_tbr, tvl1_tbr_kernels.hip): ONE table of the forms a build contains and the constexpr facts
// that follow from a row -- waves, LDS layout and size, strips.  No HIP types: the kernel file instantiates and launches exactly these
// rows, the plan (tvl1_plan.h tb_select) picks among them, tests/cpp/tvl1_plan_test.cpp compiles both alone.
#pragma once
#include <cstddef>

namespace mi {
namespace tvl1 {

// MODE: 0 = fixed work (fast math), 1 = speculative steps of the convergence-checked path, 2 = exact-math blocks.
// WPS = occupancy the register allocator is held to (launch bound); PLAN = waves/SIMD the band planner assumes (r01s: the T10 kernel is
// resident 4 waves/SIMD but fastest when the grid is cut for 3, 394 vs 340 G px-iter/s).  JW: 0 = independent waves (a workgroup = four
// consecutive bands of a 64-column strip), 1 / 2 / 3 / 4 = joined waves (one band of a 256- or 512-column strip; hand-over by tags / one
// barrier per stage / eight waves / branch-free publishes).  NG: no |grad|^2 plane (the pass forms it from I1wx, I1wy).  P16: p as
// snorm16 between passes (changes results).  FW: the warp inside the pass (1: the CPU class's arithmetic, tap-by-tap sums; 2: cv::cuda's,
// separable sums).  GAM: the illumination channel (gamma != 0), always NG.
struct TbRow {
    int MODE, T, PPL, WPS, PF, PLAN, JW;
    bool NG = false, P16 = false;
    int FW = 0;
    bool GAM = false;
};

// Ship what is used: the release library holds the kernels a release build can reach.  The forms that lost their
// A/B exist under -DMIFLOW_EXPERIMENTS only (libmiflow_exp.so), where the digest tests of their bit-identity run.  Within one
// (MODE, T, JW, NG, GAM) the FIRST row is the default, later ones are alternatives (MIFLOW_TB_VARIANT=ppl,wps,pf).
inline constexpr TbRow kTbRows[] = {
    // {MODE, T, PPL, WPS, PF, PLAN, JW, NG, P16, FW, GAM}
    // fixed work, joined waves, T = 10.  Barrier form (MIFLOW_TB_JW=2, the default): no read-ahead registers, no dump area: four
    // waves/SIMD and four workgroups/CU; the same without a |grad|^2 plane (where every pass of a warp is this kernel)
    {0, 10, 1, 4, 2, 3, 2},
    {0, 10, 1, 4, 2, 3, 2, true},
#ifdef MIFLOW_EXPERIMENTS
    {0, 10, 1, 3, 2, 3, 1},   // tags: the hand-over registers cost 14 VGPRs (3 waves/SIMD), 40.7 KB of LDS = 3 workgroups per CU
    {0, 10, 1, 4, 2, 3, 3},   // eight joined waves (MIFLOW_TB_JW=3): two workgroups of eight waves per CU
    {0, 10, 1, 4, 2, 3, 4},   // no exec-masked publishes, no border masks in interior blocks (MIFLOW_TB_JW=4)
    {0, 10, 1, 4, 2, 3, 2, true, true},     // MIFLOW_TB_P16
    // the warp inside (four producer waves beside the four joined consumers; two workgroups of eight waves per CU, i.e. two CONSUMER
    // waves per SIMD is what the band planner fills)
    {0, 10, 1, 4, 2, 2, 2, true, false, 1},
    {0, 10, 1, 4, 2, 2, 2, true, false, 2},
#endif
    // fixed work, independent waves (r01s sweep, G px-iter/s at 1080p x 16: T10 394 | T8 353 | T6 271 | T5 256 | T4 215 | T3 152 | T2 106 | T1 64)
    {0, 10, 1, 4, 2, 3, 0},
    {0, 8, 2, 2, 2, 2, 0},
    {0, 6, 1, 5, 2, 3, 0},
    {0, 5, 2, 3, 2, 3, 0},
    {0, 4, 2, 3, 2, 3, 0},
    {0, 3, 1, 7, 2, 6, 0},
    {0, 2, 1, 8, 2, 8, 0},
    {0, 1, 1, 8, 2, 8, 0},
#ifdef MIFLOW_EXPERIMENTS
    {0, 10, 2, 2, 2, 2, 0},   // alternatives (tuning sweeps, MIFLOW_TB_VARIANT)
    {0, 8, 1, 4, 2, 2, 0},
    {0, 6, 2, 3, 2, 3, 0},
#endif
    // gamma != 0 (round 6): nine dynamic registers per set.  Blocks of 10 and 5 as joined waves, 2 and 1 as
    // independent waves (any iteration count decomposes greedily: tb_plan_level).  T = 10 with ONE prefetched row: 163 VGPRs = three
    // waves/SIMD without scratch; with two it is 168 + 12 spilled dwords
    {0, 10, 1, 3, 1, 3, 2, true, false, 0, true},
    {0, 5, 1, 4, 2, 3, 2, true, false, 0, true},
    {0, 2, 1, 6, 2, 6, 0, true, false, 0, true},
    {0, 1, 1, 8, 2, 8, 0, true, false, 0, true},
    // The speculative steps (T accumulator registers more, hence one wave/SIMD less than MODE 0 at T = 10).  PLAN = 2: the bands are cut
    // for two waves per SIMD -- fewer, taller bands (less halo) than the fixed-work kernels use; the other lane's kernels fill the rest of
    // the device (r02m at 1080p x 16, class defaults: 517 -> 545 pairs/s; fixed work loses 7 %).  Without a |grad|^2 plane (round 4: the
    // convergence-checked path re-reads the statics once per block); a release build runs these where a plane is stored, too
    {1, 10, 1, 3, 2, 2, 2, true},
    {1, 5, 1, 4, 2, 2, 2, true},
#ifdef MIFLOW_EXPERIMENTS
    {1, 10, 1, 3, 2, 2, 0},   // reading the plane: independent waves ...
    {1, 5, 1, 4, 2, 2, 0},
    {1, 10, 1, 3, 2, 2, 2},   // ... and joined ones (MIFLOW_TB_JW >= 2 and MIFLOW_TB_JW_SPEC=1)
    {1, 5, 1, 4, 2, 2, 2},
#endif
    {1, 10, 1, 2, 2, 2, 2, true, false, 0, true},
    {1, 5, 1, 3, 2, 2, 2, true, false, 0, true},
    // Exact-math blocks (1 px per lane).  The stage costs about four times the fast one (three IEEE divisions, two double square
    // roots), so short blocks already move the kernel from the HBM bound of the one-iteration kernel to the issue bound.  r02y at
    // 1080p x 16, N = 10: blocks of 2 | 3 | 5 | 10 = 345 | 423 | 532 | 451 pairs/s (one launch per iteration: 228)
    {2, 5, 1, 4, 2, 3, 0},
    {2, 4, 1, 4, 2, 3, 0},
    {2, 3, 1, 5, 2, 4, 0},
    {2, 2, 1, 6, 2, 4, 0},
    {2, 1, 1, 8, 2, 4, 0},
};
constexpr int kTbRowCount = (int)(sizeof(kTbRows) / sizeof(kTbRows[0]));

// ---- LDS layout (the kernel file describes what lives where) ------------------------------------------------------------------------
// waves of a workgroup: four (independent waves: four bands of a strip; JW = 1, 2, 4: a 256-column strip); JW = 3: eight (512 columns:
// 492 owned instead of 2 x 236), barrier form
constexpr int jw_waves(int JW) { return JW == 3 ? 8 : 4; }
constexpr bool jw_fast(int JW) { return JW == 4; }
// ring slots of the static planes per wave: the row of step n is read by stages 2..T-1 at steps n+2..n+T-1
constexpr int tb_ring_slots(int T) { return T > 2 ? T - 1 : 1; }
// JW = 1: hand-over slots of 32 bytes {p11, p21 | u1, u2 | tag | pad}, an area of 2 buffers x T slots per wave and a dump of the same
// size + 8 bytes per lane where the 63 non-publishing lanes write
constexpr int XS = 32;
constexpr int xarea_bytes(int T) { return 2 * T * XS; }
constexpr int xdump_bytes(int T) { return 2 * T * XS + 64 * 8; }
// JW >= 2: slots of 16 bytes {p11, p21, u1, u2}; GAM: 32 bytes {p11, p21, u1, u2 | p31, u3, -, -}
constexpr int XS2 = 16;
constexpr int xs2_bytes(bool gam) { return gam ? 32 : XS2; }
constexpr int xarea2_bytes(int T, bool gam = false) { return 2 * T * xs2_bytes(gam); }
constexpr int xdump4_bytes(int T) { return 64 * 8 + 2 * xarea2_bytes(T) + 64; }   // JW = 4: per workgroup, shared by its waves
// FW: inboxes of FW_RING rows per consumer wave + the cubic phase table; FW_STAGE = 1: a private band of I1 per producer wave as well
constexpr int FW_RING = 4;         // inbox slots (rows) per consumer wave: two rows of lead + the two steps of consumer skew
constexpr int FW_SLOT = 3 * 64;    // floats per slot
constexpr int fw_lds_floats(int NW) { return NW * FW_RING * FW_SLOT + 128; }
#ifndef FW_STAGE
#define FW_STAGE 0   // 0 (default): the producers gather their windows (fw_produce); 1: they read them from a private LDS band of I1 (fw_produce_staged) -- bit-identical, measured no faster (r14g, r14h: 1 093 - 1 180 against 1 205 pairs/s): the fused form is bound by VALU issue, not by the gathers
#endif
constexpr int FWS_D1 = 5, FWS_D2 = 8;
constexpr int FWS_CW = 64 + 2 * FWS_D1 + 6;    // 80 columns (with 88 the workgroup needs exactly 80 KB of LDS and only one fits a CU)
constexpr int FWS_NR = 2 * FWS_D2 + 6;         // 22 rows: the six window rows of every flow within +- FWS_D2 of the band's mean
constexpr int fws_lds_floats(int NW) { return NW * FWS_NR * FWS_CW; }

// dynamic LDS of a workgroup: the rings, the hand-over areas (and dumps), the fused warp's inboxes
constexpr size_t tb_lds_bytes(const TbRow &r)
{
    const int NW = jw_waves(r.JW);
    return (size_t)NW * tb_ring_slots(r.T) * 256 * r.PPL * sizeof(float) +
           (r.JW >= 2 ? NW * xarea2_bytes(r.T, r.GAM) + (jw_fast(r.JW) ? xdump4_bytes(r.T) : 0) : r.JW ? 4 * (xarea_bytes(r.T) + xdump_bytes(r.T)) : 0) +
           (r.FW ? (fw_lds_floats(NW) + (FW_STAGE ? fws_lds_floats(NW) : 0)) * sizeof(float) : 0);
}
// waves per SIMD the band planner fills: the row's PLAN, or what the LDS of a CU (160 KB) holds in units of four-wave workgroups
constexpr int tb_plan_wps(const TbRow &r)
{
    const int lds_wps = (int)((160 * 1024) / tb_lds_bytes(r)) * jw_waves(r.JW) / 4;
    return r.PLAN < lds_wps ? r.PLAN : lds_wps;
}
// strips of a level w pixels wide: a strip covers LW pixels (a wave, or the joined waves of a workgroup) with a validity margin of M
// on each side; strip 0 starts at the image border and owns LW - M columns, the others LW - 2 M
constexpr int tb_strips(const TbRow &r, int w)
{
    const int M = (r.T + r.PPL - 1) / r.PPL * r.PPL, LW = (r.JW ? 64 * jw_waves(r.JW) : 64) * r.PPL;
    return w <= LW - M ? 1 : 1 + (w - (LW - M) + (LW - 2 * M) - 1) / (LW - 2 * M);
}
// The kernels that can store the flow interleaved into the callers' matrices (TbArgs::otab): fixed work, one pixel per lane, and not the
// joined waves that read a |grad|^2 plane -- that kernel sits at exactly 128 VGPRs and no calc's final pass runs on it
constexpr bool tb_il_form(int PPL, int JW, bool NG) { return PPL == 1 && (NG || JW == 0); }
constexpr bool tb_il_form(const TbRow &r) { return r.MODE == 0 && !r.GAM && tb_il_form(r.PPL, r.JW, r.NG); }

}  // namespace tvl1
}  // namespace mi
