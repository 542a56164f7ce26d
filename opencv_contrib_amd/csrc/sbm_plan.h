// The PLAN of StereoBM's launches (stereobm_kernels.hip): the tile geometry of a radius, the LDS layout of k_block_match and of
// k_textureness_fused (the KERNEL takes its pointers and the LAUNCHER its dynamic-LDS size from the same code), the band rule, the one
// validator, what a block-matching call launches (block_match() and launch_bm<R> only EXECUTE it).  Pure arithmetic, no HIP types.
#pragma once
#include <cstddef>
#include <utility>
#include "miflow/c_api.h"

#if defined(__HIPCC__)
#define MI_SBM_HD __host__ __device__
#else
#define MI_SBM_HD
#endif

namespace mi {
namespace sbm {

MI_SBM_HD constexpr int sbm_div_up(int a, int b) { return (a + b - 1) / b; }

// Tile width of the unpacked kernels (R >= 13) -- and, for EVERY radius, the width the band rule (bm_band_rows) counts tiles with:
// the rule was tuned before the packed kernels (R <= 12) took 48 columns, so it differs from the kernel's tile for R 1..6 and 9..12
// (60 60 56 56 52 52 | 44 44 40 40) and equals it for R 7, 8 and R >= 13.  Left alone: rb changes speed (open question).
MI_SBM_HD constexpr int bm_legacy_w(int R) { const int t = (64 - 2 * R) & ~3; return t < 16 ? 16 : t; }

template <int R>
struct Cfg {
    // R <= 12: max SSD (2R+1)^2 * 255^2 < 2^26, so (2^26-1 - SSD) << 6 | tie-break key fits one u32 and the winner is a
    // single max-reduction, done 16 columns at a time (tile width 48 = 3 groups); larger windows: generic path
    static constexpr bool PACKED = R <= 12;
    static constexpr int TW = PACKED ? 48 : bm_legacy_w(R);   // output columns per tile
    static constexpr int NC = TW + 2 * R;            // column sums per lane
    static constexpr int LS = (NC + 15) / 16 * 16;   // LDS bytes per staged left row
    static constexpr int NLW = LS / 4;               // dwords per left row
    static constexpr int NRW = (NC + 3) / 4 + 1;     // aligned dwords a lane reads per right row
};
MI_SBM_HD constexpr bool bm_packed(int R) { return R <= 12; }
MI_SBM_HD constexpr int bm_tile_w(int R) { return bm_packed(R) ? 48 : bm_legacy_w(R); }   // = Cfg<R>::TW for a runtime R

// Dynamic LDS of k_block_match for bands of rb rows.  Three regions one behind the other from offset 0, each by its SIZE in bytes
// (the kernel chains its pointers): rb + 2R staged rows of the left image (LS bytes each), as many of the right (RS each),
// comb[2][nsets][2][64] dwords.  Then, at byte OFFSET tbuf() = the next 16-byte boundary (b128 reads), for wt -- the LDS-transposed
// winner-take-all -- one [16][BM_TP] dword buffer per wave (16 * 68 dwords = 4.3 KB).  bytes(): all of it; = tbuf() without wt.
// Radius: int on the host; the kernel passes its template argument as a type (std::integral_constant) and so compiles to the code it
// had with the expressions written out in it (a runtime R, folded only after inlining, changes its register allocation).
constexpr int BM_TP = 68;   // dwords per row of the transposition buffer
template <class Radius = int>
struct BmLdsT {
    Radius R; int nsets, rb; bool wt;
    MI_SBM_HD constexpr int NC() const { return bm_tile_w(R) + 2 * R; }
    MI_SBM_HD constexpr int LS() const { return (NC() + 15) / 16 * 16; }
    MI_SBM_HD constexpr int RS() const { return (NC() + nsets * 64 - 1 + 3) / 4 * 4 + 4; }   // the lanes' disparities reach nsets * 64 - 1 columns to the left
    MI_SBM_HD constexpr size_t srows() const { return (size_t)(rb + 2 * R); }   // staged rows of each image
    MI_SBM_HD constexpr size_t left() const { return srows() * LS(); }
    MI_SBM_HD constexpr size_t right() const { return srows() * RS(); }
    MI_SBM_HD constexpr size_t comb() const { return (size_t)2 * nsets * 128 * sizeof(unsigned); }
    MI_SBM_HD constexpr size_t tbuf() const { return (left() + right() + comb() + 15) / 16 * 16; }
    MI_SBM_HD constexpr size_t tstride() const { return (size_t)16 * BM_TP * sizeof(unsigned); }   // per wave
    MI_SBM_HD constexpr size_t bytes() const { return tbuf() + (wt ? nsets * tstride() : 0); }
};
typedef BmLdsT<int> BmLds;
MI_SBM_HD constexpr BmLds bm_lds(int R, int nsets, int rb, bool wt) { return {R, nsets, rb, wt}; }
template <int... R>   // the runtime twins against Cfg<R>, R = 1..25
constexpr bool bm_twins_agree(std::integer_sequence<int, R...>) { return (... && (bm_tile_w(R + 1) == Cfg<R + 1>::TW && bm_packed(R + 1) == Cfg<R + 1>::PACKED && bm_lds(R + 1, 1, 1, false).LS() == Cfg<R + 1>::LS)); }
static_assert(bm_twins_agree(std::make_integer_sequence<int, 25>{}), "bm_tile_w / bm_lds disagree with Cfg<R>");

// Textureness post-filter: the extended domain of the two-pass form's |Sobel| plane; the tile of the fused form and its LDS, one behind
// the other: B (BR x BC) and S (TRR x TC, padded to a dword) by their sizes in u16 WORDS, then 128 ints of column sums per wave.
constexpr int TEX_MX = 32, TEX_MY = 26, TEXF_ROWS = 32;
inline void textureness_scratch_dims(int rows, int cols, int *sld, int *sh) { *sld = sbm_div_up(cols, 64) * 64 + 2 * TEX_MX; *sh = rows + 2 * TEX_MY; }
struct TexfLds { int TC, TRR, BC, BR, B, S; size_t bytes; };
MI_SBM_HD constexpr TexfLds texf_lds(int W2)
{
    const int TC = 64 + 2 * W2, TRR = TEXF_ROWS + 2 * W2, BC = TC + 2, BR = TRR + 2, B = BR * BC, S = (TRR * TC + 1) & ~1;
    return {TC, TRR, BC, BR, B, S, sizeof(unsigned short) * ((size_t)B + S) + sizeof(int) * 4 * 128};
}

// Rows per band: enough waves for the 1024 SIMDs (target ~5 per SIMD) but keep the 2R-row start-up of every band (column sums of the
// first window) a modest fraction of the work.  A batch supplies the waves, so its bands can be taller.
inline int bm_band_rows(int rows, int cols, int ndisp, int R, int pairs)
{
    const int xt = sbm_div_up(cols - ndisp - 2 * R, bm_legacy_w(R));
    const int bands = sbm_div_up(5120, xt * sbm_div_up(ndisp, 64) * pairs);   // r01f sweep: ~16 rows per band is the optimum for ONE 1080p / 128-disparity pair
    int rb = sbm_div_up(rows - 2 * R, bands > 0 ? bands : 1);
    rb = rb < 2 * R + 2 ? 2 * R + 2 : rb;
    return rb > 48 ? 48 : rb;   // taller bands cost occupancy (LDS per workgroup grows with rb): r02w at 1080p x 16: 32 | 48 | 64 | 96 rows = 4990 | 5070 | . | 4575 pairs/s
}

// THE validator.  rmin: the block matcher needs R >= 1, the textureness filter on its own also takes a 1 x 1 window.
struct SbmErr { int code; const char *msg; };
inline SbmErr sbm_check_window(int winsz, int rmin)
{
    if (winsz % 2 != 1) return {MI_ERR_BAD_ARG, "blockSize must be odd"};   // CV_Assert( winSize_ % 2 == 1 )  stereobm.cpp:146
    if ((winsz >> 1) < rmin || (winsz >> 1) > 25) return {MI_ERR_BAD_ARG, "Unsupported window size"};   // stereobm.cu:503-504
    return {MI_OK, nullptr};
}
inline SbmErr sbm_check(int ndisp, int winsz, int rows, int cols)
{
    if (!(0 < ndisp && ndisp <= 256)) return {MI_ERR_BAD_ARG, "numDisparities must be in (0,256]"};   // CV_Assert( 0 < ndisp_ && ndisp_ <= 256 )  stereobm.cpp:143
    if (ndisp % 8 != 0) return {MI_ERR_BAD_ARG, "numDisparities must be a multiple of 8"};              // CV_Assert( ndisp_ % 8 == 0 )  :145
    if (const SbmErr e = sbm_check_window(winsz, 1); e.code) return e;
    // the reference launches an empty grid here (stereobm.cu:469-470), which the CUDA runtime rejects
    if (!(cols - ndisp - 2 * (winsz >> 1) > 0 && rows - 2 * (winsz >> 1) > 0)) return {MI_ERR_BAD_SIZE, "image too small for numDisparities + blockSize"};
    return {MI_OK, nullptr};
}

struct BmSwitches { int wt, swz, rows; };   // MIFLOW_SBM_WT, MIFLOW_SBM_SWZ; MIFLOW_SBM_ROWS (experiments build; <= 0: the band rule)
struct BmPlan {
    SbmErr err;           // sbm_check's verdict; nothing below is set when it rejects
    int rows, cols, ndisp, R, nsets, rb, swz;
    int grid[3], block;   // tiles x bands x pairs workgroups of one wave per 64 disparities
    bool wt;              // first pass (MODE 0): k_block_match<R, 0, true> (transposed winner-take-all) or the plain <R, 0>
    bool verify;          // ... followed by the uniqueness pass <R, 1>
    size_t lds_first, lds_verify;   // dynamic LDS bytes of the two launches
    float thresh_scale;   // (float)(1.0 + uniquenessRatio / 100.0f)  stereobm.cu:273
};
inline BmPlan sbm_make_plan(int rows, int cols, int ndisp, int winsz, int uniqueness_ratio, int pairs, const BmSwitches &sw)
{
    BmPlan p = {};
    if ((p.err = sbm_check(ndisp, winsz, rows, cols)).code) return p;
    const int R = winsz >> 1;
    p.rows = rows; p.cols = cols; p.ndisp = ndisp; p.R = R; p.nsets = sbm_div_up(ndisp, 64);
    p.rb = sw.rows > 0 ? sw.rows : bm_band_rows(rows, cols, ndisp, R, pairs);
    p.swz = sw.swz != 0 ? 1 : 0;
    p.grid[0] = sbm_div_up(cols - ndisp - 2 * R, bm_tile_w(R)); p.grid[1] = sbm_div_up(rows - 2 * R, p.rb); p.grid[2] = pairs;
    p.block = 64 * p.nsets;
    // one first-pass kernel per radius in the release library: the transposed winner-take-all where the column sums are packed, the
    // plain form elsewhere; the experiments build keeps both for MIFLOW_SBM_WT
#ifdef MIFLOW_EXPERIMENTS
    p.wt = bm_packed(R) && sw.wt;
#else
    p.wt = bm_packed(R);
#endif
    p.verify = uniqueness_ratio > 0;
    p.lds_first = bm_lds(R, p.nsets, p.rb, p.wt).bytes();
    p.lds_verify = bm_lds(R, p.nsets, p.rb, false).bytes();
    p.thresh_scale = (float)(1.0 + uniqueness_ratio / 100.0f);
    return p;
}

}  // namespace sbm
}  // namespace mi
