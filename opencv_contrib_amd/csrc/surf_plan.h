// The PLAN of one SURF detect call (surf_api.cpp): which launch form the detector takes (octave by octave, or every stage once for all
// octaves; octave 0 on LDS tiles; its maxima flagged in the det kernel; octaves >= 1 on polyphase planes), where every octave's
// regions lie in the scratch buffers, how many elements each buffer holds, the grid of every launch and the tap geometry table.  Pure
// host arithmetic over the frame's shape and the switches, no HIP types: tests/cpp/surf_plan_test.cpp compiles it alone.  ensure()
// allocates what a plan says, detect_all (surf_kernels.hip) and the per-octave loop of detect_enqueue only EXECUTE it.
// Reference: SURF_CUDA_Invoker, xfeatures2d/src/surf.cuda.cpp:134-255.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstring>

namespace mi {
namespace surf {

struct SurfShape { int rows, cols, n_octaves, n_octave_layers, max_candidates; };
inline bool operator==(const SurfShape &a, const SurfShape &b)
{
    return a.rows == b.rows && a.cols == b.cols && a.n_octaves == b.n_octaves && a.n_octave_layers == b.n_octave_layers &&
           a.max_candidates == b.max_candidates;
}
struct SurfKnobs {
    bool fused;    // MIFLOW_SURF_FUSED (experiments build): one launch per stage for all octaves where the kernel arguments hold them
    bool lds;      // MIFLOW_SURF_LDS (experiments build): octave 0 of the all-octave det / trace launch on LDS tiles
    bool nms0;     // MIFLOW_SURF_NMS0=1: ... and its maxima flagged inside that kernel (bit-identical, measured slower: an opt-in)
    bool poly;     // MIFLOW_SURF_POLY: octaves >= 1 read their taps from polyphase planes of the integral image
    bool lds_ok;   // lds_geometry_self_check(): the compile-time tap geometry of the LDS tiles is the host's
};

constexpr int surf_div_up(int a, int b) { return (a + b - 1) / b; }
constexpr int surf_align_up(int a, int b) { return surf_div_up(a, b) * b; }
constexpr int calc_size(int octave, int layer) { return (9 + 6 * layer) << octave; }   // surf.cu:161-173

constexpr int kIntBandRows = 32;      // rows of one band of the integral image's column pass
constexpr int kMaxFusedOctaves = 6;
constexpr int kDetLayers = 6;         // layers of one det / trace launch (nOctaveLayers + 2 <= 6; more layers: several launches)
#ifndef MI_SURF_NMS_SEG
#define MI_SURF_NMS_SEG 8
#endif
constexpr int kNmsSeg = MI_SURF_NMS_SEG;   // chunks of one wave: a 4K row is 8 waves (one wave per row left the loop at 60 dependent round trips)
// octave 0 on an LDS tile: 16 x 64 samples per workgroup, patch 43 rows x 92 words (91 used); with the maxima flagged in the kernel the
// tiles overlap by one sample on every side (14 x 62 interior samples)
constexpr int kLdsTX = 64, kLdsTY = 16, kLdsSMax = 27, kLdsPW = 92, kLdsPH = kLdsTY + kLdsSMax;
constexpr int kLdsLayers = 4;
constexpr int kFuseTY = kLdsTY - 2, kFuseTX = kLdsTX - 2;

// ------------------------------------------------------------------ tap geometry
struct HaarGeo {       // per layer: tap offsets (elements, relative to the sample's top-left corner) and 1 / area, area of the 10 boxes
    int xx[4][2];      // Dxx corners [x edge 0..3][y edge 0..1]
    int yy[2][4];      // Dyy corners [x edge 0..1][y edge 0..3]
    int xy[4][4];      // Dxy corners [y edge][x edge]
    double ry[10], area[10];   // boxes: Dxx 0..2, Dyy 3..5, Dxy 6..9
};
// host side (the geometry of a layer does not depend on the sample): rintf = round-half-even = __float2int_rn of the device code
template <class Off>   // off(ey, ex): word offset of the tap (ey rows, ex columns) from the sample's top-left corner
inline HaarGeo haar_geo_off(int size, Off off)
{
    HaarGeo g;
    const float ratio = (float)size / 9;
    const auto rnh = [](float v) { return (int)rintf(v); };
    const int e0369[4] = {rnh(ratio * 0.f), rnh(ratio * 3.f), rnh(ratio * 6.f), rnh(ratio * 9.f)};
    const int e27[2] = {rnh(ratio * 2.f), rnh(ratio * 7.f)};
    const int e1458[4] = {rnh(ratio * 1.f), rnh(ratio * 4.f), rnh(ratio * 5.f), rnh(ratio * 8.f)};
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 2; ++j) { g.xx[i][j] = off(e27[j], e0369[i]); g.yy[j][i] = off(e0369[i], e27[j]); }
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) g.xy[i][j] = off(e1458[i], e1458[j]);
    for (int k = 0; k < 3; ++k) {
        g.area[k] = (double)((e0369[k + 1] - e0369[k]) * (e27[1] - e27[0]));
        g.area[3 + k] = g.area[k];   // Dyy is Dxx transposed: the same edge differences
    }
    g.area[6] = (double)((e1458[1] - e1458[0]) * (e1458[1] - e1458[0]));
    g.area[7] = (double)((e1458[3] - e1458[2]) * (e1458[1] - e1458[0]));
    g.area[8] = g.area[7];
    g.area[9] = (double)((e1458[3] - e1458[2]) * (e1458[3] - e1458[2]));
    for (int k = 0; k < 10; ++k) g.ry[k] = 1.0 / g.area[k];
    return g;
}
inline HaarGeo haar_geo(int size, int sld) { return haar_geo_off(size, [sld](int ey, int ex) { return ey * sld + ex; }); }

// ---- polyphase copies of the integral image for octaves >= 1 (round 5).  A sample of octave o sits at S[(i << o)][(j << o)] and its
// taps at fixed offsets (ey, ex) from there: the 64 lanes of a wave (consecutive j) read words 2^o apart -- 8 .. 32 lines of 64 B per
// load, the L1 tag-lookup rate that bounds the gather path (profiles/surf_counters.json).  With the integral image also stored as 4^o
// PHASE PLANES per octave, plane (y & m, x & m) holding S[y][x] at (y >> o, x >> o), the same tap is
//     plane(ey & m, ex & m)[i + (ey >> o)][j + (ex >> o)]
// i.e. consecutive lanes read CONSECUTIVE words (4-5 lines per load), and the tap is still "lane offset + wave-uniform offset": only the
// geometry table and the lane offset change, the integers read -- and with them every det / trace value -- are the same.
struct PolyGeo { int prows, pld; long long plane_words, base; };   // per octave (octave 0: unused)
inline PolyGeo poly_geo(int rows, int cols, int o, long long base)
{
    PolyGeo g;
    g.prows = (rows >> o) + 2; g.pld = surf_align_up((cols >> o) + 2, 64);
    g.plane_words = (long long)g.prows * g.pld; g.base = base;
    return g;
}
inline long long poly_total_words(int rows, int cols, int n_octaves)
{
    long long w = 0;
    for (int o = 1; o < n_octaves; ++o) w += poly_geo(rows, cols, o, 0).plane_words << (2 * o);
    return w;
}

// ---- octave 0 on an LDS tile: the tap offsets are COMPILE-TIME constants (sizes 9, 15, 21, 27 and the fixed patch stride)
constexpr int lds_rn(float v)   // round to nearest, ties to even (= __float2int_rn / rintf), v >= 0
{
    const int f = (int)v;
    const float r = v - (float)f;
    return r > 0.5f ? f + 1 : (r < 0.5f ? f : ((f & 1) ? f + 1 : f));
}
template <int L>
struct LdsGeo {   // geometry of octave 0, layer L for the patch stride: the compile-time twin of haar_geo(9 + 6 L, kLdsPW)
    static constexpr int size = 9 + 6 * L;
    static constexpr float ratio = (float)size / 9;
    static constexpr int e(int c) { return lds_rn(ratio * (float)c); }
    static constexpr int xx(int i, int j) { return e(j ? 7 : 2) * kLdsPW + e(3 * i); }
    static constexpr int yy(int j, int i) { return e(3 * i) * kLdsPW + e(j ? 7 : 2); }
    static constexpr int xy(int i, int j) { return e(i == 0 ? 1 : i == 1 ? 4 : i == 2 ? 5 : 8) * kLdsPW + e(j == 0 ? 1 : j == 1 ? 4 : j == 2 ? 5 : 8); }
    static constexpr double axx(int k) { return (double)((e(3 * k + 3) - e(3 * k)) * (e(7) - e(2))); }
    static constexpr double a6 = (double)((e(4) - e(1)) * (e(4) - e(1))), a7 = (double)((e(8) - e(5)) * (e(4) - e(1))), a9 = (double)((e(8) - e(5)) * (e(8) - e(5)));
};
// host check that the compile-time geometry is haar_geo's (a knob of the plan; tests/cpp/surf_plan_test.cpp runs it without a device)
template <int L>
inline bool lds_geo_matches()
{
    typedef LdsGeo<L> G;
    const HaarGeo h = haar_geo(G::size, kLdsPW);
    bool ok = true;
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 2; ++j) ok = ok && h.xx[i][j] == G::xx(i, j) && h.yy[j][i] == G::yy(j, i);
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) ok = ok && h.xy[i][j] == G::xy(i, j);
    for (int k = 0; k < 3; ++k) ok = ok && h.area[k] == G::axx(k);
    return ok && h.area[6] == G::a6 && h.area[7] == G::a7 && h.area[9] == G::a9;
}
inline bool lds_geometry_self_check() { return lds_geo_matches<0>() && lds_geo_matches<1>() && lds_geo_matches<2>() && lds_geo_matches<3>(); }

// ------------------------------------------------------------------ all octaves of a frame in one launch per stage (round 3)
// The planes, flag words, counts and candidate lists of an octave live at their own offsets, a workgroup finds its octave from the
// cumulative workgroup counts.  A KERNEL ARGUMENT of the k_*_all kernels: the layout is theirs.
struct OctSet {
    int n;                                   // octaves
    int nlayers;                             // nOctaveLayers
    int rows, cols, dld;
    long long plane0[kMaxFusedOctaves];      // float offset of the octave's first det / trace plane
    long long bits0[kMaxFusedOctaves];       // u64 offset of its flag words
    int row0[kMaxFusedOctaves];              // first (layer, row) index in rowcnt space (rowcnt has one extra entry per octave)
    long long seg0[kMaxFusedOctaves];        // offset of its row-segment counts
    int blk_dt[kMaxFusedOctaves + 1];        // cumulative workgroup counts of k_det_trace_all
    int blk_nms[kMaxFusedOctaves + 1];       //   ... of k_nms_flag_all (row groups x segments)
    int blk_wr[kMaxFusedOctaves + 1];        //   ... of k_nms_write_all (row groups)
    int nbx[kMaxFusedOctaves], nby[kMaxFusedOctaves], nseg[kMaxFusedOctaves], chunks[kMaxFusedOctaves];
    int lds0;                                // octave 0 of k_det_trace_all on LDS tiles (all its layers per workgroup): nby[0] counts 16-row tiles
    int poly;                                // octaves >= 1 read their taps from the polyphase planes (pld / pbase per octave; geometry table built for them)
    int pld[kMaxFusedOctaves];
    long long pbase[kMaxFusedOctaves];
    int fuse0;                               // ... and its maxima flagged in that kernel (no planes; tiles of 14 x 62 interior samples; no k_nms_flag_all workgroups)
};

struct SurfPlan {
    SurfShape shape;
    // launch forms
    bool fused;          // every detector stage once for all octaves (<= kMaxFusedOctaves octaves, nOctaveLayers + 2 <= kDetLayers: every
                         // default), keeping every octave's planes (~4/3 of octave 0's); else octave by octave through one set of planes
    bool lds0;           // fused, and octave 0 of the det / trace launch on LDS tiles (nOctaveLayers + 2 <= kLdsLayers)
    bool fuse0;          // lds0, and octave 0's maxima flagged in its own det kernel (k_det_nms0): no octave-0 planes, sign words instead
    bool poly;           // fused, more than one octave, and octaves >= 1 on the polyphase planes
    int sld, vld, dld;   // row lengths (elements) of the integral image, its column-pass scratch and the det / trace planes
    OctSet S;            // fused only: every octave's offsets and workgroup ranges
    // elements of every scratch buffer
    size_t sum_words, v_words, bt_words;   // integral image (the mask's is as large), column prefixes, band totals
    size_t plane_floats;                   // det and trace, each
    size_t bits_words, sbits_words;        // u64 flag words; sign words of octave 0 (fuse0 only, else 0: not allocated)
    size_t row_counts, seg_counts;
    int cand_lists;                        // candidate lists of shape.max_candidates entries each: one per octave (fused) or one
    size_t cand_items;                     // candidates = interpolation results
    size_t geo_bytes;                      // HaarGeo[n_octaves][kDetLayers] (fused only)
    size_t poly_words;                     // poly only
    // grids of the all-octave launches, in launch order (0: not launched)
    int grid_poly_x, grid_poly_y;          // k_poly_build
    int grid_det0;                         // k_det_nms0 (fuse0: octave 0's workgroups, = S.blk_dt[1])
    int grid_det;                          // k_det_trace_all: the other workgroups
    int grid_nms, grid_scan, grid_write;   // k_nms_flag_all, k_scan_counts_all, k_nms_write_all
    int grid_interp_x, grid_interp_y;      // k_interp_eval_all
    int grid_compact;                      // k_interp_compact_all
};

inline SurfPlan surf_make_plan(const SurfShape &Z, const SurfKnobs &K)
{
    SurfPlan p;
    memset(&p, 0, sizeof(p));
    const int rows = Z.rows, cols = Z.cols, n = Z.n_octaves, L = Z.n_octave_layers;
    p.shape = Z;
    p.fused = K.fused && n <= kMaxFusedOctaves && L + 2 <= kDetLayers;
    p.lds0 = p.fused && K.lds && K.lds_ok && L + 2 <= kLdsLayers;
    p.fuse0 = p.lds0 && K.nms0;
    p.poly = p.fused && K.poly && n > 1;
    p.sld = surf_align_up(cols + 1, 64); p.vld = surf_align_up(cols, 64); p.dld = surf_align_up(cols, 64);
    p.sum_words = (size_t)p.sld * (rows + 1);
    p.v_words = (size_t)p.vld * rows;
    p.bt_words = (size_t)p.vld * surf_div_up(rows, kIntBandRows);
    p.cand_lists = p.fused ? n : 1;
    p.cand_items = (size_t)Z.max_candidates * p.cand_lists;
    if (!p.fused) {   // one octave at a time through regions sized for octave 0
        const int chunks = surf_div_up(cols, 64);
        p.plane_floats = (size_t)p.dld * rows * (L + 2);
        p.bits_words = (size_t)L * rows * chunks;
        p.row_counts = (size_t)L * rows + 1;
        p.seg_counts = (size_t)L * rows * surf_div_up(chunks, kNmsSeg);
        return p;
    }
    OctSet &S = p.S;
    S.n = n; S.nlayers = L; S.rows = rows; S.cols = cols; S.dld = p.dld;
    S.lds0 = p.lds0; S.fuse0 = p.fuse0; S.poly = p.poly;
    long long plane = 0, bits = 0, seg = 0, pbase = 0;
    int row = 0;
    for (int o = 0; o < n; ++o) {
        const int lr = rows >> o, lc = cols >> o;
        S.plane0[o] = plane; S.bits0[o] = bits; S.row0[o] = row; S.seg0[o] = seg;
        S.chunks[o] = surf_div_up(lc, 64); S.nseg[o] = surf_div_up(S.chunks[o], kNmsSeg);
        S.nbx[o] = surf_div_up(lc, 64); S.nby[o] = surf_div_up(lr, 4);
        // every octave's range of k_det_trace_all is padded to a multiple of 8 workgroups (its XCD-contiguous order)
        if (o == 0 && p.fuse0) {   // one workgroup per 14 x 62 tile of interior samples (16 x 64 evaluated) and ALL layers
            S.nbx[0] = surf_div_up(lc, kFuseTX); S.nby[0] = surf_div_up(lr, kFuseTY);
            S.blk_dt[1] = surf_align_up(S.nbx[0] * S.nby[0], 8);
        } else if (o == 0 && p.lds0) {   // one workgroup per 16 x 64 tile and ALL layers
            S.nby[0] = surf_div_up(lr, kLdsTY);
            S.blk_dt[1] = surf_align_up(S.nbx[0] * S.nby[0], 8);
        } else
            S.blk_dt[o + 1] = S.blk_dt[o] + surf_align_up(S.nbx[o] * S.nby[o] * (L + 2), 8);
        S.blk_nms[o + 1] = S.blk_nms[o] + ((o == 0 && p.fuse0) ? 0 : surf_div_up(L * lr, 4) * S.nseg[o]);
        S.blk_wr[o + 1] = S.blk_wr[o] + surf_div_up(L * lr, 4);
        if (o >= 1) {   // (filled whether or not the planes are used: the layout does not depend on the switch)
            const PolyGeo pg = poly_geo(rows, cols, o, pbase);
            S.pld[o] = pg.pld; S.pbase[o] = pbase;
            pbase += pg.plane_words << (2 * o);
        }
        plane += (long long)(L + 2) * lr * p.dld;
        bits += (long long)L * lr * S.chunks[o];
        seg += (long long)L * lr * S.nseg[o];
        row += L * lr;
    }
    p.plane_floats = (size_t)plane;
    p.bits_words = (size_t)bits;
    p.sbits_words = p.fuse0 ? (size_t)L * rows * S.chunks[0] : 0;
    p.seg_counts = (size_t)seg;
    p.row_counts = (size_t)row + n;   // one extra entry (the total) per octave
    p.geo_bytes = sizeof(HaarGeo) * (size_t)n * kDetLayers;
    p.poly_words = p.poly ? (size_t)pbase : 0;
    if (p.poly) { p.grid_poly_x = surf_div_up(cols + 1, 256); p.grid_poly_y = rows + 1; }
    p.grid_det0 = p.fuse0 ? S.blk_dt[1] : 0;
    p.grid_det = S.blk_dt[n] - p.grid_det0;
    p.grid_nms = S.blk_nms[n]; p.grid_scan = n; p.grid_write = S.blk_wr[n];
    p.grid_interp_x = surf_div_up(Z.max_candidates, 256); p.grid_interp_y = n;
    p.grid_compact = n;
    return p;
}

// geometry of every (octave, layer) of the plan's frame, g[octave * kDetLayers + layer] (plan.geo_bytes bytes): uploaded by the handle
// when the plan changes.  With plan.poly the entries of octaves >= 1 address the polyphase planes: tap (ey, ex) of octave o = phase
// plane (ey & m, ex & m), position shifted by (ey >> o, ex >> o)
inline void surf_fill_geometry(const SurfPlan &p, HaarGeo *g)
{
    const int n = p.shape.n_octaves;
    memset(g, 0, sizeof(HaarGeo) * (size_t)n * kDetLayers);
    for (int o = 0; o < n; ++o)
        for (int l = 0; l < p.shape.n_octave_layers + 2; ++l) {
            if (p.poly && o >= 1) {
                const PolyGeo pg = poly_geo(p.shape.rows, p.shape.cols, o, 0);
                const int m = (1 << o) - 1;
                g[o * kDetLayers + l] = haar_geo_off(calc_size(o, l), [&](int ey, int ex) {
                    return (int)((long long)(((ey & m) << o) + (ex & m)) * pg.plane_words + (long long)(ey >> o) * pg.pld + (ex >> o));
                });
            } else g[o * kDetLayers + l] = haar_geo(calc_size(o, l), p.sld);
        }
}

}  // namespace surf
}  // namespace mi
