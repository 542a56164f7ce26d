// The plan of a SURF detect call (csrc/surf_plan.h): launch forms, the layout of every octave's regions in the scratch buffers, the
// element counts the handle allocates, the grids of the all-octave launches and the tap geometry table.  Plain C++, no device.
// The expressions the plan replaced -- make_octset, fused_sizes, fused_supported, fused_geometry, the sizes and the lds_tiles mask of
// surf_api.cpp ensure(), the two downgrade rules of detect_fused -- are restated in namespace old_form and compared with it field by
// field over a sweep of shapes and switches; then the layout's invariants are checked on the plan itself.
#include "surf_plan.h"
#include <cstdio>
#include <vector>

using namespace mi::surf;

static long long fails = 0;
#define CHECK(c) do { if (!(c)) { if (fails < 20) std::printf("FAILED %s:%d: %s  [%s]\n", __FILE__, __LINE__, #c, g_case); ++fails; } } while (0)
static char g_case[160] = "";

namespace old_form {

static int div_up(int a, int b) { return (a + b - 1) / b; }
static int align_up(int a, int b) { return div_up(a, b) * b; }
static int calc_size(int octave, int layer) { return (9 + 6 * layer) << octave; }
constexpr int kMaxFusedOctaves = 6, kDetLayers = 6, kNmsSeg = 8, kLdsTY = 16, kLdsTX = 64, kLdsLayers = 4, kFuseTY = 14, kFuseTX = 62;

struct PolyGeo { int prows, pld; long long plane_words, base; };
static PolyGeo poly_geo(int rows, int cols, int o, long long base)
{
    PolyGeo g;
    g.prows = (rows >> o) + 2; g.pld = align_up((cols >> o) + 2, 64);
    g.plane_words = (long long)g.prows * g.pld; g.base = base;
    return g;
}
static long long poly_total_words(int rows, int cols, int n_octaves)
{
    long long w = 0;
    for (int o = 1; o < n_octaves; ++o) w += poly_geo(rows, cols, o, 0).plane_words << (2 * o);
    return w;
}
// lds & 3: 0 = global taps, 1 = octave 0 on LDS tiles, 2 = ... and its maxima flagged there; lds & 4: polyphase planes
static OctSet make_octset(int rows, int cols, int dld, int n_octaves, int nOctaveLayers, int lds)
{
    OctSet S;
    memset(&S, 0, sizeof(S));
    S.n = n_octaves; S.nlayers = nOctaveLayers; S.rows = rows; S.cols = cols; S.dld = dld;
    S.lds0 = (nOctaveLayers + 2 <= kLdsLayers && (lds & 3)) ? 1 : 0;
    S.fuse0 = (S.lds0 && (lds & 3) >= 2) ? 1 : 0;
    S.poly = (lds & 4) && n_octaves > 1 ? 1 : 0;
    {
        long long base = 0;
        for (int o = 1; o < n_octaves; ++o) {
            const PolyGeo pg = poly_geo(rows, cols, o, base);
            S.pld[o] = pg.pld; S.pbase[o] = base;
            base += pg.plane_words << (2 * o);
        }
    }
    long long plane = 0, bits = 0, seg = 0;
    int row = 0;
    for (int o = 0; o < n_octaves; ++o) {
        const int lr = rows >> o, lc = cols >> o;
        S.plane0[o] = plane; S.bits0[o] = bits; S.row0[o] = row; S.seg0[o] = seg;
        S.chunks[o] = div_up(lc, 64); S.nseg[o] = div_up(S.chunks[o], kNmsSeg);
        S.nbx[o] = div_up(lc, 64); S.nby[o] = div_up(lr, 4);
        if (o == 0 && S.fuse0) {
            S.nbx[0] = div_up(lc, kFuseTX); S.nby[0] = div_up(lr, kFuseTY);
            S.blk_dt[1] = align_up(S.nbx[0] * S.nby[0], 8);
        } else if (o == 0 && S.lds0) {
            S.nby[0] = div_up(lr, kLdsTY);
            S.blk_dt[1] = align_up(S.nbx[0] * S.nby[0], 8);
        } else
        S.blk_dt[o + 1] = S.blk_dt[o] + align_up(S.nbx[o] * S.nby[o] * (nOctaveLayers + 2), 8);
        S.blk_nms[o + 1] = S.blk_nms[o] + ((o == 0 && S.fuse0) ? 0 : div_up(nOctaveLayers * lr, 4) * S.nseg[o]);
        S.blk_wr[o + 1] = S.blk_wr[o] + div_up(nOctaveLayers * lr, 4);
        plane += (long long)(nOctaveLayers + 2) * lr * dld;
        bits += (long long)nOctaveLayers * lr * S.chunks[o];
        seg += (long long)nOctaveLayers * lr * S.nseg[o];
        row += nOctaveLayers * lr;
    }
    return S;
}
static bool fused_supported(int n_octaves, int nOctaveLayers) { return n_octaves <= kMaxFusedOctaves && nOctaveLayers + 2 <= kDetLayers; }
struct FusedSizes { size_t plane_floats, bits_words, seg_counts, row_counts, geo_bytes, poly_words; };
static void fused_sizes(int rows, int cols, int dld, int n_octaves, int nOctaveLayers, FusedSizes *z)
{
    const OctSet S = make_octset(rows, cols, dld, n_octaves, nOctaveLayers, 0);   // "the region sizes do not depend on the octave-0 path"
    const int last = n_octaves - 1, lr = rows >> last;
    z->plane_floats = (size_t)(S.plane0[last] + (long long)(nOctaveLayers + 2) * lr * dld);
    z->bits_words = (size_t)(S.bits0[last] + (long long)nOctaveLayers * lr * S.chunks[last]);
    z->seg_counts = (size_t)(S.seg0[last] + (long long)nOctaveLayers * lr * S.nseg[last]);
    z->row_counts = (size_t)(S.row0[last] + nOctaveLayers * lr + n_octaves);
    z->geo_bytes = sizeof(HaarGeo) * (size_t)n_octaves * kDetLayers;
    z->poly_words = (size_t)poly_total_words(rows, cols, n_octaves);
}
static void fused_geometry(int sld, int n_octaves, int nOctaveLayers, void *geo_host, int rows, int cols, bool poly)
{
    HaarGeo *g = (HaarGeo *)geo_host;
    memset(g, 0, sizeof(HaarGeo) * (size_t)n_octaves * kDetLayers);
    for (int o = 0; o < n_octaves; ++o)
        for (int l = 0; l < nOctaveLayers + 2; ++l) {
            if (poly && o >= 1) {
                const PolyGeo pg = poly_geo(rows, cols, o, 0);
                const int m = (1 << o) - 1;
                g[o * kDetLayers + l] = haar_geo_off(calc_size(o, l), [&](int ey, int ex) {
                    return (int)((long long)(((ey & m) << o) + (ex & m)) * pg.plane_words + (long long)(ey >> o) * pg.pld + (ex >> o));
                });
            } else g[o * kDetLayers + l] = haar_geo(calc_size(o, l), sld);
        }
}
// what ensure() decided and allocated, and what detect_fused then ran
struct Ensure {
    bool fused, use_poly;
    int lds_tiles, launch_mask;   // the handle's mask; the mask detect_fused passed to make_octset after its two downgrade rules
    int sld, vld, dld;
    FusedSizes z;
    size_t sum_words, v_words, bt_words, sbits_words, nlists;
};
static Ensure ensure(int rows, int cols, int octaves, int layers, const SurfKnobs &K)
{
    Ensure e;
    e.sld = align_up(cols + 1, 64); e.vld = align_up(cols, 64); e.dld = align_up(cols, 64);
    e.fused = fused_supported(octaves, layers) && K.fused;
    e.lds_tiles = (K.lds_ok && K.lds) ? 1 : 0;
    if (e.lds_tiles && K.nms0) e.lds_tiles = 2;
    e.use_poly = e.fused && octaves > 1 && K.poly;
    if (e.use_poly) e.lds_tiles |= 4;
    e.z.plane_floats = (size_t)e.dld * rows * (layers + 2);
    e.z.bits_words = (size_t)layers * rows * div_up(cols, 64);
    e.z.row_counts = (size_t)layers * rows + 1;
    e.z.seg_counts = (size_t)layers * rows * div_up(div_up(cols, 64), kNmsSeg);
    e.z.geo_bytes = 0; e.z.poly_words = 0;
    if (e.fused) fused_sizes(rows, cols, e.dld, octaves, layers, &e.z);
    e.nlists = e.fused ? (size_t)octaves : 1;
    e.sum_words = (size_t)e.sld * (rows + 1);
    e.v_words = (size_t)e.vld * rows;
    e.bt_words = (size_t)e.vld * div_up(rows, 32);
    e.sbits_words = e.z.bits_words;   // always allocated, as large as bits
    // detect_fused(..., lds_tiles, s, sbits, poly): sbits was always there, poly only with use_poly
    const bool have_sbits = true, have_poly = e.use_poly;
    int ldsf = e.lds_tiles;
    if ((ldsf & 3) >= 2 && !have_sbits) ldsf = (ldsf & ~3) | 1;
    if (!have_poly) ldsf &= ~4;
    e.launch_mask = ldsf;
    return e;
}
// limits of SURF_CUDA_Invoker's constructor (surf_api.cpp limits(), surf.cuda.cpp:137-156)
static bool limits(int rows, int cols, int n_octaves, int n_octave_layers, float ratio, int *maxCandidates)
{
    if (!(n_octaves > 0 && n_octave_layers > 0 && n_octaves <= 16 && n_octave_layers <= 16)) return false;
    const int min_size = calc_size(n_octaves - 1, 0);
    if (!(rows - min_size >= 0 && cols - min_size >= 0)) return false;
    const int lr = rows >> (n_octaves - 1), lc = cols >> (n_octaves - 1);
    const int min_margin = ((calc_size(n_octaves - 1, 2) >> 1) >> (n_octaves - 1)) + 1;
    if (!(lr - 2 * min_margin > 0 && lc - 2 * min_margin > 0)) return false;
    int mf = (int)((float)(rows * cols) * ratio);
    if (mf > 65535) mf = 65535;
    int mc = (int)(1.5 * mf);
    if (mc > 65535) mc = 65535;
    if (mf <= 0) return false;
    *maxCandidates = mc;
    return true;
}

}  // namespace old_form

template <int L>
static void check_lds_geo()
{
    typedef LdsGeo<L> G;
    const HaarGeo h = haar_geo(9 + 6 * L, kLdsPW);
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 2; ++j) { CHECK(h.xx[i][j] == G::xx(i, j)); CHECK(h.yy[j][i] == G::yy(j, i)); }
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) CHECK(h.xy[i][j] == G::xy(i, j));
    for (int k = 0; k < 3; ++k) { CHECK(h.area[k] == G::axx(k)); CHECK(h.area[3 + k] == G::axx(k)); CHECK(h.ry[k] == 1.0 / G::axx(k)); }
    CHECK(h.area[6] == G::a6 && h.area[7] == G::a7 && h.area[8] == G::a7 && h.area[9] == G::a9);
}

static bool same_sizes(const SurfPlan &a, const SurfPlan &b)
{
    return a.sum_words == b.sum_words && a.v_words == b.v_words && a.bt_words == b.bt_words && a.plane_floats == b.plane_floats &&
           a.bits_words == b.bits_words && a.row_counts == b.row_counts && a.seg_counts == b.seg_counts && a.cand_lists == b.cand_lists &&
           a.cand_items == b.cand_items && a.geo_bytes == b.geo_bytes && a.poly_words == b.poly_words && a.sld == b.sld && a.vld == b.vld &&
           a.dld == b.dld;
}

// the layout's invariants, on the plan alone
static void check_invariants(const SurfPlan &p)
{
    CHECK(!p.fuse0 || p.lds0);
    CHECK(!p.lds0 || p.fused);
    CHECK(!p.poly || (p.fused && p.shape.n_octaves > 1));
    CHECK((p.sbits_words != 0) == p.fuse0);
    CHECK((p.poly_words != 0) == p.poly);
    CHECK(p.cand_items == (size_t)p.cand_lists * p.shape.max_candidates);
    if (!p.fused) {
        CHECK(p.cand_lists == 1 && p.geo_bytes == 0 && p.grid_det == 0 && p.grid_nms == 0);
        return;
    }
    const OctSet &S = p.S;
    const int n = S.n, L = S.nlayers;
    CHECK(S.blk_dt[0] == 0 && S.blk_nms[0] == 0 && S.blk_wr[0] == 0);
    for (int o = 0; o < n; ++o) {
        const int lr = S.rows >> o;
        const bool last = o == n - 1;
        // every region of octave o ends at or before the next octave's starts; the last one ends at the allocated count
        const long long plane_end = S.plane0[o] + (long long)(L + 2) * lr * S.dld;
        const long long bits_end = S.bits0[o] + (long long)L * lr * S.chunks[o];
        const long long seg_end = S.seg0[o] + (long long)L * lr * S.nseg[o];
        const long long row_end = (long long)S.row0[o] + o + L * lr + 1;   // rowcnt: one extra entry (the total) per octave
        CHECK(last ? plane_end == (long long)p.plane_floats : plane_end <= S.plane0[o + 1]);
        CHECK(last ? bits_end == (long long)p.bits_words : bits_end <= S.bits0[o + 1]);
        CHECK(last ? seg_end == (long long)p.seg_counts : seg_end <= S.seg0[o + 1]);
        CHECK(last ? row_end == (long long)p.row_counts : row_end <= (long long)S.row0[o + 1] + o + 1);
        if (o >= 1) {
            const PolyGeo pg = poly_geo(S.rows, S.cols, o, S.pbase[o]);
            const long long poly_end = S.pbase[o] + (pg.plane_words << (2 * o));
            CHECK(S.pld[o] == pg.pld && S.pld[o] % 64 == 0);
            CHECK(last ? poly_end == poly_total_words(S.rows, S.cols, n) : poly_end <= S.pbase[o + 1]);
            if (last && p.poly) CHECK(poly_end == (long long)p.poly_words);
        }
        // k_det_trace_all: every octave's range is a multiple of 8 workgroups and holds its tiles
        CHECK((S.blk_dt[o + 1] - S.blk_dt[o]) % 8 == 0);
        CHECK(S.blk_dt[o + 1] - S.blk_dt[o] >= S.nbx[o] * S.nby[o] * ((o == 0 && p.lds0) ? 1 : L + 2));
        CHECK(S.blk_dt[o + 1] >= S.blk_dt[o] && S.blk_nms[o + 1] >= S.blk_nms[o] && S.blk_wr[o + 1] >= S.blk_wr[o]);
        CHECK(S.chunks[o] * 64 >= (S.cols >> o) && S.nseg[o] * kNmsSeg >= S.chunks[o] && S.chunks[o] * 64 <= S.dld);
        CHECK((S.blk_wr[o + 1] - S.blk_wr[o]) * 4 >= L * lr);
        if (!(o == 0 && p.fuse0)) CHECK(S.blk_nms[o + 1] - S.blk_nms[o] == (S.blk_wr[o + 1] - S.blk_wr[o]) * S.nseg[o]);
    }
    CHECK((S.blk_nms[1] == 0) == p.fuse0);   // octave 0 has no k_nms_flag_all workgroups exactly when its maxima are flagged in the det kernel
    if (p.fuse0) CHECK(S.nbx[0] * kFuseTX >= S.cols && S.nby[0] * kFuseTY >= S.rows);
    else if (p.lds0) CHECK(S.nbx[0] * kLdsTX >= S.cols && S.nby[0] * kLdsTY >= S.rows);
    CHECK(S.lds0 == (int)p.lds0 && S.fuse0 == (int)p.fuse0 && S.poly == (int)p.poly);
    CHECK(p.grid_det0 + p.grid_det == S.blk_dt[n] && p.grid_det0 == (p.fuse0 ? S.blk_dt[1] : 0));
    CHECK(p.grid_nms == S.blk_nms[n] && p.grid_write == S.blk_wr[n] && p.grid_scan == n && p.grid_compact == n && p.grid_interp_y == n);
    CHECK(p.grid_interp_x * 256 >= p.shape.max_candidates && (p.grid_interp_x - 1) * 256 < p.shape.max_candidates);
    CHECK(p.poly ? (p.grid_poly_x * 256 >= S.cols + 1 && p.grid_poly_y == S.rows + 1) : (p.grid_poly_x == 0 && p.grid_poly_y == 0));
    CHECK(p.geo_bytes == sizeof(HaarGeo) * (size_t)n * kDetLayers);
}

int main()
{
    // the compile-time geometry of the LDS tiles against the host's (the runtime self-check of the library, here without a device)
    check_lds_geo<0>(); check_lds_geo<1>(); check_lds_geo<2>(); check_lds_geo<3>();
    CHECK(lds_geometry_self_check());
    CHECK(kLdsPH == 43 && kFuseTX == 62 && kFuseTY == 14 && kNmsSeg == old_form::kNmsSeg);
    CHECK(calc_size(0, 0) == 9 && calc_size(3, 3) == 216);

    std::vector<int> widths, heights;
    for (int w = 40; w <= 300; ++w) widths.push_back(w);
    for (int w : {640, 1283, 1920, 3840}) widths.push_back(w);
    for (int h = 40; h <= 130; ++h) heights.push_back(h);
    for (int h : {480, 1080, 2160}) heights.push_back(h);

    long long swept = 0, compared = 0, per_octaves[8] = {0}, fused_cases = 0;
    std::vector<HaarGeo> tab_new, tab_old;
    for (int rows : heights)
        for (int cols : widths)
            for (int n = 1; n <= 7; ++n)
                for (int L = 1; L <= 5; ++L) {
                    int maxC = 0;
                    const bool ok = old_form::limits(rows, cols, n, L, 0.01f, &maxC);
                    swept += 16;
                    if (!ok) continue;
                    compared += 16;
                    per_octaves[n] += 16;
                    const SurfShape Z = {rows, cols, n, L, maxC};
                    SurfPlan base[4];   // [fused][poly] with lds = nms0 = 0
                    for (int k = 0; k < 32; ++k) {   // the 16 settings of the four switches; then the same with the self-check failed
                        SurfKnobs K;
                        K.fused = k & 1; K.lds = k & 2; K.nms0 = k & 4; K.poly = k & 8; K.lds_ok = !(k & 16);
                        std::snprintf(g_case, sizeof(g_case), "%dx%d o=%d l=%d fused=%d lds=%d nms0=%d poly=%d lds_ok=%d", cols, rows, n, L, K.fused, K.lds,
                                      K.nms0, K.poly, K.lds_ok);
                        const SurfPlan p = surf_make_plan(Z, K);
                        const old_form::Ensure e = old_form::ensure(rows, cols, n, L, K);
                        CHECK(p.shape == Z);
                        CHECK(p.fused == e.fused && p.poly == e.use_poly);
                        CHECK(p.sld == e.sld && p.vld == e.vld && p.dld == e.dld);
                        CHECK(p.sum_words == e.sum_words && p.v_words == e.v_words && p.bt_words == e.bt_words);
                        CHECK(p.plane_floats == e.z.plane_floats && p.bits_words == e.z.bits_words);
                        CHECK(p.row_counts == e.z.row_counts && p.seg_counts == e.z.seg_counts);
                        CHECK((size_t)p.cand_lists == e.nlists && p.cand_items == e.nlists * (size_t)maxC);
                        CHECK(p.geo_bytes == e.z.geo_bytes);
                        CHECK(p.poly_words == (e.use_poly ? e.z.poly_words : 0));   // computed for every all-octave plan, allocated with use_poly only
                        if (e.fused) {
                            ++fused_cases;
                            const OctSet S = old_form::make_octset(rows, cols, e.dld, n, L, e.launch_mask);
                            CHECK(memcmp(&S, &p.S, sizeof(OctSet)) == 0);
                            CHECK(p.lds0 == (S.lds0 != 0) && p.fuse0 == (S.fuse0 != 0) && p.poly == (S.poly != 0));
                            // the sign words: the parent allocated as many as flag words, always; the kernels index octave 0's only, and
                            // only with fuse0 (k_det_nms0, nms_write_row behind oct_args)
                            CHECK(p.sbits_words == (S.fuse0 ? (size_t)L * rows * S.chunks[0] : 0) && p.sbits_words <= e.sbits_words);
                            // the grids of detect_fused
                            const int blk0 = S.fuse0 ? S.blk_dt[1] : 0;
                            CHECK(p.grid_det0 == blk0 && p.grid_det == S.blk_dt[n] - blk0);
                            CHECK(p.grid_nms == S.blk_nms[n] && p.grid_scan == n && p.grid_write == S.blk_wr[n]);
                            CHECK(p.grid_interp_x == old_form::div_up(maxC, 256) && p.grid_interp_y == n && p.grid_compact == n);
                            if (S.poly) CHECK(p.grid_poly_x == old_form::div_up(cols + 1, 256) && p.grid_poly_y == rows + 1);
                        } else {
                            OctSet zero;
                            memset(&zero, 0, sizeof(zero));
                            CHECK(memcmp(&zero, &p.S, sizeof(OctSet)) == 0 && !p.lds0 && !p.fuse0 && !p.poly);
                        }
                        check_invariants(p);
                        // the size figures do not depend on the octave-0 path (the sentence fused_sizes relied on), nor on the self-check
                        const int b = (K.fused ? 1 : 0) + (K.poly ? 2 : 0);
                        if (!K.lds && !K.nms0 && K.lds_ok) base[b] = p;
                        else CHECK(same_sizes(p, base[b]));
                        // a failed self-check is the switch turned off
                        if (!K.lds_ok) {
                            SurfKnobs K0 = K;
                            K0.lds = false; K0.lds_ok = true;
                            const SurfPlan q = surf_make_plan(Z, K0);
                            CHECK(memcmp(&q.S, &p.S, sizeof(OctSet)) == 0 && same_sizes(p, q) && q.sbits_words == p.sbits_words && !p.lds0);
                        }
                        // the geometry table, poly on and off, byte for byte
                        if (p.fused && !K.lds && !K.nms0 && K.lds_ok) {
                            tab_new.assign((size_t)n * kDetLayers, HaarGeo());
                            tab_old.assign((size_t)n * kDetLayers, HaarGeo());
                            CHECK(p.geo_bytes == sizeof(HaarGeo) * tab_new.size());
                            surf_fill_geometry(p, tab_new.data());
                            old_form::fused_geometry(e.sld, n, L, tab_old.data(), rows, cols, e.use_poly);
                            CHECK(memcmp(tab_new.data(), tab_old.data(), p.geo_bytes) == 0);
                            // ... and every tap of every valid sample lies inside what it reads: the integral image, or the
                            // octave's 4^o phase planes
                            for (int o = 0; o < n; ++o)
                                for (int l = 0; l < L + 2; ++l) {
                                    const int size = calc_size(o, l);
                                    if (size > rows || size > cols) continue;
                                    const int si = 1 + ((rows - size) >> o), sj = 1 + ((cols - size) >> o);
                                    const HaarGeo &g = tab_new[(size_t)o * kDetLayers + l];
                                    const bool pl = p.poly && o >= 1;
                                    const long long lane_max = pl ? (long long)(si - 1) * p.S.pld[o] + (sj - 1)
                                                                  : (long long)((si - 1) << o) * p.sld + ((sj - 1) << o);
                                    const long long words = pl ? poly_geo(rows, cols, o, 0).plane_words << (2 * o) : (long long)p.sum_words;
                                    int taps[32];   // xx, yy, xy: 32 offsets back to back
                                    memcpy(taps, &g, sizeof(taps));
                                    for (int q = 0; q < 32; ++q) CHECK(taps[q] >= 0 && taps[q] + lane_max < words);
                                }
                        }
                    }
                    // the candidate count changes nothing but the lists and the grid over them (the handle keeps larger lists)
                    {
                        SurfKnobs K = {true, true, false, true, true};
                        SurfShape Z2 = Z;
                        Z2.max_candidates = maxC / 2 + 1;
                        const SurfPlan a = surf_make_plan(Z, K), b2 = surf_make_plan(Z2, K);
                        CHECK(memcmp(&a.S, &b2.S, sizeof(OctSet)) == 0 && a.plane_floats == b2.plane_floats && a.bits_words == b2.bits_words &&
                              a.row_counts == b2.row_counts && a.seg_counts == b2.seg_counts && a.poly_words == b2.poly_words &&
                              a.geo_bytes == b2.geo_bytes && a.cand_lists == b2.cand_lists && b2.cand_items <= a.cand_items);
                    }
                }
    g_case[0] = 0;
    // What share of the sweep limits() lets through is arithmetic: rows and cols of at least 23 << (octaves - 1) (the margin rule; the
    // size rule 9 << (octaves - 1) is weaker).  For the sweep above that is 57 031 of 174 370 (shape, octaves) pairs = 32.7 %: most of
    // the small shapes do not admit four or more octaves.  The counts are asserted exactly, so that no case can drop out silently.
    long long expect = 0;
    for (int n = 1; n <= 7; ++n) {
        long long vh = 0, vw = 0;
        for (int h : heights) vh += h >= (23 << (n - 1));
        for (int w : widths) vw += w >= (23 << (n - 1));
        CHECK(per_octaves[n] == vh * vw * 5 * 16 && per_octaves[n] > 0);
        expect += vh * vw * 5 * 16;
    }
    CHECK(swept == (long long)heights.size() * (long long)widths.size() * 7 * 5 * 16);
    CHECK(compared == expect && compared == 57031LL * 5 * 16);
    CHECK(fused_cases > compared / 4);
    std::printf("surf_plan_test: %lld of %lld cases of the sweep compared (%.1f %%; limits() rejects the rest), %lld of them all-octave plans\n",
                compared, swept, 100.0 * (double)compared / (double)swept, fused_cases);

    // the shapes and forms the GPU suite runs, spelled out
    {
        const SurfKnobs K = {true, true, false, true, true};
        const SurfPlan p = surf_make_plan(SurfShape{2160, 3840, 4, 2, 65535}, K);   // the benchmark's frame
        CHECK(p.fused && p.lds0 && !p.fuse0 && p.poly && p.sld == 3904 && p.dld == 3840);
        CHECK(p.S.nbx[0] == 60 && p.S.nby[0] == 135 && p.S.blk_dt[1] == 8104 && p.cand_lists == 4);
        const SurfPlan q = surf_make_plan(SurfShape{300, 400, 3, 5, 9000}, K);        // nOctaveLayers + 2 > kDetLayers: octave by octave
        CHECK(!q.fused && !q.lds0 && !q.poly && q.cand_lists == 1 && q.plane_floats == (size_t)448 * 300 * 7);
        const SurfPlan r = surf_make_plan(SurfShape{300, 400, 4, 4, 9000}, K);        // 6 layers: all octaves, but no LDS tiles (4 layers at most)
        CHECK(r.fused && !r.lds0 && r.poly);
        SurfKnobs N = K;
        N.nms0 = true;
        const SurfPlan f = surf_make_plan(SurfShape{98, 124, 2, 2, 182}, N);          // 124 = 2 x 62: exactly two tiles of the flagged form
        CHECK(f.fuse0 && f.S.nbx[0] == 2 && f.S.nby[0] == 7 && f.S.blk_nms[1] == 0);
        CHECK(surf_make_plan(SurfShape{98, 125, 2, 2, 182}, N).S.nbx[0] == 3);
    }
    if (fails) { std::printf("surf_plan_test: %lld check(s) FAILED\n", fails); return 1; }
    std::printf("surf_plan_test: ok\n");
    return 0;
}
