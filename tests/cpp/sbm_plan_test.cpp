// The plan of StereoBM's launches (csrc/sbm_plan.h): tile geometry, the LDS layouts of k_block_match and k_textureness_fused, the band
// rule, the validator and sbm_make_plan.  Plain C++, no device.  The expressions the plan replaced -- Cfg<R>'s widths, the LDS sizes
// written out in k_block_match / launch_bm and in k_textureness_fused / textureness_fused(), the band rule, grid and block of
// block_match_impl, textureness_scratch_dims, check_bm_params -- are restated in namespace old_form and compared with it field by field
// over a sweep of radii, disparity ranges, batch sizes, image sizes and switches; then the layouts' invariants are checked on the plan.
#include "sbm_plan.h"
#include <cstdio>
#include <cstring>
#include <type_traits>

using namespace mi::sbm;

static long long fails = 0;
static char g_case[160] = "";
#define CHECK(c) do { if (!(c)) { if (fails < 20) std::printf("FAILED %s:%d: %s  [%s]\n", __FILE__, __LINE__, #c, g_case); ++fails; } } while (0)

namespace old_form {

static int div_up(int a, int b) { return (a + b - 1) / b; }
static int align_up(int a, int b) { return div_up(a, b) * b; }
static int tile_w_of(int R)   // the band rule's width
{
    const int t = (64 - 2 * R) & ~3;
    return t < 16 ? 16 : t;
}
static bool packed(int R) { return R <= 12; }
static int TW(int R) { return packed(R) ? 48 : tile_w_of(R); }   // Cfg<R>::TW
static int NC(int R) { return TW(R) + 2 * R; }
static int LS(int R) { return (NC(R) + 15) / 16 * 16; }
static int band_rows(int rows, int cols, int ndisp, int R, int pairs)   // block_match_impl
{
    const int nsets = div_up(ndisp, 64);
    const int xt = div_up(cols - ndisp - 2 * R, tile_w_of(R));
    const int vrows = rows - 2 * R;
    int bands = div_up(5120, xt * nsets * pairs);
    int rb = div_up(vrows, bands > 0 ? bands : 1);
    rb = rb < 2 * R + 2 ? 2 * R + 2 : rb;
    rb = rb > 48 ? 48 : rb;
    return rb;
}
static int RS(int R, int nsets) { return (NC(R) + nsets * 64 - 1 + 3) / 4 * 4 + 4; }
static size_t lds(int R, int nsets, int rb, bool with_tbuf)   // launch_bm
{
    size_t b = (size_t)(rb + 2 * R) * (LS(R) + RS(R, nsets)) + (size_t)2 * nsets * 128 * sizeof(unsigned);
    b = (b + 15) / 16 * 16;
    return with_tbuf ? b + (size_t)nsets * 16 * 68 * sizeof(unsigned) : b;
}
static size_t texf_lds(int winsz)   // textureness_fused()
{
    const int W2 = winsz / 2;
    const int TC = 64 + 2 * W2, TRR = 32 + 2 * W2;
    return sizeof(unsigned short) * ((size_t)(TRR + 2) * (TC + 2) + (((size_t)TRR * TC + 1) & ~(size_t)1)) + sizeof(int) * 4 * 128;
}
static int check(int ndisp, int winsz, int rows, int cols, const char **msg)   // check_bm_params
{
    if (!(0 < ndisp && ndisp <= 256)) { *msg = "numDisparities must be in (0,256]"; return MI_ERR_BAD_ARG; }
    if (!(ndisp % 8 == 0)) { *msg = "numDisparities must be a multiple of 8"; return MI_ERR_BAD_ARG; }
    if (!(winsz % 2 == 1)) { *msg = "blockSize must be odd"; return MI_ERR_BAD_ARG; }
    if (!((winsz >> 1) >= 1 && (winsz >> 1) <= 25)) { *msg = "Unsupported window size"; return MI_ERR_BAD_ARG; }
    if (!(cols - ndisp - 2 * (winsz >> 1) > 0 && rows - 2 * (winsz >> 1) > 0)) { *msg = "image too small for numDisparities + blockSize"; return MI_ERR_BAD_SIZE; }
    *msg = nullptr;
    return MI_OK;
}

}  // namespace old_form

static size_t g_max_lds = 0;
static int g_max_lds_R = 0, g_max_lds_nd = 0, g_max_lds_rb = 0;

// the layout of one launch against the restated sizes, and its invariants
static void check_bm_layout(int R, int nsets, int rb, bool wt)
{
    const BmLds L = bm_lds(R, nsets, rb, wt);
    CHECK(L.LS() == old_form::LS(R) && L.RS() == old_form::RS(R, nsets));
    CHECK(L.bytes() == old_form::lds(R, nsets, rb, wt));
    CHECK(L.tbuf() == old_form::lds(R, nsets, rb, false));
    // regions in order, one behind the other: left rows at 0, right rows, comb, (aligned) the waves' transposition buffers
    const size_t srows = (size_t)(rb + 2 * R), right0 = L.left(), comb0 = right0 + L.right(), comb1 = comb0 + L.comb();
    CHECK(L.left() == srows * L.LS() && L.right() == srows * L.RS() && L.comb() == sizeof(unsigned) * 2 * nsets * 2 * 64);
    CHECK(L.LS() >= L.NC() && L.LS() % 4 == 0 && L.RS() % 4 == 0);
    // a lane's reads of a right row (NRW dwords from byte offset (nsets * 64 - 1 - d) & ~3) stay inside the row
    CHECK(((nsets * 64 - 1) >> 2) * 4 + ((L.NC() + 3) / 4 + 1) * 4 <= L.RS());
    CHECK(comb0 % 4 == 0 && comb1 <= L.tbuf() && L.tbuf() - comb1 < 16 && L.tbuf() % 16 == 0);
    // a wave's slice holds its [16][BM_TP] dwords (the highest index written is 15 * BM_TP + 63) and ends where the next begins
    CHECK(L.tstride() == sizeof(unsigned) * 16 * BM_TP && 15 * BM_TP + 63 < 16 * BM_TP && L.tstride() % 16 == 0);
    CHECK(L.bytes() == (wt ? L.tbuf() + nsets * L.tstride() : L.tbuf()));
}

// the kernel's form of the layout (radius as a type) is the host's
template <int R>
static void check_typed_layout()
{
    for (int nsets = 1; nsets <= 4; ++nsets)
        for (int rb : {1, 16, 48})
            for (int wt = 0; wt < 2; ++wt) {
                std::snprintf(g_case, sizeof(g_case), "typed R %d nsets %d rb %d wt %d", R, nsets, rb, wt);
                const BmLdsT<std::integral_constant<int, R>> T = {{}, nsets, rb, wt != 0};
                const BmLds L = bm_lds(R, nsets, rb, wt != 0);
                CHECK(T.NC() == L.NC() && T.LS() == L.LS() && T.RS() == L.RS() && T.left() == L.left() && T.right() == L.right() && T.comb() == L.comb() &&
                      T.tbuf() == L.tbuf() && T.tstride() == L.tstride() && T.bytes() == L.bytes());
                CHECK(T.NC() == Cfg<R>::NC && T.LS() == Cfg<R>::LS && bm_tile_w(R) == Cfg<R>::TW);
            }
}
template <int... R>
static void check_typed_layouts(std::integer_sequence<int, R...>) { (check_typed_layout<R + 1>(), ...); }

int main()
{
    long long compared = 0, rejected = 0;
    static const int ndisps[] = {8, 64, 72, 128, 200, 256}, pairss[] = {1, 2, 5, 16, 64};
    for (int R = 1; R <= 25; ++R)
        for (int ndisp : ndisps) {
            const int winsz = 2 * R + 1, TW = old_form::TW(R), nsets = old_form::div_up(ndisp, 64);
            // widths: 1, TW and TW + 1 valid columns (the smallest image, one full tile, one tile and a column), two tiles and a ragged one,
            // and fixed ones up to 1080p (the small ones are rejected for wide disparity ranges); heights likewise around the band rule
            const int widths[] = {ndisp + 2 * R + 1, ndisp + 2 * R + TW, ndisp + 2 * R + TW + 1, ndisp + 2 * R + 2 * TW + 5, 64, 320, 641, 1920};
            const int heights[] = {2 * R + 1, 2 * R + 2, 4 * R + 3, 4 * R + 4, 6 * R + 5, 2 * R + 49, 16, 40, 481, 1080};
            for (int cols : widths)
                for (int rows : heights)
                    for (int pairs : pairss)
                        for (int sw = 0; sw < 8; ++sw)
                            for (int uniq : {0, 10}) {
                                const BmSwitches S = {sw & 1, (sw >> 1) & 1, (sw & 4) ? 24 : 0};
                                std::snprintf(g_case, sizeof(g_case), "R %d ndisp %d %dx%d pairs %d wt %d swz %d rows %d uniq %d", R, ndisp, cols, rows, pairs, S.wt, S.swz, S.rows, uniq);
                                const BmPlan P = sbm_make_plan(rows, cols, ndisp, winsz, uniq, pairs, S);
                                const char *msg;
                                const int rc = old_form::check(ndisp, winsz, rows, cols, &msg);
                                CHECK(P.err.code == rc);
                                if (rc) { ++rejected; CHECK(P.err.msg && !std::strcmp(P.err.msg, msg)); continue; }
                                ++compared;
                                const int rb_rule = old_form::band_rows(rows, cols, ndisp, R, pairs), rb = S.rows > 0 ? S.rows : rb_rule;
                                CHECK(bm_band_rows(rows, cols, ndisp, R, pairs) == rb_rule);
                                CHECK(P.rows == rows && P.cols == cols && P.ndisp == ndisp && P.R == R && P.nsets == nsets && P.rb == rb && P.swz == S.swz);
                                CHECK(P.grid[0] == old_form::div_up(cols - ndisp - 2 * R, TW) && P.grid[1] == old_form::div_up(rows - 2 * R, rb) && P.grid[2] == pairs);
                                CHECK(P.block == 64 * nsets);
#ifdef MIFLOW_EXPERIMENTS
                                const bool wt = old_form::packed(R) && S.wt;
#else
                                const bool wt = old_form::packed(R);
#endif
                                CHECK(P.wt == wt && P.verify == (uniq > 0));
                                CHECK(P.lds_first == old_form::lds(R, nsets, rb, wt) && P.lds_verify == old_form::lds(R, nsets, rb, false));
                                CHECK(P.thresh_scale == (float)(1.0 + uniq / 100.0f));
                                check_bm_layout(R, nsets, rb, wt);
                                check_bm_layout(R, nsets, rb, false);
                                // coverage: the grid reaches every valid column and row
                                CHECK(P.grid[0] * bm_tile_w(R) >= cols - ndisp - 2 * R && (P.grid[0] - 1) * bm_tile_w(R) < cols - ndisp - 2 * R);
                                CHECK(P.grid[1] * rb >= rows - 2 * R && (P.grid[1] - 1) * rb < rows - 2 * R);
                                if (S.rows <= 0) {   // the band rule's bounds, and with them the LDS a launch can ask for
                                    CHECK((2 * R + 2 < 48 ? 2 * R + 2 : 48) <= rb && rb <= 48);
                                    CHECK(P.lds_first < 64 * 1024 && P.lds_verify <= P.lds_first);
                                    // (200 and 256 disparities are both four sets: the last one found is named)
                                    if (P.lds_first >= g_max_lds) { g_max_lds = P.lds_first; g_max_lds_R = R; g_max_lds_nd = ndisp; g_max_lds_rb = rb; }
                                }
                            }
        }
    std::snprintf(g_case, sizeof(g_case), "totals");
    CHECK(compared == 777440 && rejected == 182560);
    // by hand: R = 12, 256 disparities, 48-row bands: 72 rows x (80 + 332) B + 4 KB of comb + 4 waves x 4 352 B = 51 168 B
    CHECK(g_max_lds == 51168 && g_max_lds_R == 12 && g_max_lds_nd == 256 && g_max_lds_rb == 48);
    check_typed_layouts(std::make_integer_sequence<int, 25>{});

    // the band rule's width is not the tile's for R 1..6 and 9..12
    for (int R = 1; R <= 25; ++R) {
        std::snprintf(g_case, sizeof(g_case), "widths R %d", R);
        CHECK(bm_tile_w(R) == old_form::TW(R) && bm_legacy_w(R) == old_form::tile_w_of(R) && bm_packed(R) == old_form::packed(R));
        CHECK((bm_legacy_w(R) != bm_tile_w(R)) == (R <= 6 || (R >= 9 && R <= 12)));
    }
    // known band heights (bench.py's mirror pins the same two)
    CHECK(bm_band_rows(1080, 1920, 128, 7, 1) == 16);
    CHECK(bm_band_rows(1080, 1920, 128, 7, 8) == 48);

    // the fused textureness filter's LDS and the two-pass form's scratch plane
    size_t max_texf = 0;
    for (int winsz = 1; winsz <= 51; winsz += 2) {
        std::snprintf(g_case, sizeof(g_case), "texf winsz %d", winsz);
        const TexfLds T = texf_lds(winsz / 2);
        CHECK(T.bytes == old_form::texf_lds(winsz));
        CHECK(T.TC == 64 + 2 * (winsz / 2) && T.TRR == TEXF_ROWS + 2 * (winsz / 2) && T.BC == T.TC + 2 && T.BR == T.TRR + 2);
        // B, S (u16 words, S ending on a dword) and the four waves' 128 column sums, one behind the other
        CHECK(T.B == T.BR * T.BC && T.S >= T.TRR * T.TC && T.S - T.TRR * T.TC < 2 && (T.B + T.S) % 2 == 0);
        CHECK(T.bytes == sizeof(unsigned short) * (size_t)(T.B + T.S) + 4 * 128 * sizeof(int) && T.bytes < 64 * 1024);
        CHECK(64 + 2 * (winsz / 2) <= 128);   // the window of output column 63 ends inside a wave's 128 column sums
        if (T.bytes > max_texf) max_texf = T.bytes;
    }
    for (int rows : {1, 17, 480, 1080})
        for (int cols : {1, 63, 64, 65, 641, 1920}) {
            std::snprintf(g_case, sizeof(g_case), "scratch dims %dx%d", cols, rows);
            int sld = 0, sh = 0;
            textureness_scratch_dims(rows, cols, &sld, &sh);
            CHECK(sld == old_form::align_up(cols, 64) + 2 * 32 && sh == rows + 2 * 26 && TEX_MX == 32 && TEX_MY == 26);
        }

    // the validator: one rejected case for each requirement, with its code and text; then what it admits
    struct { int ndisp, winsz, rows, cols, code; const char *msg; } bad[] = {
        {0, 15, 100, 400, MI_ERR_BAD_ARG, "numDisparities must be in (0,256]"},
        {264, 15, 100, 400, MI_ERR_BAD_ARG, "numDisparities must be in (0,256]"},
        {12, 15, 100, 400, MI_ERR_BAD_ARG, "numDisparities must be a multiple of 8"},
        {64, 14, 100, 400, MI_ERR_BAD_ARG, "blockSize must be odd"},
        {64, 1, 100, 400, MI_ERR_BAD_ARG, "Unsupported window size"},
        {64, 53, 100, 400, MI_ERR_BAD_ARG, "Unsupported window size"},
        {64, 15, 100, 78, MI_ERR_BAD_SIZE, "image too small for numDisparities + blockSize"},
        {64, 15, 14, 400, MI_ERR_BAD_SIZE, "image too small for numDisparities + blockSize"},
    };
    for (const auto &b : bad) {
        std::snprintf(g_case, sizeof(g_case), "bad ndisp %d winsz %d %dx%d", b.ndisp, b.winsz, b.cols, b.rows);
        const SbmErr e = sbm_check(b.ndisp, b.winsz, b.rows, b.cols);
        const char *msg;
        CHECK(e.code == b.code && e.msg && !std::strcmp(e.msg, b.msg) && old_form::check(b.ndisp, b.winsz, b.rows, b.cols, &msg) == b.code);
        CHECK(sbm_make_plan(b.rows, b.cols, b.ndisp, b.winsz, 0, 1, BmSwitches{1, 1, 0}).err.code == b.code);
    }
    std::snprintf(g_case, sizeof(g_case), "validator");
    CHECK(sbm_check(64, 15, 15, 79).code == MI_OK && sbm_check(256, 51, 51, 307).code == MI_OK && sbm_check(8, 3, 3, 11).code == MI_OK);
    // the window alone (the textureness stage: a 1 x 1 window is allowed there, as before)
    CHECK(sbm_check_window(1, 0).code == MI_OK && sbm_check_window(51, 0).code == MI_OK && sbm_check_window(1, 1).code == MI_ERR_BAD_ARG);
    CHECK(sbm_check_window(53, 0).code == MI_ERR_BAD_ARG && sbm_check_window(8, 0).code == MI_ERR_BAD_ARG && sbm_check_window(-1, 0).code == MI_ERR_BAD_ARG);

    std::printf("compared %lld plans (%lld rejected shapes skipped); largest block-matching LDS %zu B (R %d, %d disparities, %d-row bands), largest fused-textureness LDS %zu B\n",
                compared, rejected, g_max_lds, g_max_lds_R, g_max_lds_nd, g_max_lds_rb, max_texf);
    if (fails) { std::printf("sbm_plan_test: %lld FAILED\n", fails); return 1; }
    std::printf("sbm_plan_test: ok\n");
    return 0;
}
