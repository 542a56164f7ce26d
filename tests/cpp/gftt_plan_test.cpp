// The plan of CornernessCriteria / CornersDetector (opencv_contrib_amd/csrc/gftt_plan.h) is pure host arithmetic: the validators, the
// launch form of the response and its tiles, the capacity, the scratch layout, the launch list with the sort's steps, and the host loop
// of minDistance.  Stand-alone program (its own main), built with and without the address and undefined-behaviour sanitizers by
// tests/test_gftt_plan.py.  With "constants" as its argument it prints the plan's constants, which the GPU tests take their shapes from.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "gftt_plan.h"

using namespace mi::gftt;

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); exit(1); } } while (0)

static int ceil_div(int a, int b) { return (a + b - 1) / b; }

static int largest_fused()
{
    int b = 1;
    while (gftt_fused_lds(b + 1) <= GFTT_LDS_LIMIT) ++b;
    return b;
}

static void check_response(int rows, int cols, int bs, int form)
{
    const GfttResponsePlan p = gftt_response_plan(rows, cols, bs, form);
    const bool fits = gftt_fused_lds(bs) <= GFTT_LDS_LIMIT;
    if (form == GFTT_FORM_FUSED && !fits) { CHECK(p.err.code == MI_ERR_BAD_ARG && p.launches.empty()); return; }
    CHECK(p.err.code == MI_OK && p.rows == rows && p.cols == cols && p.block_size == bs);
    CHECK(p.form == (form != GFTT_FORM_AUTO ? form : fits ? GFTT_FORM_FUSED : GFTT_FORM_PLANES));
    CHECK(p.lo == bs / 2 && p.lo + p.hi + 1 == bs && p.hi <= p.lo);   // corners.cu:73-76: asymmetric for even sizes
    CHECK(p.tiles_x == ceil_div(cols, GFTT_TILE_W) && p.tiles_y == ceil_div(rows, GFTT_TILE_H) && p.ntiles == p.tiles_x * p.tiles_y);
    CHECK(p.tiles_x * GFTT_TILE_W >= cols && (p.tiles_x - 1) * GFTT_TILE_W < cols);
    CHECK(p.tiles_y * GFTT_TILE_H >= rows && (p.tiles_y - 1) * GFTT_TILE_H < rows);
    if (p.form == GFTT_FORM_FUSED) {
        CHECK(p.launches.size() == 1 && p.launches[0].kernel == GFTT_K_RESPONSE);
        // the Dx / Dy tile holds every window of the tile's pixels, the source tile one pixel more on each side
        CHECK(p.dw == GFTT_TILE_W + p.lo + p.hi && p.dh == GFTT_TILE_H + p.lo + p.hi && p.sw == p.dw + 2 && p.sh == p.dh + 2);
        CHECK(p.lds_bytes == ((size_t)p.sw * p.sh + 2 * (size_t)p.dw * p.dh) * 4 && p.lds_bytes <= GFTT_LDS_LIMIT);
        CHECK(p.launches[0].lds == p.lds_bytes);
    } else {
        CHECK(p.launches.size() == 2 && p.launches[0].kernel == GFTT_K_DERIV && p.launches[1].kernel == GFTT_K_WINDOW);
        CHECK(p.launches[0].lds == 0 && p.launches[1].lds == 0);
    }
    for (const GfttLaunch &k : p.launches)
        CHECK(k.grid_x == (unsigned)p.tiles_x && k.grid_y == (unsigned)p.tiles_y && k.block == GFTT_BLOCK && GFTT_BLOCK == 4 * GFTT_TILE_W);
}

// a bitonic network of the plan's launches run on the host: what the kernels do, step for step
static void run_sort(const std::vector<GfttLaunch> &ls, std::vector<unsigned long long> &a, int npad)
{
    auto step = [&](int k, int j) {
        for (int i = 0; i < npad; ++i) {
            const int l = i | j;
            if ((i & j) || l == i) continue;
            const bool asc = (i & k) == 0;
            if ((a[i] > a[l]) == asc) std::swap(a[i], a[l]);
        }
    };
    for (const GfttLaunch &l : ls) {
        if (l.kernel == GFTT_K_SORT_LOCAL) { for (int k = 2; k <= GFTT_SORT_TILE; k <<= 1) for (int j = k / 2; j >= 1; j >>= 1) step(k, j); }
        else if (l.k > npad) continue;
        else if (l.kernel == GFTT_K_SORT_GLOBAL) step(l.k, l.j);
        else for (int j = GFTT_SORT_TILE / 2; j >= 1; j >>= 1) step(l.k, j);
    }
}

static void check_sort(int sort_cap, int count)
{
    std::vector<GfttLaunch> ls;
    gftt_sort_launches(sort_cap, &ls);
    CHECK(ls[0].kernel == GFTT_K_SORT_LOCAL && ls[0].grid_x == (unsigned)(sort_cap / GFTT_SORT_TILE) && ls[0].block == GFTT_SORT_THREADS);
    int levels = 0;
    for (int k = sort_cap; k > GFTT_SORT_TILE; k >>= 1) ++levels;
    CHECK((int)ls.size() == 1 + levels + levels * (levels + 1) / 2);
    for (const GfttLaunch &l : ls) {
        if (l.kernel == GFTT_K_SORT_GLOBAL) CHECK(l.j >= GFTT_SORT_TILE && l.j < l.k && (size_t)l.grid_x * l.block * 2 == (size_t)sort_cap);
        if (l.kernel == GFTT_K_SORT_MERGE) CHECK(l.k > GFTT_SORT_TILE && l.k <= sort_cap && l.grid_x == (unsigned)(sort_cap / GFTT_SORT_TILE));
    }
    int npad = GFTT_SORT_TILE;
    while (npad < count) npad <<= 1;
    CHECK(npad <= sort_cap);
    std::vector<unsigned long long> a(sort_cap, ~0ull), want;
    unsigned long long s = 88172645463325252ull;
    for (int i = 0; i < count; ++i) { s ^= s << 13; s ^= s >> 7; s ^= s << 17; a[i] = s % 1000; }   // many ties
    want.assign(a.begin(), a.begin() + count);
    std::sort(want.begin(), want.end());
    run_sort(ls, a, npad);
    for (int i = 0; i < count; ++i) CHECK(a[i] == want[i]);
}

static void check_plan(int rows, int cols, int bs)
{
    const GfttPlan p = gftt_make_plan(rows, cols, bs, GFTT_FORM_AUTO);
    CHECK(p.err.code == MI_OK);
    const long long area = (long long)rows * cols;
    CHECK(p.capacity == std::max(1000, (int)((double)area * 0.05)) && p.capacity == gftt_capacity(rows, cols));
    CHECK(p.sort_cap >= p.capacity && p.sort_cap >= GFTT_SORT_TILE && (p.sort_cap & (p.sort_cap - 1)) == 0);
    CHECK(p.sort_cap == GFTT_SORT_TILE || p.sort_cap / 2 < p.capacity);
    CHECK(p.segs_x == ceil_div(cols, GFTT_SEG) && p.nseg == rows * p.segs_x && p.nfind == ceil_div(p.nseg, GFTT_FIND_SEGS));
    const bool planes = p.resp.form == GFTT_FORM_PLANES;
    const size_t plane = (size_t)area * 4;
    // areas in order, aligned, none overlapping, each holding what its kernel writes
    const size_t offs[] = {p.off_resp, p.off_dx, p.off_dy, p.off_wgmax, p.off_ctl, p.off_masks, p.off_bcount, p.off_bbase, p.off_keys, p.off_pts,
                           p.scratch_bytes};
    const size_t need[] = {plane, planes ? plane : 0, planes ? plane : 0, (size_t)p.resp.ntiles * 4, GFTT_CTL_INTS * 4, (size_t)p.nseg * 8,
                           (size_t)p.nfind * 4, (size_t)p.nfind * 4, (size_t)p.sort_cap * 8, (size_t)p.capacity * 8};
    CHECK(offs[0] == 0);
    for (int i = 0; i < 10; ++i) CHECK(offs[i] % GFTT_ALIGN == 0 && offs[i + 1] >= offs[i] + need[i] && offs[i + 1] < offs[i] + need[i] + GFTT_ALIGN);
    // the list: response, threshold, find, scan, emit, the sort, points
    size_t i = p.resp.launches.size();
    CHECK(p.launches.size() > i + 5);
    CHECK(p.launches[i].kernel == GFTT_K_THRESHOLD && p.launches[i].grid_x == 1 && p.launches[i].block == GFTT_SCAN_THREADS); ++i;
    CHECK(p.launches[i].kernel == GFTT_K_FIND && p.launches[i].grid_x == (unsigned)p.nfind && p.launches[i].block == GFTT_BLOCK); ++i;
    CHECK(p.launches[i].kernel == GFTT_K_SCAN && p.launches[i].grid_x == 1 && p.launches[i].block == GFTT_SCAN_THREADS); ++i;
    CHECK(p.launches[i].kernel == GFTT_K_EMIT && p.launches[i].grid_x == (unsigned)p.nfind); ++i;
    std::vector<GfttLaunch> ls;
    gftt_sort_launches(p.sort_cap, &ls);
    for (const GfttLaunch &l : ls) { CHECK(p.launches[i].kernel == l.kernel && p.launches[i].k == l.k && p.launches[i].j == l.j && p.launches[i].grid_x == l.grid_x); ++i; }
    CHECK(p.launches[i].kernel == GFTT_K_POINTS && (size_t)p.launches[i].grid_x * GFTT_BLOCK >= (size_t)p.capacity && i + 1 == p.launches.size());
    CHECK(gftt_output_cols(rows, cols, 0) == p.capacity && gftt_output_cols(rows, cols, 10) == 10 &&
          gftt_output_cols(rows, cols, p.capacity + 1) == p.capacity);
}

static void check_validators()
{
    CHECK(gftt_check_corner(MI_8UC1, 3, 3, GFTT_BORDER_REFLECT101).code == MI_OK && gftt_check_corner(MI_32FC1, 255, 3, GFTT_BORDER_REFLECT).code == MI_OK);
    CHECK(gftt_check_corner(MI_8UC1, 3, 3, GFTT_BORDER_REPLICATE).code == MI_OK);
    for (int ksize : {-1, 0, 1, 5, 7}) CHECK(gftt_check_corner(MI_8UC1, 3, ksize, GFTT_BORDER_REFLECT101).code == MI_ERR_NOT_IMPL);
    for (int border : {0, 3, 5, 16}) CHECK(gftt_check_corner(MI_8UC1, 3, 3, border).code == MI_ERR_BAD_ARG);   // CONSTANT, WRAP, TRANSPARENT, ISOLATED
    CHECK(gftt_check_corner(MI_32SC1, 3, 3, GFTT_BORDER_REFLECT101).code == MI_ERR_BAD_TYPE);
    CHECK(gftt_check_corner(MI_8UC1, 0, 3, GFTT_BORDER_REFLECT101).code == MI_ERR_BAD_ARG && gftt_check_corner(MI_8UC1, 256, 3, 4).code == MI_ERR_BAD_ARG);
    CHECK(gftt_check_params(0, 0.01, 0).code == MI_OK && gftt_check_params(1000, 1e-9, 7.5).code == MI_OK);
    CHECK(gftt_check_params(-1, 0.01, 0).code == MI_ERR_BAD_ARG && gftt_check_params(0, 0.0, 0).code == MI_ERR_BAD_ARG);
    CHECK(gftt_check_params(0, -0.5, 0).code == MI_ERR_BAD_ARG && gftt_check_params(0, 0.01, -1e-9).code == MI_ERR_BAD_ARG);
    CHECK(gftt_check_params(0, std::nan(""), 0).code == MI_ERR_BAD_ARG && gftt_check_params(0, 0.01, std::nan("")).code == MI_ERR_BAD_ARG);
    CHECK(gftt_check_params(0, 0.01, 1073741824.0).code == MI_ERR_BAD_ARG);
    const GfttMatDesc ok = {40, 140, MI_8UC1, 140, true};
    CHECK(gftt_check_image(ok, MI_8UC1, nullptr).code == MI_OK && gftt_check_image(ok, MI_32FC1, nullptr).code == MI_ERR_BAD_TYPE);
    GfttMatDesc m = ok;
    CHECK(gftt_check_image(ok, MI_8UC1, &m).code == MI_OK);
    m.cols = 139; CHECK(gftt_check_image(ok, MI_8UC1, &m).code == MI_ERR_BAD_SIZE);
    m = ok; m.type = MI_32FC1; CHECK(gftt_check_image(ok, MI_8UC1, &m).code == MI_ERR_BAD_TYPE);
    m = ok; m.has_data = false; m.type = 77; CHECK(gftt_check_image(ok, MI_8UC1, &m).code == MI_OK);   // a mask without data is no mask
    GfttMatDesc d = ok;
    d.step = 139; CHECK(gftt_check_image(d, MI_8UC1, nullptr).code == MI_ERR_BAD_ARG);
    d = ok; d.has_data = false; CHECK(gftt_check_image(d, MI_8UC1, nullptr).code == MI_ERR_BAD_ARG);
    d = ok; d.rows = 0; CHECK(gftt_check_image(d, MI_8UC1, nullptr).code == MI_ERR_BAD_SIZE);
    d = {40, 140, MI_32FC1, 562, true}; CHECK(gftt_check_image(d, MI_32FC1, nullptr).code == MI_ERR_BAD_ARG);   // step no multiple of 4
    // overflow guards: 32767 is the last legal side, everything above is refused before any arithmetic on the area
    for (int side : {32768, 32769, 65536, 1 << 30, 2147483647}) {
        d = {side, 8, MI_8UC1, 8, true}; CHECK(gftt_check_image(d, MI_8UC1, nullptr).code == MI_ERR_BAD_SIZE);
        d = {8, side, MI_8UC1, (size_t)side, true}; CHECK(gftt_check_image(d, MI_8UC1, nullptr).code == MI_ERR_BAD_SIZE);
        CHECK(gftt_make_plan(side, 8, 3, 0).err.code == MI_ERR_BAD_SIZE && gftt_make_plan(8, side, 3, 0).err.code == MI_ERR_BAD_SIZE);
        CHECK(gftt_response_plan(side, side, 3, 0).err.code == MI_ERR_BAD_SIZE);
    }
    CHECK(gftt_make_plan(0, 8, 3, 0).err.code == MI_ERR_BAD_SIZE && gftt_make_plan(8, 8, 0, 0).err.code == MI_ERR_BAD_ARG);
    CHECK(gftt_make_plan(8, 8, 3, 3).err.code == MI_ERR_BAD_ARG);
}

static void check_min_distance()
{
    // three points on a row, 2 apart: with minDistance 3 the middle one goes, and then the third stays (it is 4 from the first)
    const float pts[] = {10, 10, 12, 10, 14, 10, 10, 12.5f, 200, 3};
    std::vector<float> out;
    gftt_min_distance(pts, 5, 40, 300, 3.0, 0, &out);
    CHECK(out.size() == 6 && out[0] == 10 && out[2] == 14 && out[4] == 200);   // (10, 12.5) is 2.5 from (10, 10)
    gftt_min_distance(pts, 5, 40, 300, 3.0, 2, &out);
    CHECK(out.size() == 4 && out[2] == 14);
    gftt_min_distance(pts, 5, 40, 300, 2.5, 0, &out);   // cvRound(2.5) = 2: ties to even; 2.5 is not < 2.5
    CHECK(out.size() == 8 && out[2] == 14 && out[4] == 10 && out[5] == 12.5f);
    gftt_min_distance(pts, 0, 40, 300, 3.0, 0, &out);
    CHECK(out.empty());
    CHECK(gftt_cv_round(0.5) == 0 && gftt_cv_round(1.5) == 2 && gftt_cv_round(2.5) == 2 && gftt_cv_round(7.5) == 8 && gftt_cv_round(1.0) == 1);
}

int main(int argc, char **argv)
{
    if (argc > 1 && !strcmp(argv[1], "constants")) {
        printf("%d %d %d %d %d %d %zu %d\n", GFTT_TILE_W, GFTT_TILE_H, GFTT_SEG, GFTT_FIND_SEGS, GFTT_SORT_TILE, GFTT_MAX_SIDE, GFTT_LDS_LIMIT,
               largest_fused());
        return 0;
    }
    check_validators();
    check_min_distance();
    const int big = largest_fused();
    CHECK(big >= 7 && gftt_fused_lds(big) <= GFTT_LDS_LIMIT && gftt_fused_lds(big + 1) > GFTT_LDS_LIMIT);
    const int hs[] = {1, 3, GFTT_TILE_H - 1, GFTT_TILE_H, GFTT_TILE_H + 1, 2 * GFTT_TILE_H, 2 * GFTT_TILE_H + 1, 480, 1080};
    const int ws[] = {1, 3, GFTT_TILE_W - 1, GFTT_TILE_W, GFTT_TILE_W + 1, 2 * GFTT_TILE_W, 2 * GFTT_TILE_W + 1, 640, 1920};
    for (int h : hs)
        for (int w : ws) {
            for (int bs : {1, 2, 3, 4, 5, 7, big - 1, big, big + 1, GFTT_MAX_BLOCK_SIZE})
                for (int form : {GFTT_FORM_AUTO, GFTT_FORM_FUSED, GFTT_FORM_PLANES}) check_response(h, w, bs, form);
            check_plan(h, w, 3);
            check_plan(h, w, big + 1);
        }
    // capacities: the floor of 1000, the first area above it, the sizes of the measurements, the largest legal frame
    CHECK(gftt_capacity(1, 1) == 1000 && gftt_capacity(100, 200) == 1000 && gftt_capacity(100, 201) == 1005);
    CHECK(gftt_capacity(480, 640) == 15360 && gftt_capacity(1080, 1920) == 103680 && gftt_capacity(2160, 3840) == 414720);
    CHECK(gftt_capacity(32767, 32767) == (int)(1073676289.0 * 0.05));
    check_plan(2160, 3840, 3);
    check_plan(32767, 32767, 3);
    check_plan(32767, 1, 3);
    check_plan(1, 32767, big + 1);
    const GfttPlan huge = gftt_make_plan(32767, 32767, 3, 0);
    CHECK(huge.sort_cap == 1 << 26 && huge.nseg == 32767 * 512 && huge.scratch_bytes > 4 * 1073676289ull);
    for (int cap : {GFTT_SORT_TILE, 2 * GFTT_SORT_TILE, 8 * GFTT_SORT_TILE})
        for (int count : {1, 2, 63, 1000, GFTT_SORT_TILE, GFTT_SORT_TILE + 1, cap - 1, cap})
            if (count <= cap) check_sort(cap, count);
    printf("gftt_plan_test: ok\n");
    return 0;
}
