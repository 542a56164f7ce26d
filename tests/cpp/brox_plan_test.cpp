// The host plan of cv::cuda::BroxOpticalFlow (opencv_contrib_amd/csrc/brox_plan.h), checked without a GPU.  A stand-alone program:
//   brox_plan_test                       the self-test: validation, level sizes, the scratch layout, the launch list of both forms
//   brox_plan_test constants             the numbers the Python tests read from the header
//   brox_plan_test levels W H SF OUTER   the level sizes "w h" per line, level 0 first
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include "brox_plan.h"

using namespace mi::brox;

#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

static mi_brox_params defaults() { return {0.197f, 50.0f, 0.8f, 5, 150, 10}; }

static int count(const BroxPlan &p, int kernel, int level = -1)
{
    int n = 0;
    for (const BroxLaunch &k : p.launches) n += k.kernel == kernel && (level < 0 || k.level == level);
    return n;
}

static int self_test()
{
    // validation: NCVBroxOpticalFlow.cu:606-610 and the scale factor
    mi_brox_params p = defaults();
    CHECK(brox_check_params(p).code == MI_OK);
    { mi_brox_params q = p; q.alpha = 0.f; CHECK(brox_check_params(q).code == MI_ERR_BAD_ARG); q.alpha = -1.f; CHECK(brox_check_params(q).code == MI_ERR_BAD_ARG); }
    { mi_brox_params q = p; q.alpha = NAN; CHECK(brox_check_params(q).code == MI_ERR_BAD_ARG); }
    { mi_brox_params q = p; q.gamma = -0.5f; CHECK(brox_check_params(q).code == MI_ERR_BAD_ARG); q.gamma = 0.f; CHECK(brox_check_params(q).code == MI_OK); }
    { mi_brox_params q = p; q.scale_factor = 0.f; CHECK(brox_check_params(q).code == MI_ERR_BAD_ARG); q.scale_factor = 1.f; CHECK(brox_check_params(q).code == MI_ERR_BAD_ARG); }
    { mi_brox_params q = p; q.inner_iterations = 0; CHECK(brox_check_params(q).code == MI_ERR_BAD_ARG); }
    { mi_brox_params q = p; q.outer_iterations = 0; CHECK(brox_check_params(q).code == MI_ERR_BAD_ARG); }
    { mi_brox_params q = p; q.solver_iterations = -3; CHECK(brox_check_params(q).code == MI_ERR_BAD_ARG); }
    CHECK(brox_check_size(4, 4).code == MI_OK && brox_check_size(3, 9).code == MI_ERR_BAD_ARG && brox_check_size(9, 3).code == MI_ERR_BAD_ARG);
    CHECK(brox_check_size(32768, 8).code == MI_ERR_BAD_SIZE);
    CHECK(brox_make_plan(3, 9, p, 0).err.code == MI_ERR_BAD_ARG && brox_make_plan(3, 9, p, 0).launches.empty());

    // a level with a side of 1 is refused (the filter's mirror maps -2 -> 3 -> -2 there); sides of 2 and 3 are planned
    { mi_brox_params q = p; q.scale_factor = 0.05f; const BroxPlan bad = brox_make_plan(16, 16, q, 0); CHECK(bad.err.code == MI_ERR_BAD_ARG && bad.launches.empty()); }
    { mi_brox_params q = p; q.scale_factor = 0.0625f; CHECK(brox_make_plan(16, 16, q, 0).err.code == MI_ERR_BAD_ARG); }
    { mi_brox_params q = p; q.scale_factor = 0.07f; const BroxPlan ok = brox_make_plan(16, 16, q, 0); CHECK(ok.err.code == MI_OK && ok.levels.size() == 2 && ok.levels[1].w == 2); }
    { mi_brox_params q = p; q.scale_factor = 0.15f; const BroxPlan ok = brox_make_plan(16, 16, q, 0); CHECK(ok.err.code == MI_OK && ok.levels[1].w == 3 && ok.levels[1].h == 3); }
    { mi_brox_params q = p; q.scale_factor = 0.06f; CHECK(brox_make_plan(16, 400, q, 0).err.code == MI_ERR_BAD_ARG && brox_make_plan(400, 16, q, 0).err.code == MI_ERR_BAD_ARG); }
    for (int n = 2; n <= 3; ++n)   // the kernel's mirror (k_brox_deriv) on the four out-of-range indices stays inside such a side
        for (int i : {-2, -1, n, n + 1}) { int j = i; if (j < 0) j = 1 - j; if (j >= n) j = n + n - j - 1; CHECK(j >= 0 && j < n); }

    // level sizes: the 15-pixel rule, the cut by outer_iterations, one level below 16
    std::vector<int> ws, hs;
    brox_level_sizes(16, 16, 0.8f, 150, &ws, &hs);
    CHECK(ws.size() == 2 && ws[1] == 13 && hs[1] == 13);              // 13 is not above 15: no third level
    brox_level_sizes(15, 400, 0.8f, 150, &ws, &hs);
    CHECK(ws.size() == 1);
    brox_level_sizes(640, 480, 0.8f, 3, &ws, &hs);
    CHECK(ws.size() == 3 && ws[1] == 512 && hs[1] == 384 && ws[2] == 410 && hs[2] == 308);   // ceilf(640 * 0.64f) = 410
    brox_level_sizes(640, 480, 0.8f, 1, &ws, &hs);
    CHECK(ws.size() == 1);
    brox_level_sizes(640, 480, 0.8f, 150, &ws, &hs);
    CHECK(ws.size() >= 16 && hs.back() <= 15 + 4 && hs[hs.size() - 2] > 15);
    for (size_t l = 1; l < ws.size(); ++l) CHECK(brox_resize_down_fits(ws[l - 1], ws[l], 0.8f) && brox_resize_down_fits(hs[l - 1], hs[l], 0.8f));
    CHECK(!brox_resize_down_fits(8, 8, 0.5f) && brox_resize_down_fits(8, 4, 0.5f));

    // the scratch layout: 22 level-0 planes, then two planes per level above 0; aligned, disjoint, inside scratch_bytes
    for (int form = BROX_FORM_PLAIN; form <= BROX_FORM_BLOCKED; ++form) {
        const int rows = 70, cols = 37;
        p = defaults(); p.inner_iterations = 2; p.solver_iterations = 5;
        const BroxPlan plan = brox_make_plan(rows, cols, p, form);
        CHECK(plan.err.code == MI_OK);
        const int n = (int)plan.levels.size();
        CHECK(n == 6 && plan.levels[0].w == cols && plan.levels[0].h == rows);
        const size_t plane0 = brox_plane(cols, rows);
        CHECK(plane0 % BROX_PLANE_ALIGN == 0 && plane0 >= (size_t)brox_ld(cols) * rows && brox_ld(cols) == 48);
        std::set<size_t> starts;
        size_t end = 0;
        for (int s = 0; s < S_COUNT; ++s) { CHECK(plan.off_slot[s] == (size_t)s * plane0); starts.insert(plan.off_slot[s]); end = plan.off_slot[s] + plane0; }
        for (int l = 1; l < n; ++l) {
            const BroxLevel &L = plan.levels[l];
            CHECK(L.ld == brox_ld(L.w) && L.ld % BROX_LD_ALIGN == 0 && L.w < plan.levels[l - 1].w);
            CHECK(L.off_i0 == end); end += brox_plane(L.w, L.h);
            CHECK(L.off_i1 == end); end += brox_plane(L.w, L.h);
            CHECK(L.off_i0 % BROX_PLANE_ALIGN == 0 && L.off_i1 % BROX_PLANE_ALIGN == 0);
        }
        CHECK(plan.scratch_bytes == end * sizeof(float));

        // the launch list: pyramid down, zero u / v once, then per level coarse to fine: zero, two derivative launches, per inner
        // iteration two prepares and the solver, then the prolongation or, at level 0, the output
        CHECK(plan.launches[0].kernel == BROX_K_RESIZE_DOWN && plan.launches[0].level == 1 && plan.launches[0].gz == 2);
        CHECK(count(plan, BROX_K_RESIZE_DOWN) == n - 1 && count(plan, BROX_K_RESIZE_UP) == n - 1 && count(plan, BROX_K_ADD_OUT) == 1);
        CHECK(count(plan, BROX_K_ZERO) == n + 1 && count(plan, BROX_K_DERIV1) == n && count(plan, BROX_K_DERIV2) == n);
        CHECK(count(plan, BROX_K_PREPARE1) == n * 2 && count(plan, BROX_K_PREPARE2) == n * 2);
        CHECK(plan.launches.back().kernel == BROX_K_ADD_OUT && plan.launches.back().level == 0);
        const int per_system = form == BROX_FORM_PLAIN ? 2 * 5 : 3;   // blocked: 2 + 2 + 1 iterations
        CHECK(plan.sor_launches == n * 2 * per_system);
        CHECK(count(plan, form == BROX_FORM_PLAIN ? BROX_K_SOR_PLAIN : BROX_K_SOR_BLOCKED) == plan.sor_launches);
        CHECK(count(plan, form == BROX_FORM_PLAIN ? BROX_K_SOR_BLOCKED : BROX_K_SOR_PLAIN) == 0);
        int last_level = n, sum = 0;
        for (const BroxLaunch &k : plan.launches) {
            if (k.kernel == BROX_K_RESIZE_DOWN) continue;
            if (k.kernel != BROX_K_RESIZE_UP) { CHECK(k.level <= last_level); last_level = k.level; }
            const BroxLevel &L = plan.levels[k.level];
            if (k.kernel == BROX_K_SOR_BLOCKED) {
                CHECK(k.gx == brox_div_up(L.w, BROX_SOR_TILE_X) && k.gy == brox_div_up(L.h, BROX_SOR_TILE_Y) && k.threads == BROX_SOR_THREADS);
                CHECK(k.arg >= 1 && k.arg <= BROX_SOR_KMAX);
                if (k.level == 0) sum += k.arg;
            } else {
                CHECK(k.gx == brox_div_up(L.w, BROX_BLOCK_X) && k.gy == brox_div_up(L.h, BROX_BLOCK_Y) && k.threads == 256);
                if (k.kernel == BROX_K_SOR_PLAIN) CHECK(k.arg == 0 || k.arg == 1);
            }
        }
        if (form == BROX_FORM_BLOCKED) CHECK(sum == 2 * 5);   // every solver iteration of level 0 runs exactly once
        // a plain solver alternates its colours, black first
        if (form == BROX_FORM_PLAIN) {
            int expect = 0;
            for (const BroxLaunch &k : plan.launches) if (k.kernel == BROX_K_SOR_PLAIN) { CHECK(k.arg == expect); expect ^= 1; }
        }
    }
    // the selection rule: explicit forms pass through, AUTO follows BROX_BLOCKED_MIN_SIDE
    CHECK(brox_sor_form(640, 480, BROX_FORM_PLAIN) == BROX_FORM_PLAIN && brox_sor_form(4, 4, BROX_FORM_BLOCKED) == BROX_FORM_BLOCKED);
    for (int side : {4, 16, 640, 32767}) {
        const int want = side >= BROX_BLOCKED_MIN_SIDE ? BROX_FORM_BLOCKED : BROX_FORM_PLAIN;
        CHECK(brox_sor_form(side, side, BROX_FORM_AUTO) == want && brox_sor_form(32767, side, BROX_FORM_AUTO) == want);
    }
    CHECK(BROX_SOR_HALO == 2 * BROX_SOR_KMAX && BROX_SOR_LDS_X == BROX_SOR_TILE_X + 2 * BROX_SOR_HALO);
    CHECK(6 * BROX_SOR_LDS_X * BROX_SOR_LDS_Y * sizeof(float) <= 64 * 1024);   // the blocked kernel's six LDS tiles
    std::printf("brox_plan_test: ok\n");
    return 0;
}

int main(int argc, char **argv)
{
    if (argc == 2 && !std::strcmp(argv[1], "constants")) {
        std::printf("%d %d %d %d %d %d\n", (int)BROX_SOR_TILE_X, (int)BROX_SOR_TILE_Y, (int)BROX_SOR_KMAX, (int)BROX_SOR_HALO, (int)BROX_MIN_SIDE, (int)S_COUNT);
        return 0;
    }
    if (argc == 6 && !std::strcmp(argv[1], "levels")) {
        std::vector<int> ws, hs;
        brox_level_sizes(std::atoi(argv[2]), std::atoi(argv[3]), (float)std::atof(argv[4]), std::atoi(argv[5]), &ws, &hs);
        for (size_t l = 0; l < ws.size(); ++l) std::printf("%d %d\n", ws[l], hs[l]);
        return 0;
    }
    return self_test();
}
