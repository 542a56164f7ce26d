// The plan of StereoBeliefPropagation (csrc/sbp_plan.h) on the host: validator, level sizes, buffer alternation, the zeroed set, the
// launch order and the form rule, against the reference's host code restated here (stereobp.cpp:178-195, 234-359).  Plain C++, no device.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cmath>
#include "sbp_plan.h"

using namespace mi::sbp;

static int fails = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); ++fails; } } while (0)

static void check_plan(int rows, int cols, int ndisp, int iters, int levels, int msg_type, int cn)
{
    const SbpPlan p = sbp_make_plan(rows, cols, ndisp, iters, levels, msg_type, cn, 10.0f);
    CHECK(p.err.code == MI_OK);
    if (p.err.code) return;
    CHECK((int)p.lv.size() == levels && p.elem == (msg_type == SBP_MSG_32F ? 4 : 2));
    // level sizes (stereobp.cpp:316-317) and the set each level works in: mem_idx = (levels & 1) ? 0 : 1 at the coarsest level, then
    // alternating (:329-339)
    int r = rows, c = cols, mem_idx = (levels & 1) ? 0 : 1;
    int set_of[64];
    for (int i = levels - 1; i >= 0; --i) { set_of[i] = mem_idx; mem_idx = (mem_idx + 1) & 1; }
    size_t need[2] = {0, 0}, data_end = 0;
    for (int i = 0; i < levels; ++i) {
        if (i) { r = (r + 1) / 2; c = (c + 1) / 2; }
        const SbpLevel &L = p.lv[i];
        CHECK(L.rows == r && L.cols == c && L.set == set_of[i] && L.pitch >= c && L.pitch % 32 == 0);
        const size_t n = (size_t)ndisp * r * L.pitch;
        if (n > need[L.set]) need[L.set] = n;
        if (i || cn) { CHECK(L.data_off == data_end); data_end += n; }   // the data planes lie one behind the other, disjoint
    }
    CHECK(p.lv[0].set == 0);                         // output reads u_, d_, l_, r_ (:355)
    CHECK(p.zeroed_set == set_of[levels - 1]);       // :243-268: set 0 for odd levels, set 1 for even
    CHECK(p.zeroed_set == ((levels & 1) ? 0 : 1));
    CHECK(p.set_elems[0] == need[0] && p.set_elems[1] == need[1] && p.data_elems == data_end);
    // form rule
    const int cap = ndisp <= 16 ? 16 : ndisp <= 32 ? 32 : ndisp <= 64 ? 64 : 0;
    CHECK(p.form == (cap ? SBP_FORM_REG : SBP_FORM_GEN) && p.cap == cap);
    // launch order: comp_data, step_down 1 .. levels - 1, zero, then per level from the coarsest: [level_up] + iters iterations t = 0 ..
    size_t k = 0;
    const auto next = [&](int kernel, int level, int t) {
        CHECK(k < p.launches.size());
        if (k >= p.launches.size()) return;
        const SbpLaunch &l = p.launches[k++];
        CHECK(l.kernel == kernel && l.level == level && l.t == t);
        if (kernel == SBP_K_ITERATE) CHECK(l.form == p.form);
    };
    if (cn) next(SBP_K_COMP_DATA, 0, 0);
    for (int i = 1; i < levels; ++i) next(SBP_K_STEP_DOWN, i, 0);
    next(SBP_K_ZERO, levels - 1, 0);
    for (int i = levels - 1; i >= 0; --i) {
        if (i != levels - 1) next(SBP_K_LEVEL_UP, i, 0);
        for (int t = 0; t < iters; ++t) next(SBP_K_ITERATE, i, t);
    }
    next(SBP_K_OUTPUT, 0, 0);
    CHECK(k == p.launches.size());
}

int main()
{
    int n = 0;
    for (int levels = 1; levels <= 5; ++levels)
        for (int rows : {3 << (levels - 1), (3 << (levels - 1)) + 1, 67, 480})
            for (int cols : {3 << (levels - 1), 41, 131, 640})
                for (int ndisp : {1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 200})
                    for (int mt : {SBP_MSG_16S, SBP_MSG_32F})
                        for (int cn : {0, 1, 3, 4}) {
                            if (sbp_check_size(rows, cols, levels).code) continue;
                            check_plan(rows, cols, ndisp, 1 + levels % 3, levels, mt, cn);
                            ++n;
                        }
    CHECK(n == 7296);   // 7680 combinations less the shapes the size check rejects
    // form boundaries of the register form, and the forced forms
    CHECK(sbp_reg_cap(1) == 16 && sbp_reg_cap(16) == 16 && sbp_reg_cap(17) == 32 && sbp_reg_cap(32) == 32 && sbp_reg_cap(33) == 64 &&
          sbp_reg_cap(64) == 64 && sbp_reg_cap(65) == 0);
    CHECK(sbp_make_plan(24, 32, 64, 2, 2, SBP_MSG_32F, 1, 10.f, SBP_FORM_GEN).form == SBP_FORM_GEN);
    CHECK(sbp_make_plan(24, 32, 64, 2, 2, SBP_MSG_32F, 1, 10.f, SBP_FORM_GEN).cap == 0);
    CHECK(sbp_make_plan(24, 32, 64, 2, 2, SBP_MSG_32F, 1, 10.f, SBP_FORM_REG).cap == 64);
    CHECK(sbp_make_plan(24, 32, 65, 2, 2, SBP_MSG_32F, 1, 10.f, SBP_FORM_REG).err.code == MI_ERR_BAD_ARG);
    // the validator: one rejected case per assert, with the asserted condition as the text
    const auto rejected = [](const SbpPlan &p, int code, const char *text) { return p.err.code == code && p.launches.empty() && strstr(p.err.msg, text); };
    CHECK(rejected(sbp_make_plan(24, 32, 0, 2, 2, SBP_MSG_32F, 1, 10.f), MI_ERR_BAD_ARG, "0 < ndisp_"));
    CHECK(rejected(sbp_make_plan(24, 32, 8, 0, 2, SBP_MSG_32F, 1, 10.f), MI_ERR_BAD_ARG, "0 < iters_"));
    CHECK(rejected(sbp_make_plan(24, 32, 8, 2, 0, SBP_MSG_32F, 1, 10.f), MI_ERR_BAD_ARG, "0 < levels_"));
    CHECK(rejected(sbp_make_plan(24, 32, 8, 2, 2, 0, 1, 10.f), MI_ERR_BAD_ARG, "msg_type_ == CV_32F || msg_type_ == CV_16S"));
    CHECK(rejected(sbp_make_plan(24, 32, 8, 2, 3, SBP_MSG_16S, 1, 819.2f), MI_ERR_BAD_ARG, "numeric_limits<short>::max()"));   // 4 * 10 * 819.2 = 32768
    CHECK(sbp_make_plan(24, 32, 8, 2, 3, SBP_MSG_16S, 1, 819.0f).err.code == MI_OK);                                             // 32760
    CHECK(sbp_make_plan(24, 32, 8, 2, 3, SBP_MSG_32F, 1, 819.2f).err.code == MI_OK);                                             // the range condition binds 16-bit messages only
    CHECK(rejected(sbp_make_plan(24, 32, 8, 2, 2, SBP_MSG_32F, 2, 10.f), MI_ERR_BAD_TYPE, "left.type() == CV_8UC1"));
    CHECK(rejected(sbp_make_plan(24, 32, 8, 2, 5, SBP_MSG_32F, 1, 10.f), MI_ERR_BAD_SIZE, "min_image_dim_size"));               // 24 >> 4 = 1
    CHECK(sbp_make_plan(24, 32, 8, 2, 4, SBP_MSG_32F, 1, 10.f).err.code == MI_OK);                                               // 24 >> 3 = 3
    CHECK(rejected(sbp_make_plan(2, 32, 8, 2, 1, SBP_MSG_32F, 1, 10.f), MI_ERR_BAD_SIZE, "min_image_dim_size"));
    CHECK(rejected(sbp_make_plan(1 << 20, 1 << 20, 8, 2, 40, SBP_MSG_32F, 1, 10.f), MI_ERR_BAD_SIZE, "min_image_dim_size"));     // no shift by 39
    CHECK(rejected(sbp_make_plan(1 << 20, 1 << 20, 8, 2, 40, SBP_MSG_16S, 1, 0.f), MI_ERR_BAD_ARG, "numeric_limits<short>::max()"));
    // estimateRecommendedParams (stereobp.cpp:367-378)
    for (int w : {1, 3, 7, 100, 640, 1920, 4096})
        for (int h : {1, 2, 480, 1080, 5000}) {
            int nd, it, lv;
            sbp_estimate(w, h, std::log((double)(w > h ? w : h)), &nd, &it, &lv);
            int e_nd = w / 4; if (e_nd & 1) ++e_nd;
            const int mm = w > h ? w : h;
            int e_lv = (int)(std::log((double)mm) + 1) * 4 / 5; if (e_lv == 0) ++e_lv;
            CHECK(nd == e_nd && it == mm / 100 + 2 && lv == e_lv);
        }
    if (fails) { printf("sbp_plan_test: %d FAILED\n", fails); return 1; }
    printf("sbp_plan_test: ok (%d plans)\n", n);
    return 0;
}
