// The PLAN of StereoBeliefPropagation (stereobp_kernels.hip): the validator (the reference's asserts, stereobp.cpp:178-195 and
// :210-225), the level sizes, which of the two message sets a level works in and which set starts from zero, the form of the
// iteration kernel, the scratch layout and the ordered launch list.  compute() only EXECUTES the list.  Pure arithmetic, no HIP types.
#pragma once
#include <cstddef>
#include <vector>
#include "miflow/c_api.h"

namespace mi {
namespace sbp {

constexpr int SBP_MSG_16S = 3, SBP_MSG_32F = 5;   // CV_16S, CV_32F: the depth codes msg_type takes (cudastereo.hpp:189)

// Forms of the iteration kernel.  REG: a lane keeps the four new messages of its pixel (4 x capacity values) in registers from the
// first sum to the final subtraction and writes each value once; capacities 16 / 32 / 64, the smallest that holds ndisp.  GEN: any
// ndisp >= 1, the message lives in global memory between its passes as in the reference (stereobp.cu:389-426).
enum { SBP_FORM_AUTO = 0, SBP_FORM_REG = 1, SBP_FORM_GEN = 2 };
constexpr int SBP_REG_CAPS[3] = {16, 32, 64};
constexpr int SBP_REG_MAX = 64;   // 4 x 64 values + addresses stay inside the 512 VGPRs of a lone wave per SIMD
inline int sbp_reg_cap(int ndisp)
{
    for (int c : SBP_REG_CAPS) if (ndisp <= c) return c;
    return 0;   // the register form does not take this ndisp
}

enum SbpKernel {
    SBP_K_COMP_DATA = 0,   // k_sbp_comp_data    images -> data cost of level 0 (interior pixels)
    SBP_K_STEP_DOWN,       // k_sbp_step_down    data cost of level - 1 -> level
    SBP_K_ZERO,            // memset             the four messages of the coarsest level := 0
    SBP_K_LEVEL_UP,        // k_sbp_level_up     the four messages of level + 1 (other set) -> level
    SBP_K_ITERATE,         // k_sbp_iterate_reg / _gen   one checkerboard half-sweep, parity t
    SBP_K_OUTPUT           // k_sbp_output       winner per pixel, border 0, in the caller's disparity type
};

struct SbpErr { int code; const char *msg; };
struct SbpLevel {
    int rows, cols;
    int pitch;            // elements per row of the level's message and data planes
    int set;              // message set the level iterates in: 0 = full size, 1 = half size (stereobp.cpp:329-339)
    size_t data_off;      // element offset of the level's data cost in the data scratch (level 0 of compute_data: the caller's matrix)
};
struct SbpLaunch { int kernel, level, t, form; };
struct SbpPlan {
    SbpErr err;           // the validator's verdict; nothing below is set when it rejects
    int rows, cols, ndisp, iters, levels, msg_type, channels;
    int elem;             // sizeof(T)
    int form, cap;        // SBP_FORM_REG with its capacity, or SBP_FORM_GEN (cap 0)
    int zeroed_set;       // = the coarsest level's set (stereobp.cpp:243-268)
    std::vector<SbpLevel> lv;
    size_t set_elems[2];  // elements of ONE message (u) of each set; a set holds u, d, l, r one behind the other
    size_t data_elems;    // elements of the data pyramid
    std::vector<SbpLaunch> launches;
};

inline int sbp_align(int n, int a) { return (n + a - 1) / a * a; }

// stereobp.cpp:178-180 = :210-212
inline SbpErr sbp_check_params(int ndisp, int iters, int levels, int msg_type, float max_data_term)
{
    if (!(0 < ndisp && 0 < iters && 0 < levels)) return {MI_ERR_BAD_ARG, "0 < ndisp_ && 0 < iters_ && 0 < levels_"};
    if (!(msg_type == SBP_MSG_32F || msg_type == SBP_MSG_16S)) return {MI_ERR_BAD_ARG, "msg_type_ == CV_32F || msg_type_ == CV_16S"};
    if (msg_type == SBP_MSG_16S) {
        const float scale = 10.0f;
        // (1 << (levels - 1)) is an int in the reference; from 32 levels on the shift is undefined there and rejected here
        if (levels > 31 || !((float)(1 << (levels - 1)) * scale * max_data_term < 32767.0f))
            return {MI_ERR_BAD_ARG, "msg_type_ == CV_32F || (1 << (levels_ - 1)) * scale_ * max_data_term_ < std::numeric_limits<short>::max()"};
    }
    return {MI_OK, nullptr};
}
// stereobp.cpp:191-195 = :221-225: divisor = (int) pow(2.f, levels - 1)
inline SbpErr sbp_check_size(int rows, int cols, int levels)
{
    const int m = rows < cols ? rows : cols;
    const int lowest = levels - 1 >= 31 ? 0 : m >> (levels - 1);
    if (!(lowest > 2)) return {MI_ERR_BAD_SIZE, "std::min(lowest_cols, lowest_rows) > min_image_dim_size"};
    return {MI_OK, nullptr};
}

// form: SBP_FORM_AUTO (the rule), or one of the two forced (stage tests); a forced REG with ndisp beyond its capacities is rejected.
// channels: 1 / 3 / 4 for compute(left, right), 0 for compute(data): no comp_data launch, level 0 reads the caller's cost volume.
inline SbpPlan sbp_make_plan(int rows, int cols, int ndisp, int iters, int levels, int msg_type, int channels, float max_data_term,
                             int form = SBP_FORM_AUTO)
{
    SbpPlan p = {};
    if ((p.err = sbp_check_params(ndisp, iters, levels, msg_type, max_data_term)).code) return p;
    if (!(channels == 0 || channels == 1 || channels == 3 || channels == 4)) {
        p.err = {MI_ERR_BAD_TYPE, "left.type() == CV_8UC1 || left.type() == CV_8UC3 || left.type() == CV_8UC4"};
        return p;
    }
    if ((p.err = sbp_check_size(rows, cols, levels)).code) return p;
    const int cap = sbp_reg_cap(ndisp);
    if (form == SBP_FORM_AUTO) form = cap ? SBP_FORM_REG : SBP_FORM_GEN;
    if (!(form == SBP_FORM_GEN || (form == SBP_FORM_REG && cap))) {
        p.err = {MI_ERR_BAD_ARG, "form: the register form holds at most 64 disparities"};
        return p;
    }
    p.rows = rows; p.cols = cols; p.ndisp = ndisp; p.iters = iters; p.levels = levels; p.msg_type = msg_type; p.channels = channels;
    p.elem = msg_type == SBP_MSG_32F ? 4 : 2;
    p.form = form; p.cap = form == SBP_FORM_REG ? cap : 0;
    p.lv.resize(levels);
    p.set_elems[0] = p.set_elems[1] = 0;
    size_t off = 0;
    for (int i = 0; i < levels; ++i) {
        SbpLevel &L = p.lv[i];
        L.rows = i ? (p.lv[i - 1].rows + 1) / 2 : rows;   // stereobp.cpp:316-317
        L.cols = i ? (p.lv[i - 1].cols + 1) / 2 : cols;
        L.pitch = sbp_align(L.cols, 32);
        L.set = i & 1;   // mem_idx starts at (levels & 1) ? 0 : 1 for level levels - 1 and alternates: level 0 always lands in set 0
        const size_t n = (size_t)ndisp * L.rows * L.pitch;
        if (n > p.set_elems[L.set]) p.set_elems[L.set] = n;
        L.data_off = off;
        if (i || channels) off += n;
    }
    p.data_elems = off;
    p.zeroed_set = p.lv[levels - 1].set;
    if (channels) p.launches.push_back({SBP_K_COMP_DATA, 0, 0, 0});
    for (int i = 1; i < levels; ++i) p.launches.push_back({SBP_K_STEP_DOWN, i, 0, 0});
    p.launches.push_back({SBP_K_ZERO, levels - 1, 0, 0});
    for (int i = levels - 1; i >= 0; --i) {
        if (i != levels - 1) p.launches.push_back({SBP_K_LEVEL_UP, i, 0, 0});
        for (int t = 0; t < iters; ++t) p.launches.push_back({SBP_K_ITERATE, i, t, form});   // t restarts at every level (stereobp.cu:464)
    }
    p.launches.push_back({SBP_K_OUTPUT, 0, 0, 0});
    return p;
}

// StereoBeliefPropagation::estimateRecommendedParams, stereobp.cpp:367-378; log_mm = log((double)max(width, height))
inline void sbp_estimate(int width, int height, double log_mm, int *ndisp, int *iters, int *levels)
{
    *ndisp = width / 4;
    if ((*ndisp & 1) != 0) ++*ndisp;
    const int mm = width > height ? width : height;
    *iters = mm / 100 + 2;
    *levels = (int)(log_mm + 1) * 4 / 5;
    if (*levels == 0) ++*levels;
}

}  // namespace sbp
}  // namespace mi
