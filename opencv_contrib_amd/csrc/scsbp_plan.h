// The PLAN of StereoConstantSpaceBP (stereocsbp_kernels.hip): the validator (the reference's asserts in its order, stereocsbp.cpp:154-161,
// and the clamp of :171), the level sizes and planes per level (:179-188), which of the two message / disparity sets a level works in
// (:238-264), what is zeroed, the form and capacity of each level's iteration kernel, the scratch layout and the ordered launch list.
// compute() only EXECUTES the list.  Pure arithmetic, no HIP types.
#pragma once
#include <cmath>
#include <cstddef>
#include <vector>
#include "miflow/c_api.h"

namespace mi {
namespace scsbp {

constexpr int CSBP_MSG_16S = 3, CSBP_MSG_32F = 5;   // CV_16S, CV_32F
constexpr int CSBP_MAX_LEVELS = 8;                  // stereocsbp.cpp:155; the data-cost table of stereocsbp.cu:314-319 ends at 2^8

// Forms of the iteration kernel.  REG: the candidates' sums, their disparities and the new message of a pixel stay in registers (the
// sums and disparities) and in a lane-private LDS column (the new message) from the first sum to the final subtraction; capacities
// 4 .. 64, the smallest power of two that holds the level's planes.  GEN: any number of planes, the message and the reference's temp
// plane live in global memory between the passes (stereocsbp.cu:656-690).
enum { CSBP_FORM_AUTO = 0, CSBP_FORM_REG = 1, CSBP_FORM_GEN = 2 };
constexpr int CSBP_REG_CAPS[5] = {4, 8, 16, 32, 64};
constexpr int CSBP_REG_MAX = 64;
inline int csbp_reg_cap(int planes)
{
    for (int c : CSBP_REG_CAPS) if (planes <= c) return c;
    return 0;   // the register form does not take this many planes
}

enum CsbpKernel {
    CSBP_K_ZERO = 0,        // memset            both sets := 0, whole (see CsbpPlan::set_elems)
    CSBP_K_INIT_DATA_COST,  // k_csbp_data_cost  images -> ndisp cost planes of the coarsest level in the scratch
    CSBP_K_FIRST_K,         // k_csbp_first_k    scratch -> the level's planes cheapest disparities and their costs
    CSBP_K_COMP_DATA_COST,  // k_csbp_data_cost  images + the parents' candidates -> data_cost (2 x planes of the level)
    CSBP_K_INIT_MESSAGE,    // k_csbp_init_message   + the parents' messages -> the level's candidates, costs and messages (other set)
    CSBP_K_ITERATE,         // k_csbp_message_reg / _gen   one checkerboard half-sweep, parity t & 1
    CSBP_K_DISP             // k_csbp_disp       winner per pixel, border 0, in the caller's disparity type
};

struct CsbpErr { int code; const char *msg; };
struct CsbpLevel {
    int rows, cols;
    int pitch;        // elements per row of every plane of the level: ONE pitch for all levels, as in the reference
    int planes;       // nr_plane << level
    int set;          // message / disparity set the level works in
    int form, cap;    // of its iteration kernel
};
struct CsbpLaunch { int kernel, level, t, form; };
struct CsbpPlan {
    CsbpErr err;          // the validator's verdict; nothing below is set when it rejects
    int rows, cols, ndisp, iters, levels, nr_plane, msg_type, channels, local;
    int elem;             // sizeof(T)
    std::vector<CsbpLevel> lv;
    // Elements of ONE member (u) of each set; a set holds u, d, l, r, disp_selected one behind the other.  Every member is the
    // reference's (rows * nr_plane) x cols matrix (stereocsbp.cpp:196-212) and plane k of a level starts at row k * level rows, as there:
    // at a level with an odd number of rows or columns the last row / column has no parent (y / 2 == the parent's rows), and the
    // reference reads on into the next plane, or past the level's planes into what a coarser level of the same set left there, or into
    // memory nothing wrote.  With the reference's addressing and both sets zeroed whole at the start of every compute those reads are
    // defined and equal the reference run on zero-initialised memory.
    size_t set_elems[2];
    size_t cost_elems;    // data_cost: the 2 x planes candidates' costs of the finer levels
    size_t sel_elems;     // data_cost_selected
    size_t temp_elems;    // scratch: ndisp planes of the coarsest level, the summed costs of init_message, the general form's temp
    std::vector<CsbpLaunch> launches;
};

inline int csbp_align(int n, int a) { return (n + a - 1) / a * a; }

// stereocsbp.cpp:154-155, then :171.  -> the clamped level count in *levels
inline CsbpErr csbp_check_params(int ndisp, int iters, int *levels, int nr_plane, int msg_type)
{
    if (!(msg_type == CSBP_MSG_32F || msg_type == CSBP_MSG_16S)) return {MI_ERR_BAD_ARG, "msg_type_ == CV_32F || msg_type_ == CV_16S"};
    if (!(0 < ndisp && 0 < iters && 0 < *levels && 0 < nr_plane && *levels <= CSBP_MAX_LEVELS))
        return {MI_ERR_BAD_ARG, "0 < ndisp_ && 0 < iters_ && 0 < levels_ && 0 < nr_plane_ && levels_ <= 8"};
    const int by_ndisp = (int)(std::log((double)ndisp) / std::log(2.0));
    if (by_ndisp < *levels) *levels = by_ndisp;
    if (*levels < 1)
        return {MI_ERR_BAD_ARG, "ndisp == 1: levels_ = min(levels_, int(log(ndisp_) / log(2.0))) is 0, which is undefined in the reference"};
    return {MI_OK, nullptr};
}

// form: CSBP_FORM_AUTO (the rule), or one of the two forced; a forced REG falls back to GEN on the levels it cannot hold.
inline CsbpPlan csbp_make_plan(int rows, int cols, int channels, int ndisp, int iters, int levels, int nr_plane, int msg_type, int local,
                               int form = CSBP_FORM_AUTO)
{
    CsbpPlan p = {};
    if ((p.err = csbp_check_params(ndisp, iters, &levels, nr_plane, msg_type)).code) return p;
    if (!(channels == 1 || channels == 3 || channels == 4)) {
        p.err = {MI_ERR_BAD_TYPE, "left.type() == CV_8UC1 || left.type() == CV_8UC3 || left.type() == CV_8UC4"};
        return p;
    }
    if (!(rows > 0 && cols > 0)) { p.err = {MI_ERR_BAD_SIZE, "empty image"}; return p; }
    if ((rows >> (levels - 1)) < 1 || (cols >> (levels - 1)) < 1) {
        p.err = {MI_ERR_BAD_SIZE, "the coarsest level is empty: an empty launch, which is undefined in the reference"};
        return p;
    }
    if ((long long)nr_plane << (levels - 1) > (1 << 24)) { p.err = {MI_ERR_BAD_ARG, "nr_plane << (levels - 1) is too large"}; return p; }
    if (!(form == CSBP_FORM_AUTO || form == CSBP_FORM_REG || form == CSBP_FORM_GEN)) { p.err = {MI_ERR_BAD_ARG, "form"}; return p; }
    p.rows = rows; p.cols = cols; p.ndisp = ndisp; p.iters = iters; p.levels = levels; p.nr_plane = nr_plane; p.msg_type = msg_type;
    p.channels = channels; p.local = local ? 1 : 0;
    p.elem = msg_type == CSBP_MSG_32F ? 4 : 2;
    p.lv.resize(levels);
    p.set_elems[0] = p.set_elems[1] = 0;
    p.cost_elems = p.sel_elems = p.temp_elems = 0;
    const auto grow = [](size_t &a, size_t b) { if (b > a) a = b; };
    for (int i = 0; i < levels; ++i) {
        CsbpLevel &L = p.lv[i];
        L.rows = i ? p.lv[i - 1].rows / 2 : rows;   // stereocsbp.cpp:183-188
        L.cols = i ? p.lv[i - 1].cols / 2 : cols;
        L.planes = i ? p.lv[i - 1].planes * 2 : nr_plane;
        L.pitch = csbp_align(cols, 32);
        L.set = (levels - 1 - i) & 1;   // cur_idx = 0 at the coarsest level, flipped by every init_message (:238, :254-263)
        L.cap = csbp_reg_cap(L.planes);
        L.form = form == CSBP_FORM_GEN || !L.cap ? CSBP_FORM_GEN : CSBP_FORM_REG;
        if (L.form == CSBP_FORM_GEN) L.cap = 0;
    }
    for (int i = 0; i < levels; ++i) {
        const CsbpLevel &L = p.lv[i];
        const size_t px = (size_t)L.rows * L.pitch;
        grow(p.sel_elems, px * L.planes);
        if (L.form == CSBP_FORM_GEN) grow(p.temp_elems, px * L.planes);
        if (i == levels - 1) grow(p.temp_elems, px * ndisp);
        else { grow(p.cost_elems, px * L.planes * 2); grow(p.temp_elems, px * L.planes * 2); }
    }
    p.set_elems[0] = p.set_elems[1] = (size_t)rows * nr_plane * p.lv[0].pitch;
    p.launches.push_back({CSBP_K_ZERO, levels - 1, 0, 0});
    for (int i = levels - 1; i >= 0; --i) {
        if (i == levels - 1) {
            p.launches.push_back({CSBP_K_INIT_DATA_COST, i, 0, 0});
            p.launches.push_back({CSBP_K_FIRST_K, i, 0, 0});
        } else {
            p.launches.push_back({CSBP_K_COMP_DATA_COST, i, 0, 0});
            p.launches.push_back({CSBP_K_INIT_MESSAGE, i, 0, 0});
        }
        for (int t = 0; t < iters; ++t) p.launches.push_back({CSBP_K_ITERATE, i, t, p.lv[i].form});   // t restarts at every level (stereocsbp.cu:731)
    }
    p.launches.push_back({CSBP_K_DISP, 0, 0, 0});
    return p;
}

// StereoConstantSpaceBP::estimateRecommendedParams, stereocsbp.cpp:342-355
inline void csbp_estimate(int width, int height, int *ndisp, int *iters, int *levels, int *nr_plane)
{
    *ndisp = (int)((float)width / 3.14f);
    if ((*ndisp & 1) != 0) ++*ndisp;
    const int mm = width > height ? width : height;
    *iters = mm / 100 + ((mm > 1200) ? -4 : 4);
    *levels = (int)std::log((double)mm) * 2 / 3;
    if (*levels == 0) ++*levels;
    *nr_plane = (int)((float)*ndisp / std::pow(2.0, *levels + 1));
}

}  // namespace scsbp
}  // namespace mi
