// cv::cuda::BroxOpticalFlow: the pure host plan.  No HIP in here: tests/cpp/brox_plan_test.cpp compiles it with the host compiler.
// It answers three questions for one calc: which pyramid levels exist (NCVBroxOpticalFlow.cu:698-785), where every plane lies in the
// handle's scratch, and which launches run in which order.  brox_api.cpp only walks the list.
#pragma once
#include <cmath>
#include <cstddef>
#include <vector>
#include "miflow/c_api.h"

namespace mi {
namespace brox {

struct BroxErr { int code; const char *msg; };

enum { BROX_MIN_SIDE = 4,      // the derivative filter's mirror (NPP_staging.cu:1433-1446) reads index 3 for -2: 4 is the smallest side
       BROX_MIN_LEVEL_SIDE = 2,   // of a level above 0: the mirror's second step brings 3 back inside a side of 2 or 3 (as in the
                                  // reference), but with a side of 1 it maps -2 -> 3 -> -2 and leaves the plane: such a pyramid is refused
       BROX_LD_ALIGN = 16,     // floats: every row of a scratch plane starts on 64 bytes
       BROX_PLANE_ALIGN = 64,  // floats: every plane starts on 256 bytes
       BROX_BLOCK_X = 64, BROX_BLOCK_Y = 4,   // pointwise / stencil kernels: one wave per row segment
       BROX_SOR_KMAX = 2,      // solver iterations one launch of the blocked form runs at most
       BROX_SOR_TILE_X = 64, BROX_SOR_TILE_Y = 16, BROX_SOR_HALO = 2 * BROX_SOR_KMAX,
       BROX_SOR_LDS_X = BROX_SOR_TILE_X + 2 * BROX_SOR_HALO, BROX_SOR_LDS_Y = BROX_SOR_TILE_Y + 2 * BROX_SOR_HALO,
       BROX_SOR_THREADS = 256 };
enum { BROX_FORM_AUTO = 0, BROX_FORM_PLAIN = 1, BROX_FORM_BLOCKED = 2 };

// NCVBroxOpticalFlow.cu:606-610, and 0 < scale_factor < 1 (at 1 the pyramid would repeat the frame outer_iterations times)
inline BroxErr brox_check_params(const mi_brox_params &p)
{
    if (!(p.alpha > 0.f)) return {MI_ERR_BAD_ARG, "alpha > 0"};
    if (!(p.gamma >= 0.f)) return {MI_ERR_BAD_ARG, "gamma >= 0"};
    if (!(p.scale_factor > 0.f && p.scale_factor < 1.f)) return {MI_ERR_BAD_ARG, "0 < scale_factor < 1"};
    if (p.inner_iterations <= 0) return {MI_ERR_BAD_ARG, "inner_iterations > 0"};
    if (p.outer_iterations <= 0) return {MI_ERR_BAD_ARG, "outer_iterations > 0"};
    if (p.solver_iterations <= 0) return {MI_ERR_BAD_ARG, "solver_iterations > 0"};
    return {MI_OK, ""};
}

inline BroxErr brox_check_size(int rows, int cols)
{
    if (rows < BROX_MIN_SIDE || cols < BROX_MIN_SIDE) return {MI_ERR_BAD_ARG, "a frame narrower or lower than 4 is outside the derivative filter's mirror"};
    if (rows > 32767 || cols > 32767) return {MI_ERR_BAD_SIZE, "rows and cols are at most 32767"};
    return {MI_OK, ""};
}

struct BroxLevel { int w, h, ld; size_t off_i0, off_i1; };   // offsets in floats; level 0 is the caller's two frames, read in place

// NCVBroxOpticalFlow.cu:698-785: scale is a binary32 product; a level's size comes from the SOURCE size; levels are added while the
// previous one is wider and higher than 15 and fewer than outer_iterations exist
inline void brox_level_sizes(int w, int h, float scale_factor, int outer_iterations, std::vector<int> *ws, std::vector<int> *hs)
{
    ws->assign(1, w); hs->assign(1, h);
    float scale = 1.0f;
    scale *= scale_factor;
    int pw = w, ph = h;
    while (pw > 15 && ph > 15 && (int)ws->size() < outer_iterations) {
        const int lw = (int)ceilf((float)w * scale), lh = (int)ceilf((float)h * scale);
        ws->push_back(lw); hs->push_back(lh);
        scale *= scale_factor;
        pw = lw; ph = lh;
    }
}

// resizeSuperSample_32f (NPP_staging.cu:2073-2149) reads source indices up to max(floor(begin) + 1, ceil(end)) of its last output's
// window (processLine reads its last tap even where the window is one sample): true where that stays inside a side of `src` samples
inline bool brox_resize_down_fits(int src, int dst, float scale_factor)
{
    const float s = 1.0f / scale_factor, x = s * (float)(dst - 1);
    const float b = floorf(fmaxf(x - s, 0.0f)), e = ceilf(fminf(x + s, (float)src - 1.0f));
    return b + 1.0f <= (float)src - 1.0f && e <= (float)src - 1.0f;
}

inline int brox_ld(int w) { return (w + BROX_LD_ALIGN - 1) / BROX_LD_ALIGN * BROX_LD_ALIGN; }
inline size_t brox_plane(int w, int h) { return ((size_t)brox_ld(w) * h + BROX_PLANE_ALIGN - 1) / BROX_PLANE_ALIGN * BROX_PLANE_ALIGN; }

// THE selection rule of the solver's form: a level whose sides both reach BROX_BLOCKED_MIN_SIDE runs the blocked form.  Measured on
// MI355X (profiles/brox): the blocked form wins only per iteration on a 1080p level (34.3 against 37.2 us), loses at
// 640 x 480 (10.2 against 9.4 us) and loses every whole calc (+13 .. +39 %), so the constant lies above every legal size: plain everywhere.
enum { BROX_BLOCKED_MIN_SIDE = 1 << 30 };
inline int brox_sor_form(int w, int h, int form)
{
    if (form != BROX_FORM_AUTO) return form;
    return (w >= BROX_BLOCKED_MIN_SIDE && h >= BROX_BLOCKED_MIN_SIDE) ? BROX_FORM_BLOCKED : BROX_FORM_PLAIN;
}

enum BroxKernel { BROX_K_RESIZE_DOWN,  // level l-1 -> level l, both frames
                  BROX_K_ZERO,         // u, v of the coarsest level / du, dv of a level
                  BROX_K_DERIV1,       // Ix0, Iy0, Ix, Iy
                  BROX_K_DERIV2,       // Ixx, Iyy, Ixy
                  BROX_K_PREPARE1, BROX_K_PREPARE2,
                  BROX_K_SOR_PLAIN,    // arg: colour
                  BROX_K_SOR_BLOCKED,  // arg: solver iterations of this launch
                  BROX_K_RESIZE_UP,    // u + du, v + dv of level l -> u, v of level l-1, times 1 / scale_factor
                  BROX_K_ADD_OUT };    // u + du, v + dv of level 0 -> the caller's flow
struct BroxLaunch { int kernel, level; unsigned gx, gy, gz, threads; int arg; };

// the plane slots of the solver; every slot holds a level-0 plane
enum BroxSlot { S_IX, S_IXX, S_IX0, S_IY, S_IYY, S_IY0, S_IXY, S_DIFFX, S_DIFFY, S_DENU, S_DENV, S_NDUDV, S_NU, S_NV,
                S_U, S_V, S_U2, S_V2, S_DU, S_DV, S_DU2, S_DV2, S_COUNT };

struct BroxPlan {
    BroxErr err;
    std::vector<BroxLevel> levels;       // 0 = the frame
    size_t off_slot[S_COUNT];            // floats
    size_t scratch_bytes;
    std::vector<BroxLaunch> launches;
    int sor_launches;
};

inline unsigned brox_div_up(int a, int b) { return (unsigned)((a + b - 1) / b); }

// the solver's launches of one inner iteration's linear system
inline void brox_sor_launches(int w, int h, int level, int solver_iterations, int form, std::vector<BroxLaunch> *out)
{
    if (brox_sor_form(w, h, form) == BROX_FORM_BLOCKED) {
        for (int it = 0; it < solver_iterations; it += BROX_SOR_KMAX) {
            const int k = solver_iterations - it < BROX_SOR_KMAX ? solver_iterations - it : BROX_SOR_KMAX;
            out->push_back({BROX_K_SOR_BLOCKED, level, brox_div_up(w, BROX_SOR_TILE_X), brox_div_up(h, BROX_SOR_TILE_Y), 1, BROX_SOR_THREADS, k});
        }
        return;
    }
    for (int it = 0; it < solver_iterations; ++it)
        for (int colour = 0; colour < 2; ++colour)
            out->push_back({BROX_K_SOR_PLAIN, level, brox_div_up(w, BROX_BLOCK_X), brox_div_up(h, BROX_BLOCK_Y), 1, BROX_BLOCK_X * BROX_BLOCK_Y, colour});
}

inline BroxPlan brox_make_plan(int rows, int cols, const mi_brox_params &p, int form)
{
    BroxPlan plan = {};
    plan.err = brox_check_params(p);
    if (plan.err.code == MI_OK) plan.err = brox_check_size(rows, cols);
    if (plan.err.code != MI_OK) return plan;
    std::vector<int> ws, hs;
    brox_level_sizes(cols, rows, p.scale_factor, p.outer_iterations, &ws, &hs);
    for (size_t l = 1; l < ws.size(); ++l)
        if (ws[l] < BROX_MIN_LEVEL_SIDE || hs[l] < BROX_MIN_LEVEL_SIDE) {
            plan.err = {MI_ERR_BAD_ARG, "scale_factor gives a pyramid level with a side of 1: the derivative filter's mirror leaves such a level"};
            return plan;
        }
    for (size_t l = 1; l < ws.size(); ++l)
        if (!brox_resize_down_fits(ws[l - 1], ws[l], p.scale_factor) || !brox_resize_down_fits(hs[l - 1], hs[l], p.scale_factor)) {
            plan.err = {MI_ERR_BAD_SIZE, "a pyramid level's supersample window leaves the level above it"};
            return plan;
        }
    size_t o = 0;
    const size_t plane0 = brox_plane(cols, rows);
    for (int s = 0; s < S_COUNT; ++s) { plan.off_slot[s] = o; o += plane0; }
    for (size_t l = 0; l < ws.size(); ++l) {
        BroxLevel L = {ws[l], hs[l], brox_ld(ws[l]), 0, 0};
        if (l > 0) {
            L.off_i0 = o; o += brox_plane(L.w, L.h);
            L.off_i1 = o; o += brox_plane(L.w, L.h);
        }
        plan.levels.push_back(L);
    }
    plan.scratch_bytes = o * sizeof(float);
    const unsigned T = BROX_BLOCK_X * BROX_BLOCK_Y;
    auto grid = [&](int kernel, int level, unsigned gz, int arg) {
        const BroxLevel &L = plan.levels[level];
        plan.launches.push_back({kernel, level, brox_div_up(L.w, BROX_BLOCK_X), brox_div_up(L.h, BROX_BLOCK_Y), gz, T, arg});
    };
    const int n = (int)plan.levels.size();
    for (int l = 1; l < n; ++l) grid(BROX_K_RESIZE_DOWN, l, 2, 0);
    grid(BROX_K_ZERO, n - 1, 1, S_U);
    for (int l = n - 1; l >= 0; --l) {
        const BroxLevel &L = plan.levels[l];
        grid(BROX_K_ZERO, l, 1, S_DU);
        grid(BROX_K_DERIV1, l, 4, 0);
        grid(BROX_K_DERIV2, l, 3, 0);
        for (int in = 0; in < p.inner_iterations; ++in) {
            grid(BROX_K_PREPARE1, l, 1, 0);
            grid(BROX_K_PREPARE2, l, 1, 0);
            const size_t before = plan.launches.size();
            brox_sor_launches(L.w, L.h, l, p.solver_iterations, form, &plan.launches);
            plan.sor_launches += (int)(plan.launches.size() - before);
        }
        if (l > 0) grid(BROX_K_RESIZE_UP, l - 1, 2, 0);   // the grid of the DESTINATION level
        else grid(BROX_K_ADD_OUT, 0, 1, 0);
    }
    return plan;
}

}  // namespace brox
}  // namespace mi
