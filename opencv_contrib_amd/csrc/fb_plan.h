// The PLAN of one mi_farneback_calc_batch call (farneback_api.cpp): which pyramid levels exist, their geometry, the form every launch
// takes, where every plane lies in the handle's scratch, and the ORDERED LIST of launches with the chain (stream) each runs on.  Pure host
// arithmetic over the call's shape and the tuning knobs, no HIP types: tests/cpp/fb_plan_test.cpp compiles it alone.  The entry point only
// EXECUTES the list; the launchers resolve a *_AUTO form with the rule functions below and choose nothing themselves.
// Reference: FarnebackOpticalFlowImpl::calcImpl, cudaoptflow/src/farneback.cpp:314-482.
#pragma once
#include "fb_groups.h"
#include <cmath>
#include <vector>

namespace mi {
namespace fb {

// Launch forms.  AUTO (a launcher's default, for the stage-level entry points) = the rule function of the kind; a plan holds resolved forms
// only.  A forced form that has no kernel for the request is MI_ERR_BAD_ARG with nothing launched (mi_selftest.h runs every form on the same planes).
enum BlurForm { BLUR_AUTO = 0, BLUR_GENERIC_FAST, BLUR_GENERIC_FULL, BLUR_TILED };   // FULL: the border rule with every fold (kh >= w or h)
enum PolyForm { POLY_AUTO = 0, POLY_ROW, POLY_TILED };
enum IterForm { ITER_AUTO = 0, ITER_ROW, ITER_TILE256, ITER_TILE64 };
constexpr int kFmtPairs = 64;        // pairs per launch of the steps that take the caller's matrices as a by-value table (FmtTab)

struct FbShape {
    int W, H, B;                     // frame size, pairs of the batch
    int num_levels; double pyr_scale; bool fast_pyramids;
    int num_iters;
    bool use_init;                   // OPTFLOW_USE_INITIAL_FLOW
    int win_size = 13, poly_n = 5;
};
struct FbKnobs {
    int fuse, pair;                  // MIFLOW_FB_FUSE / MIFLOW_FB_PAIR: -1 = automatic, 0 / 1 = forced
    int group_mb;                    // MIFLOW_FB_GROUP_MB: last-level-cache budget of the pair groups in flight
    int chains;                      // streams the groups of a level may alternate over: 2, or 1 (tuning; always 1 while the caller's stream is captured)
    int simds;                       // SIMDs of the device (the underfill thresholds are in workgroups per CU)
    bool iterate2_ok = true;         // two iterations per launch are allowed (false: never paired, whatever the window size)
    // the switches of the form rules below, with the release defaults
    int fb_tiled = 1, fb_rows = 4, fb_narrow = -1;   // MIFLOW_FB_TILED, _ROWS (4 | 8), _NARROW (-1 = automatic, 0 / 1 = forced): the iteration kernel
    int fb_poly_tiled = 1, fb_blur_tiled = 1;        // MIFLOW_FB_POLY_TILED, _BLUR_TILED: expansion / pre-blur on row tiles
    int fb_direct = 1;                               // MIFLOW_FB_DIRECT: the pre-blur may read the caller's matrices
};

inline int fb_round(double v) { return (int)std::lrint(v); }   // cvRound
inline int fb_div_up(int a, int b) { return (a + b - 1) / b; }

// ---- the form rules: pure functions of a launch's geometry and the knobs
// Iteration.  Tiled kernels exist for winSize 9, 13 (the default), 15, 21.  Narrow 64 x 4 tiles where the 256-column grid would leave most of
// the device idle (fewer workgroups than two per CU): the launch then costs its dependent steps, and a 64 x 4 tile has a third of them.
inline bool fb_iter_has_tile(int kh) { return kh == 4 || kh == 6 || kh == 7 || kh == 10; }
inline IterForm fb_iter_form(int w, int h, int batch, int kh, const FbKnobs &K)
{
    if (!K.fb_tiled || !fb_iter_has_tile(kh)) return ITER_ROW;
    const bool narrow = K.fb_narrow >= 0 ? K.fb_narrow != 0 : (long long)fb_div_up(w, 256) * fb_div_up(h, K.fb_rows) * batch < 2LL * (K.simds / 4);
    return narrow && K.fb_rows == 4 ? ITER_TILE64 : ITER_TILE256;
}
// two iterations per launch: instantiated for winSize 9, 13, 15
inline bool fb_iter2_ok(int kh, const FbKnobs &K) { return K.fb_tiled && (kh == 4 || kh == 6 || kh == 7); }
// Expansion of `planes` (pairs x frames) planes: the 8-row tiles need a grid that fills the device, and do not sample a resize
inline PolyForm fb_poly_form(int w, int h, int planes, int poly_n, bool resized, const FbKnobs &K)
{
    return !resized && K.fb_poly_tiled && (long long)fb_div_up(w, 256 - 2 * poly_n) * fb_div_up(h, 8) * planes >= 1024 ? POLY_TILED : POLY_ROW;
}
// Pre-blur.  fast: the taps reach less than one image size past the border; tiles for the half sizes the pyramid of pyrScale 0.5
// (1, 1, 4, 9, 19) and its neighbours use.  direct: the tiled blur has an instantiation that reads the caller's matrices.
inline bool fb_blur_fast(int w, int h, int kh) { return kh < w && kh < h && w >= 2 && h >= 2; }
inline bool fb_blur_has_tile(int w, int h, int kh) { return fb_blur_fast(w, h, kh) && (kh == 1 || kh == 2 || kh == 3 || kh == 4 || kh == 9 || kh == 19); }
inline BlurForm fb_blur_form(int w, int h, int kh, const FbKnobs &K)
{
    return fb_blur_has_tile(w, h, kh) && K.fb_blur_tiled ? BLUR_TILED : fb_blur_fast(w, h, kh) ? BLUR_GENERIC_FAST : BLUR_GENERIC_FULL;
}
inline bool fb_blur_direct_ok(int w, int h, int kh, const FbKnobs &K) { return fb_blur_has_tile(w, h, kh) && K.fb_blur_tiled != 0; }

struct FbLevel {
    int w, h, ld;                    // level image (farneback.cpp:374-395); ld = floats per plane row
    double scale, sigma;
    int smooth;                      // pre-blur kernel size (odd, >= 3)
    // how the level's flow planes start
    bool coarsest;
    bool init_resize;                // coarsest, initial flow given, not level 0: resized from the caller's flow (:398-404)
    bool zero_flow;                  // coarsest, no initial flow, iterations > 0: no fill -- the first matrix update takes the flow as zero and the iterations write every pixel
    bool clear_flow;                 // coarsest, no initial flow, no iterations: the planes are cleared
    bool zoom_fused;                 // finer level of another size: the coarser flow is sampled inside the first matrix update (:412-417, same arithmetic)
    bool zoom;                       // finer level otherwise: a resize (or copy) launch
    // how its launches are cut
    GroupPlan groups;                // pairs per launch chain (fb_groups.h); groups.pairs == B: the whole batch
    bool staged;                     // groups.pairs < B: the zoom and the frames' side (blur, expansion) run group by group too
    bool pair_it;                    // two iterations per launch (levels whose 64 x 4 grid underfills the device)
    // where its planes lie (floats from the start of a pair's block)
    long long flow;                  // x plane; y = x + one full-size plane
    long long img[2];                // the two frames' level images the expansion reads: the pyrDown chain (fastPyramids), else the blurred
                                     // frames (level of the full size, or resize sampled in the expansion) or the level planes behind a resize launch
};

// Scratch of one pair, in floats: 34 full-size planes.  The block of pair b starts b * bs behind pair 0's.  The two frames' planes of a kind
// are ADJACENT -- frame 1 = frame 0 + one plane (pn), R[1] = R[0] + five -- because the pyramid kernels run both frames in one launch; so
// are the x and y plane of a flow slot (one fill clears both).
struct FbLayout {
    long long pn, bs;                // floats of a full-size plane / of a pair's block
    long long frames, blurred, lvl;  // 2 planes each: the converted frames, their pre-blur, the resized level images
    long long R, M, bufM;            // R: 2 x 5 planes (both expansions); M, bufM: 5 each, alternating over the iterations
    long long flow[3];               // 2 planes each: slot 0 = level 0 (and the initial flow), slots 1, 2 alternate over the coarse levels
    long long pyr;                   // 2 planes for the fast-pyramid levels >= 1 of both frames (sum over the half sizes < one plane per frame)
};
inline FbLayout fb_layout(int W, int H)
{
    FbLayout A;
    A.pn = (long long)((W + 63) / 64 * 64) * H;
    A.bs = 34 * A.pn;
    A.frames = 0; A.blurred = 2 * A.pn; A.lvl = 4 * A.pn; A.R = 6 * A.pn; A.M = 16 * A.pn; A.bufM = 21 * A.pn;
    for (int a = 0; a < 3; ++a) A.flow[a] = (26 + 2 * a) * A.pn;
    A.pyr = 32 * A.pn;
    return A;
}

enum FbOp {
    FB_CONVERT,                // caller's frames -> f32 planes.  form 1: pairs b0 .. b0 + nb - 1 (<= kFmtPairs) in one launch; 0: the single-pair kernel
    FB_SPLIT_FLOW,             // caller's initial flow of pair b0 -> flow slot 0
    FB_PYR_DOWN,               // fastPyramids: image of frame `iter`, level - 1 -> level
    FB_INIT_RESIZE,            // coarsest flow = resize(initial flow) * scale
    FB_CLEAR_FLOW,             // coarsest flow = 0.  form = fills: 1 (over both planes and the gap between them) or 2
    FB_ZOOM,                   // flow = resize (or copy) of the coarser level's * 1 / pyrScale
    FB_BLUR,                   // frames -> blurred, both frames; form: BlurForm
    FB_BLUR_DIRECT,            // caller's frames of pairs b0 .. b0 + nb - 1 (<= kFmtPairs) -> blurred
    FB_LEVEL_RESIZE,           // blurred -> level planes
    FB_POLY_EXP,               // level images -> R, both frames; form: PolyForm
    FB_POLY_EXP_RESIZED,       // blurred -> R, the resize sampled on the fly (row form)
    FB_UPDATE_MATRICES,        // flow (zero_flow: taken as zero), R -> M
    FB_UPDATE_MATRICES_ZOOM,   // the zoom and the first matrix update in one launch
    FB_ITERATE,                // form: IterForm
    FB_ITERATE2,               // iterations iter and iter + 1 in one launch
    FB_MERGE,                  // flow slot 0 -> the caller's matrices.  form as FB_CONVERT
    FB_FORK, FB_JOIN           // chain 1 starts behind chain 0 / chain 0 goes on behind chain 1
};
struct FbLaunch {
    int op, level;
    int b0, nb;                      // the pairs of its group
    int chain;                       // 0: the caller's stream, 1: the handle's
    int iter;                        // iteration index (FB_PYR_DOWN: the frame)
    int form;                        // resolved form (see the op)
    bool update;                     // iterations: the matrices are updated for a next one
    bool flip;                       // iterations: M is read from bufM and written to M
    bool writes_merged;              // iterations: this launch also writes the caller's flow matrix
};
struct FbPlan {
    int levels;                      // the level loop runs k = levels .. 0
    bool fuse_small;                 // launch-latency-bound call: the few-launch forms (resize sampled in the consumers, merge written by the last iteration)
    bool direct;                     // every level's pre-blur reads the caller's matrices: no conversion pass
    std::vector<FbLevel> lv;         // lv[k]
    FbLayout lay;
    std::vector<FbLaunch> launches;
};

inline FbPlan fb_make_plan(const FbShape &S, const FbKnobs &K)
{
    FbPlan p;
    // crop unnecessary levels, farneback.cpp:330-340 (MIN_SIZE = 32, :54)
    double scale = 1;
    p.levels = 0;
    for (; p.levels < S.num_levels; p.levels++) {
        scale *= S.pyr_scale;
        if (S.W * scale < 32 || S.H * scale < 32) break;
    }
    p.fuse_small = K.fuse >= 0 ? K.fuse != 0 : (long long)S.W * S.H * S.B <= 1500000;
    p.lv.resize(p.levels + 1);
    const FbLayout &A = p.lay = fb_layout(S.W, S.H);
    const int kh = S.win_size / 2;
    // fastPyramids: the levels are the pyrDown chain's sizes (:346-359), not the rounded scales
    std::vector<int> fw(p.levels + 1), fh(p.levels + 1);
    fw[0] = S.W; fh[0] = S.H;
    for (int i = 1; i <= p.levels; ++i) { fw[i] = (fw[i - 1] + 1) / 2; fh[i] = (fh[i - 1] + 1) / 2; }
    p.direct = !S.fast_pyramids && K.fb_direct != 0;
    for (int k = p.levels; k >= 0; k--) {
        FbLevel &L = p.lv[k];
        scale = 1;
        for (int i = 0; i < k; i++) scale *= S.pyr_scale;
        L.scale = scale;
        L.sigma = (1. / scale - 1) * 0.5;
        int smooth = fb_round(L.sigma * 5) | 1;
        L.smooth = smooth > 3 ? smooth : 3;
        L.w = S.fast_pyramids ? fw[k] : fb_round(S.W * scale);
        L.h = S.fast_pyramids ? fh[k] : fb_round(S.H * scale);
        L.ld = (L.w + 63) / 64 * 64;
        L.coarsest = k == p.levels;
        L.init_resize = L.coarsest && S.use_init && k > 0;
        L.zero_flow = L.coarsest && !S.use_init && S.num_iters > 0;
        L.clear_flow = L.coarsest && !S.use_init && S.num_iters <= 0;
        const bool same_size = !L.coarsest && p.lv[k + 1].w == L.w && p.lv[k + 1].h == L.h;
        L.zoom_fused = !L.coarsest && !same_size && K.fuse != 0;
        L.zoom = !L.coarsest && !L.zoom_fused;
        L.groups = GroupPlan{S.B, 1, false};
        if (!p.fuse_small) L.groups = plan_pair_groups(S.B, 22LL * (long long)L.ld * L.h * (long long)sizeof(float), K.group_mb, K.chains);
        L.staged = L.groups.pairs < S.B;
        // (not the narrow rule of fb_iter_form: that one counts 256-column tiles against two per CU with `<`, this one 64 x 4 tiles with
        // `<=`.  Two thresholds for two kernels, each as it was measured; they are not meant to agree.)
        L.pair_it = p.fuse_small && K.iterate2_ok && fb_iter2_ok(kh, K) &&
                    (K.pair >= 0 ? K.pair != 0 : (long long)fb_div_up(L.w, 64) * fb_div_up(L.h, 4) * S.B <= 2LL * (K.simds / 4));
        L.flow = A.flow[k > 0 ? 1 + (k & 1) : 0];
        const bool full = L.w == S.W && L.h == S.H;
        L.img[0] = full || p.fuse_small ? A.blurred : A.lvl;
        L.img[1] = L.img[0] + A.pn;
        if (!fb_blur_direct_ok(S.W, S.H, L.smooth / 2, K)) p.direct = false;
    }
    if (S.fast_pyramids) {
        long long o = A.pyr;
        for (int i = 0; i <= p.levels; ++i)
            for (int f = 0; f < 2; ++f) {
                p.lv[i].img[f] = i ? o : A.frames + f * A.pn;
                if (i) o += (long long)p.lv[i].ld * p.lv[i].h;
            }
    }

    // ---- the launches, in the order they are enqueued
    std::vector<FbLaunch> &Q = p.launches;
    {
        size_t n = 8 + (size_t)S.B * (S.use_init ? 2 : 1) + 2 * (size_t)p.levels;
        for (const FbLevel &L : p.lv) n += 5 + (size_t)L.groups.groups * (size_t)(6 + fb_div_up(L.groups.pairs, kFmtPairs) + (S.num_iters > 0 ? S.num_iters : 0));
        Q.reserve(n);
    }
    auto add = [&Q](int op, int level, int b0, int nb, int chain = 0, int form = 0) { Q.push_back(FbLaunch{op, level, b0, nb, chain, 0, form, false, false, false}); };
    auto per_pair_step = [&](int op) {   // one launch per kFmtPairs pairs of a batch (blockIdx.z = pair), the single-pair kernel otherwise
        if (S.B > 1) for (int b0 = 0; b0 < S.B; b0 += kFmtPairs) add(op, 0, b0, std::min(kFmtPairs, S.B - b0), 0, 1);
        else add(op, 0, 0, 1);
    };
    // blur + resize + polynomial expansion of BOTH frames for level k (the reference's loop over the two frames, :434-454, each stage once for
    // both), for a pair group of the level: the expansions it is about to iterate on are still in the last-level cache
    auto frames_side = [&](int k, int b0, int nb, int chain) {
        const FbLevel &L = p.lv[k];
        const bool full = L.w == S.W && L.h == S.H;
        if (!S.fast_pyramids) {
            if (p.direct) for (int c0 = 0; c0 < nb; c0 += kFmtPairs) add(FB_BLUR_DIRECT, k, b0 + c0, std::min(kFmtPairs, nb - c0), chain);
            else add(FB_BLUR, k, b0, nb, chain, fb_blur_form(S.W, S.H, L.smooth / 2, K));
            // the level image = cuda::resize of the blurred frame (:447-448).  Few pairs: sampled inside the expansion kernel (same
            // arithmetic, same bits, one launch less); many pairs: through the level planes (the expansion reads each sample 11 times)
            if (!full && p.fuse_small) { add(FB_POLY_EXP_RESIZED, k, b0, nb, chain, POLY_ROW); return; }
            if (!full) add(FB_LEVEL_RESIZE, k, b0, nb, chain);
        }
        add(FB_POLY_EXP, k, b0, nb, chain, fb_poly_form(L.w, L.h, nb * 2, S.poly_n, false, K));
    };
    bool merged = false;
    if (S.fast_pyramids) per_pair_step(FB_CONVERT);   // convertTo(CV_32F), :342-345; the fast pyramid is built from the converted frames
    for (int b = 0; b < S.B && S.use_init; ++b) add(FB_SPLIT_FLOW, 0, b, 1);
    for (int i = 1; i <= p.levels && S.fast_pyramids; ++i)   // :346-359
        for (int f = 0; f < 2; ++f) { add(FB_PYR_DOWN, i, 0, S.B); Q.back().iter = f; }
    if (!S.fast_pyramids && !p.direct) per_pair_step(FB_CONVERT);
    for (int k = p.levels; k >= 0; k--) {   // :396-471
        const FbLevel &L = p.lv[k];
        if (L.init_resize) add(FB_INIT_RESIZE, k, 0, S.B);
        // one fill while the gap cleared with the planes is small (a single pair: one launch less); a batch would clear B full-size planes for two coarse ones
        else if (L.clear_flow) add(FB_CLEAR_FLOW, k, 0, S.B, 0, (long long)sizeof(float) * A.pn * S.B <= (8LL << 20) ? 1 : 2);
        if (!L.staged) {   // once for the batch, as the reference orders them
            if (L.zoom) add(FB_ZOOM, k, 0, S.B);
            frames_side(k, 0, S.B, 0);
        }
        // Pair GROUPS (fb_groups.h): the matrix update and ALL iterations of a few pairs whose planes fit the last-level cache, then the next
        // group.  The same launches on the same data in the same order per pair: bit-identical.  Groups are independent chains of launches: two
        // of them run side by side, the second on the handle's stream -- the launches of a chain wait for each other's last workgroups,
        // and the other chain fills those tails.
        if (L.groups.two) add(FB_FORK, k, 0, S.B);
        int gi = 0;
        for (int b0 = 0; b0 < S.B; b0 += L.groups.pairs, ++gi) {
            const int nb = std::min(L.groups.pairs, S.B - b0), chain = L.groups.two ? gi & 1 : 0;
            if (L.staged) {
                if (L.zoom) add(FB_ZOOM, k, b0, nb, chain);
                frames_side(k, b0, nb, chain);
            }
            add(L.zoom_fused ? FB_UPDATE_MATRICES_ZOOM : FB_UPDATE_MATRICES, k, b0, nb, chain);   // :458
            bool flip = false;
            for (int i = 0; i < S.num_iters; i++, flip = !flip) {   // :465-471 -> updateFlow_boxFilter / _gaussianBlur :278-312, one launch
                const bool two_it = L.pair_it && i + 1 < S.num_iters;
                const int form = two_it ? 0 : fb_iter_form(L.w, L.h, nb, kh, K);
                add(two_it ? FB_ITERATE2 : FB_ITERATE, k, b0, nb, chain, form);
                FbLaunch &l = Q.back();
                l.iter = i;
                if (two_it) ++i;
                l.update = i < S.num_iters - 1;
                l.flip = flip;
                // the final iteration of a single small call writes the caller's matrix itself: the two-iteration kernel, or a tiled one
                l.writes_merged = k == 0 && i == S.num_iters - 1 && S.B == 1 && p.fuse_small && (two_it || form != ITER_ROW);
                merged = merged || l.writes_merged;
            }
        }
        if (L.groups.two) add(FB_JOIN, k, 0, S.B);
    }
    if (!merged) per_pair_step(FB_MERGE);   // cuda::merge :197-198
    return p;
}

}  // namespace fb
}  // namespace mi
