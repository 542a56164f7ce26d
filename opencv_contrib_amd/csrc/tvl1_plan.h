// The PLAN of one lane's TV-L1 calc (tvl1_api.cpp lane_calc): the pyramid levels and the scratch arena's layout, which control
// features the calc uses (convergence check, speculative steps, history, host feedback) with the slot count they need, and per warp
// the form of its iterations and their block lengths.  Pure host arithmetic over the call's shape and the tuning knobs, no HIP types:
// tests/cpp/tvl1_plan_test.cpp compiles it alone.  lane_calc only EXECUTES a plan.
// Reference: OpticalFlowDual_TVL1_Impl::calcImpl / procOneScale, cudaoptflow/src/tvl1flow.cpp:185-382.
#pragma once
#include "miflow/c_api.h"
#include "tvl1_tb_table.h"
#include <algorithm>
#include <array>
#include <cmath>
#include <cstddef>
#include <initializer_list>
#include <vector>

namespace mi {
namespace tvl1 {

// All scratch planes of one pyramid level are dense float planes, `ld` floats per row
// (multiple of 64), `ps` floats between consecutive pairs of the batch.
struct Geo {
    int w, h, ld;
    long long ps;  // pair stride (floats)
    int batch;
};

constexpr int kTbMaxBlock = 10;        // longest block of the streaming fast-math kernels (k_iterate_tbr)
constexpr int kTbExactMaxBlock = 5;    // ... of the exact-math blocks (MODE 2)
constexpr int kTileMaxBlock = 10;      // ... of the register-tile kernel (its margin, TILE_M)
constexpr double kLargeLevel = 12e6;   // px x pairs from which the T = 10 kernel pays for a long first speculative block

// The tuning switches and register-tile facts a plan depends on (tvl1_api.cpp tv_knobs() fills them once from tuning()).
struct TvKnobs {
    long long tile_maxpx;            // levels of at most this many pixels x pairs run on the register-tile kernel (0: never) ...
    int tile_spec;                   // ... the speculative steps too
    int tile_variant, tile_small_wgs, tile_variants, tile_rows[8];   // register-tile shape: forced index (-1: by grid size) / small-grid
                                                                     // threshold / shapes in the table and their rows (owned + margins)
    int tile_fb_block, tile_fb_model;   // one-or-two-pair calcs on tiles: block length / cost model's us per pass (0: off)
    bool tb_force;                   // greedy blocks of exactly the cap (tuning sweeps)
    int tb_nograd, tb_jw, tb_jw_spec;   // the warp leaves |grad|^2 to the passes / joined-wave form of the T = 10 pass / ... of the speculative steps too
    int tb_ppl, tb_wps, tb_pf;       // MIFLOW_TB_VARIANT: the alternative row of a block length (-1: the default row)
    int tb_p16;                      // p as snorm16 between passes (experiments build)
    int tb_il;                       // the calc's final pass writes the flow into the callers' matrices itself (0: k_pack_flow behind every calc)
    int tb_fw;                       // warp fused into the pass (experiments build; 0 in the release library)
    int tb_skip_p, tb_hist, spec, exact_tb;
    int fb_poll, fb_ahead;
    int warp_fast, warp_lds, x_skip;
};

// ---- helpers shared with the kernel files ------------------------------------------------------------------------------------------

// this level (pixels x pairs) is small enough for the register-tile kernel
inline bool tile_eligible(const Geo &g, const TvKnobs &K)
{
    return K.tile_maxpx > 0 && (long long)g.w * g.h * g.batch <= K.tile_maxpx;
}
// a launch of T iterations on level g runs on the register-tile kernel: fixed work (spec = false) or speculative steps (spec = true)
inline bool runs_on_tiles(const Geo &g, int T, const TvKnobs &K, bool spec = false)
{
    return tile_eligible(g, K) && T <= kTileMaxBlock && (spec ? K.tile_spec != 0 : !K.tb_force);
}

// ---- which kernel runs a block ------------------------------------------------------------------------------------------------------
enum class TbUse { Fixed, Indep, Exact, Spec };   // fixed work / ... on independent waves only (test hook) / exact-math blocks / speculative steps

// THE selection rule of the streaming kernels: the row of kTbRows that runs T iterations, or nullptr where the build has none.
// gam: the illumination channel (its own rows, which never read a |grad|^2 plane); nograd: no plane is stored; fw: the warp inside the
// pass (1 / 2, fixed work).  Fixed work with a plane takes the joined-wave row of MIFLOW_TB_JW where one of that length exists, else the
// independent-wave row named by MIFLOW_TB_VARIANT, else the first one; the speculative steps with a plane take the joined or independent
// row that reads it where the build has one (experiments), else the row that forms |grad|^2 itself and ignores the stored plane.
inline const TbRow *tb_select(TbUse use, int T, bool gam, bool nograd, const TvKnobs &K, int fw = 0)
{
    const int mode = use == TbUse::Spec ? 1 : use == TbUse::Exact ? 2 : 0;
    const auto first = [&](auto pred) -> const TbRow * {
        for (const TbRow &r : kTbRows)
            if (r.MODE == mode && r.T == T && r.GAM == gam && (r.FW != 0) == (fw != 0) && pred(r)) return &r;
        return nullptr;
    };
    const auto any = [](const TbRow &) { return true; };
    const auto indep = [](const TbRow &r) { return r.JW == 0 && !r.NG; };
    if (use == TbUse::Exact) return gam || nograd ? nullptr : first(any);
    if (use == TbUse::Indep) return nograd ? nullptr : gam ? first([](const TbRow &r) { return r.JW == 0; }) : first(indep);
    if (gam) return first(any);
    if (use == TbUse::Spec) {
        const TbRow *reads = nograd ? nullptr : (K.tb_jw >= 2 && K.tb_jw_spec) ? first([](const TbRow &r) { return r.JW == 2 && !r.NG; }) : first(indep);
        return reads ? reads : first([](const TbRow &r) { return r.NG; });
    }
    if (fw) return first([&](const TbRow &r) { return r.FW == fw; });
    if (nograd) return first([&](const TbRow &r) { return r.NG && r.P16 == (K.tb_p16 != 0); });
    if (K.tb_jw && K.tb_ppl < 0)
        if (const TbRow *joined = first([&](const TbRow &r) { return r.JW == K.tb_jw && !r.NG; })) return joined;
    const TbRow *variant = first([&](const TbRow &r) { return indep(r) && r.PPL == K.tb_ppl && r.WPS == K.tb_wps && r.PF == K.tb_pf; });
    return variant ? variant : first(indep);
}

// What runs one block: the register tile, or a streaming row with the planner's band height (rows = 0) or a given one.  Neither: the
// build has no kernel of that length (the launch reports it).
struct TbKernel {
    bool tile;
    const TbRow *row;
    int rows;
};
// What a caller outside the plan may force (the stage-level entry, tvl1_stage_api.cpp); lane_calc passes none.
struct TbOverride {
    bool force_streaming;     // never the register tile
    int rows;                 // band height (0: the planner's)
    bool independent_waves;   // fixed work on the independent-wave row of the block length
};
inline TbKernel tb_kernel(TbUse use, int T, const Geo &g, bool gam, bool nograd, const TvKnobs &K, const TbOverride &o = TbOverride{})
{
    if (!o.force_streaming && (use == TbUse::Fixed || use == TbUse::Spec) && runs_on_tiles(g, T, K, use == TbUse::Spec))
        return TbKernel{true, nullptr, 0};
    return TbKernel{false, tb_select(o.independent_waves ? TbUse::Indep : use, T, gam, nograd, K), o.rows};
}

// a fixed-work pass of T iterations can do without a stored |grad|^2 plane: the default joined-wave kernel has a row that forms it, on a
// streaming level
inline bool tb_nograd_ok(int T, const Geo &g, const TvKnobs &K)
{
    return K.tb_nograd && K.tb_jw == 2 && K.tb_ppl < 0 && !runs_on_tiles(g, T, K) && tb_select(TbUse::Fixed, T, false, true, K);
}
// the same for the speculative steps (the register-tile kernel reads the stored plane)
inline bool tb_spec_nograd_ok(const Geo &g, const TvKnobs &K)
{
    return K.tb_nograd && K.tb_jw >= 2 && K.tb_jw_spec && !(tile_eligible(g, K) && K.tile_spec != 0);
}
// a warp whose iterations are ONE pass of the default T = 10 kernel runs inside that pass (k_iterate_tbr FW); the two warp arithmetics
// that exist in that form: CPU class + tap-by-tap sums, cv::cuda + separable sums.  (The producers' window gather needs an interior.)
inline bool tb_fused_ok(int T, const Geo &g, int semantics, bool fast_warp, const TvKnobs &K)
{
    if (!K.tb_fw || !tb_nograd_ok(T, g, K) || g.w < 6 || g.h < 6) return false;
    return (semantics == MI_SEM_CPU_REF && !fast_warp) || (semantics == MI_SEM_CUDA_COMPAT && fast_warp);
}

// register-tile shape for level g (MIFLOW_TILE_VARIANT < 0: by the size of the grid -- where 64-row tiles of 16 waves give the device
// fewer than four workgroups per CU, 48-row tiles of 8 waves x 6 rows run the same iterations faster, r10c; the speculative steps take
// the small shape up to twice the grid size, r19k)
inline int tile_auto_variant(const Geo &g, bool spec, const TvKnobs &K)
{
    if (K.tile_variant >= 0) return K.tile_variant < K.tile_variants ? K.tile_variant : 0;
    constexpr int M = kTileMaxBlock, LW = 64, STRIDE = LW - 2 * M;
    const long long nstrips = g.w <= LW - M ? 1 : 1 + (g.w - (LW - M) + STRIDE - 1) / STRIDE;
    const long long wgs = nstrips * ((g.h + (64 - 2 * M) - 1) / (64 - 2 * M)) * g.batch;
    return wgs < (long long)K.tile_small_wgs * (spec ? 2 : 1) ? 1 : 0;
}
// rows (owned + margins) of the tiles the speculative steps of level g run on
inline int tile_rows_for(const Geo &g, const TvKnobs &K) { return K.tile_rows[tile_auto_variant(g, true, K)]; }

// the largest of the block lengths `sup` that fits, again and again
inline std::vector<int> greedy_blocks(int n, int cap, std::initializer_list<int> sup)
{
    std::vector<int> blocks;
    for (int left = n; left > 0; left -= blocks.back()) {
        int t = 1;
        for (int c : sup) if (c <= left && c <= cap) t = std::max(t, c);
        blocks.push_back(t);
    }
    return blocks;
}
// Decompose n iterations into supported time blocks minimising the modelled cost.  cost[T] = measured ps per pixel-iteration of
// k_iterate_tbr<T> at 1080p x 16 pairs (tools/sweep_tb.py, profiles/r01s): deeper blocks save HBM passes but cost registers
// (occupancy) and halo recomputation.
inline std::vector<int> tb_plan(int n, int cap, const TvKnobs &K)
{
    static const int sup[] = {1, 2, 3, 4, 5, 6, 8, 10};
    static const double cost[11] = {0, 15.6, 9.4, 6.6, 4.65, 3.9, 3.7, 0, 2.83, 0, 2.54};
    std::vector<int> blocks;
    if (n <= 0) return blocks;
    if (K.tb_force) return greedy_blocks(n, cap, {1, 2, 3, 4, 5, 6, 8, 10});   // tuning sweeps: blocks of exactly `cap` (then the largest that fit)
    std::vector<double> best(n + 1, 1e300);
    std::vector<int> pick(n + 1, 1);
    best[0] = 0;
    for (int i = 1; i <= n; ++i)
        for (int t : sup) {
            if (t > i || t > cap) continue;
            const double c = best[i - t] + t * cost[t];
            if (c < best[i]) { best[i] = c; pick[i] = t; }
        }
    for (int i = n; i > 0; i -= pick[i]) blocks.push_back(pick[i]);
    return blocks;
}
// the same for level g: gamma != 0 takes greedy blocks of the lengths the channel's streaming kernels exist in (the GAM rows,
// tvl1_tbr_kernels.hip); on the register-tile kernel any block up to the margin costs one launch: fewest launches win
inline std::vector<int> tb_plan_level(const Geo &g, int n, int cap, bool gam, const TvKnobs &K)
{
    if (!tile_eligible(g, K) || K.tb_force) return gam ? greedy_blocks(n, cap, {10, 5, 2, 1}) : tb_plan(n, cap, K);
    return greedy_blocks(n, std::min(cap, kTileMaxBlock), {1, 2, 3, 4, 5, 6, 7, 8, 9, 10});
}
// Kernel block sizes of a warp's speculative steps; list 0 / 1 / 2 = the first warp of a large level / of a small one / later warps,
// 3 = levels on the register-tile kernel.  Streaming kernels (MODE 1 instantiations: 10 and 5): a pass of the T = 5 kernel costs half
// of a T = 10 pass on the small pyramid levels and two thirds on a large one (profiles/r02k), and most warps settle within a few
// iterations: only the first warp of a LARGE level starts with the long kernel; after twelve short blocks the plan continues with long
// ones to bound the launch count.  Register tiles: a launch costs its iterations, not its block size, and a converged warp pays ~3 us
// per remaining (empty) launch -- the fewest launches, blocks of the margin (one or two pairs: shorter blocks on tiles of a smaller
// margin own more of their 64 columns x rows, MIFLOW_TILE_FB_BLOCK).  The blocks cover n + 30 iterations so that blocks cut short by
// the device's estimate cannot make the limit unreachable.
inline std::vector<int> tb_spec_plan(int n, int list, int B, const TvKnobs &K)
{
    std::vector<int> blocks;
    const int want = n + (n > 10 ? 30 : n > 1 ? 10 : 0);
    const int tile = (B <= 2 && K.tile_fb_block > 0) ? std::min(K.tile_fb_block, kTileMaxBlock) : kTileMaxBlock;
    for (int sum = 0; sum < want; sum += blocks.back())
        blocks.push_back(list == 3 ? tile : n <= 5 ? 5 : list == 0 ? 10 : blocks.size() < 12 ? 5 : 10);
    return blocks;
}

// ---- band height of the streaming kernels (k_iterate_tbr) --------------------------------------------------------------------------
// Every band wave streams its R rows + 2T rows of halo in whole blocks of P = T + 1 + PF steps.
struct TbBandShape {
    int T, PF, H;
    long long per_band;   // waves per band row: strips x pairs (x the waves of a joined group)
    long long cap;        // resident waves the plan fills: SIMDs x waves per SIMD
    long long simds;      // independent waves only (0 for the joined forms): a workgroup is four consecutive bands of a strip, so with
    int wps;              // nb < 4 bands it has only nb live waves -- at most nb per SIMD where nb < wps (r02z4)
};
inline long long tb_band_wave_steps(int T, int PF, int rows)
{
    const int P = T + 1 + PF;
    return (long long)((rows + 2 * T + P - 1) / P) * P;
}
// executed steps of all bands of one strip: (nb - 1) bands of R rows and the remainder
inline long long tb_band_sum_steps(int T, int PF, int H, int R)
{
    const int nb = (H + R - 1) / R;
    return (nb - 1) * tb_band_wave_steps(T, PF, R) + tb_band_wave_steps(T, PF, H - (nb - 1) * R);
}
// The band COUNT (the round-3 rule, unchanged): the one that minimises rounds x steps of equal bands of ceil(H / nb) rows, rounds =
// ceil(waves / capacity), so that the grid fills the SIMDs in whole rounds while the 2T-row overlap stays small; bands of at least 8 rows.
inline int tb_band_count(const TbBandShape &b)
{
    long long best_cost = -1;
    int best_nb = 1;
    for (int nb = 1; nb <= b.H; ++nb) {
        const int R = (b.H + nb - 1) / nb;
        if (R < 8 && nb > 1) break;
        const long long cap_nb = b.simds > 0 && nb < 4 && nb < b.wps ? b.simds * nb : b.cap;
        const long long rounds = (b.per_band * nb + cap_nb - 1) / cap_nb;
        const long long cost = rounds * tb_band_wave_steps(b.T, b.PF, R);
        if (best_cost < 0 || cost < best_cost) { best_cost = cost; best_nb = nb; }
    }
    return best_nb;
}
inline int tb_band_rows_equal(const TbBandShape &b) { const int nb = tb_band_count(b); return (b.H + nb - 1) / nb; }   // the round-3 height
// The band HEIGHT for that count: equal bands of R0 = ceil(H / nb) rows usually end in the middle of their last block (up to P - 1 steps
// whose rows are never stored).  Any R with ceil(H / R) = nb cuts the same number of bands, the last one taking the remainder: pick the
// R >= R0 that minimises the SUM of the bands' executed steps, among those whose full bands run no more blocks than a band of R0 rows
// does (so the longest wave of the launch is never longer than before: a launch alone on the device cannot get slower); ties -> the
// smallest R.  R0 itself is admissible, so the sum never grows.
inline int tb_band_rows(const TbBandShape &b)
{
    const int nb = tb_band_count(b);
    const int R0 = (b.H + nb - 1) / nb;
    if (nb == 1) return R0;
    const long long tallest = tb_band_wave_steps(b.T, b.PF, R0);
    int best = R0;
    long long best_sum = tb_band_sum_steps(b.T, b.PF, b.H, R0);
    for (int R = R0 + 1; (long long)(nb - 1) * R < b.H; ++R) {   // ceil(H / R) == nb  <=>  (nb - 1) R < H <= nb R
        if (tb_band_wave_steps(b.T, b.PF, R) > tallest) break;
        const long long sum = tb_band_sum_steps(b.T, b.PF, b.H, R);
        if (sum < best_sum) { best_sum = sum; best = R; }
    }
    return best;
}

// ---- the plan ----------------------------------------------------------------------------------------------------------------------

struct TvShape {
    int W, H, B, type;               // frame size, pairs of this lane, input type (MI_8UC1 / MI_32FC1)
    mi_tvl1_params P;
    int lanes;                       // lanes the call runs on
    bool capturing;                  // the stream is being captured into a graph
};

enum class TvForm {
    Blocked,        // fixed work, fast math: T iterations per HBM pass (k_iterate_tbr / the register-tile kernel)
    ExactBlocked,   // fixed work, exact math: blocks of up to 5 iterations (MODE 2), bit-identical to one launch per iteration
    Spec,           // convergence-checked, fast math: speculative blocks (MODE 1) and one settling launch
    PerIter,        // one launch per iteration (convergence-checked exact math, time_block = 1, the median filter with a check)
};

struct TvWarp {
    TvForm form;
    std::vector<int> blocks;   // Blocked: the passes of one outer iteration; ExactBlocked: all passes; Spec: the speculative blocks
    std::vector<TbKernel> run; // what runs each of them (tb_kernel); the three flags below are read from it
    int outer;                 // Blocked: outer iterations (the median filter runs before each); 1 otherwise
    bool on_tiles;             // Spec: the steps run on the register-tile kernel
    bool nograd;               // the warp does not store |grad|^2 (no kernel of `run` reads the plane)
    bool fused;                // the warp runs inside its single pass (k_iterate_tbr FW): no warp launch
    bool warp_launch;          // the warp is enqueued (not fused, not dropped by the MIFLOW_X_SKIP=1 timing experiment)
    bool skip_iterations;      // MIFLOW_X_SKIP=2 timing experiment: the blocked passes are counted, not enqueued
    bool skip_p_last;          // the last pass does not store p (the last pass of a scale: the next scale starts from p = 0)
    bool pack_in_pass;         // the last pass IS the calc's last launch: it stores the flow interleaved into the callers' matrices (no
                               // pack_flow launch).  The last warp of scale 0 only
};

constexpr size_t kNoPlane = (size_t)-1;
struct TvArena {                     // float offsets into the lane's arena block (kNoPlane: the plane does not exist)
    size_t total = 0;                // floats
    std::vector<std::array<size_t, 8>> lv;   // per level: I0, I1, u[set][u1, u2, u3]
    size_t scr[6];                   // full-resolution scratch: median temporaries x 2, I1wx, I1wy, |grad|^2, rho_c
    size_t p[12];                    // [set][p11, p12, p21, p22, p31, p32]
};

struct TvPlan {
    std::vector<Geo> geo;            // levels built; the coarsest may be built but not used
    int used;                        // levels used (the reference's nscales after its 16 px cut)
    TvArena arena;
    int iters;                       // iterations x inner iterations per warp
    int median;                      // median filter size, 0: off
    bool check, spec, hist;          // epsilon > 0: device loop control / as speculative steps / whose first blocks follow the previous calc
    bool fb, fb_poll;                // host feedback between launches (polled flags / copied slots)
    bool fast_warp;                  // the warp's bicubic sums in separable form
    long long Q;                     // control slots per pair
    unsigned long long hist_sig;     // geometry / batch / loop shape the history belongs to
    std::vector<std::vector<TvWarp>> warp;   // [scale][warp] of the used scales
};

// Level sizes: dsize = saturate_cast<int>(ssize * scaleStep) (cudawarping/src/resize.cpp:78); a level below 16 px is built but not
// used (cudaoptflow/src/tvl1flow.cpp:243-247).
inline std::vector<Geo> tv_levels(const mi_tvl1_params &P, int W, int H, int B, int *used)
{
    std::vector<Geo> geo;
    int w = W, h = H;
    *used = 0;
    for (int s = 0; s < P.nscales; ++s) {
        if (s > 0) {
            w = (int)std::lrint(w * P.scale_step);
            h = (int)std::lrint(h * P.scale_step);
            if (w < 1 || h < 1) break;
        }
        geo.push_back(Geo{w, h, (w + 63) / 64 * 64, (long long)((w + 63) / 64 * 64) * h, B});
        if (s > 0 && (w < 16 || h < 16)) break;
        *used = s + 1;
    }
    return geo;
}

// every plane 64-float aligned; u3 / p31 / p32 only when gamma != 0, the median temporaries only with the median filter
inline TvArena tv_arena(const std::vector<Geo> &geo, int B, bool gam, bool med)
{
    TvArena a;
    auto take = [&](size_t nfloats) { const size_t o = a.total; a.total += (nfloats + 63) / 64 * 64; return o; };
    for (const Geo &g : geo) {
        const size_t n = (size_t)g.ps * B;
        std::array<size_t, 8> o;
        o[0] = take(n); o[1] = take(n);
        for (int k = 0; k < 6; ++k) o[2 + k] = (k % 3 == 2 && !gam) ? kNoPlane : take(n);
        a.lv.push_back(o);
    }
    const size_t nfull = (size_t)geo[0].ps * B;
    for (int k = 0; k < 6; ++k) a.scr[k] = (k < 2 && !med) ? kNoPlane : take(nfull);
    for (int k = 0; k < 12; ++k) a.p[k] = (k % 6 >= 4 && !gam) ? kNoPlane : take(nfull);
    return a;
}

// the speculative blocks of a warp once the previous calc's count hprev of it is known (polled host feedback): on tiles, the block
// length = tile margin for the whole warp from a cost model fitted to the traces of profiles/r10 -- a pass costs ~7 us
// (MIFLOW_TILE_FB_MODEL) of launch and hand-over plus (tile lanes) x (10.8 ps of loads and stores + 2.4 ps per iteration), tile
// lanes = pixels x 64 / (64 - 2M) x TR / (TR - 2M), TR = tile rows.  Few iterations or a small level: one block of the margin that just
// holds them; many iterations on a level that fills the device: more, shorter blocks whose tiles own more of their pixels.
inline int spec_tile_block(int hprev, const Geo &g, const TvKnobs &K)
{
    const double px = (double)g.w * g.h * g.batch, TR = (double)tile_rows_for(g, K);
    int best = 10;
    double best_cost = 1e30;
    for (int bl : {4, 7, 10}) {
        const double passes = (double)((hprev + bl - 1) / bl);
        const double lanes = px * 64.0 / (64.0 - 2.0 * bl) * TR / (TR - 2.0 * bl);
        const double cost = passes * (double)K.tile_fb_model + lanes * (passes * 10.8e-6 + (double)hprev * 2.4e-6);
        if (cost < best_cost) { best_cost = cost; best = bl; }
    }
    return best;
}
// bl = 0: the cost model's block length; without the model a first block of at most 4 / 7 iterations runs on tiles of that margin
inline std::vector<int> spec_blocks(const TvWarp &w, const Geo &g, int hprev, const TvKnobs &K, int bl = 0)
{
    std::vector<int> plan = w.blocks;
    if (!w.on_tiles || hprev < 1 || plan.empty()) return plan;
    if (K.tile_fb_model != 0) {
        if (bl <= 0) bl = spec_tile_block(hprev, g, K);
        int total = 0;
        for (int v : plan) total += v;
        plan.assign((size_t)((total + bl - 1) / bl), bl);
    } else if (hprev <= 7) plan[0] = hprev <= 4 ? 4 : 7;
    return plan;
}
// Host feedback's first read-back: behind the launch where the previous warp of this scale stopped (the first warp: where the coarser
// scale's first warp did), or with a count from the previous calc, behind the block in which iteration hprev falls
inline int spec_first_poll(const std::vector<int> &plan, int hprev, int prev_done)
{
    if (hprev <= 0) return std::max(1, prev_done);
    int kq = 0, sum = 0;
    while (kq < (int)plan.size() && (sum += plan[kq]) < hprev) ++kq;
    return std::max(1, std::min(kq + 1, (int)plan.size() - 1));
}
// the first block's length from an earlier warp's count (measured on textured pairs: the second warp of a scale needs about half of the
// first, later warps slightly fewer than their predecessor, the first warp of a scale about 0.7 of the first warp one scale coarser)
inline void spec_hist_fraction(int wp, int *num, int *den)
{
    *num = wp == 0 ? 7 : wp == 1 ? 9 : 4;
    *den = wp == 0 ? 10 : wp == 1 ? 20 : 5;
}

inline TvPlan tv_make_plan(const TvShape &S, const TvKnobs &K)
{
    const mi_tvl1_params &P = S.P;
    const int B = S.B;
    const bool gam = P.gamma != 0.0;
    TvPlan p;
    p.geo = tv_levels(P, S.W, S.H, B, &p.used);
    p.median = P.median_filtering > 1 ? P.median_filtering : 0;
    p.arena = tv_arena(p.geo, B, gam, p.median != 0);
    p.iters = P.iterations * P.inner_iterations;
    p.check = P.epsilon > 0.0 && p.iters > 0;
    p.spec = p.check && !P.exact_math && P.time_block != 1 && !p.median && K.spec != 0;
    p.hist = p.spec && K.tb_hist != 0;
    // host feedback: only where the calc is one lane on the caller's stream (a wait inside lane k would hold up the enqueue of lane
    // k + 1), and never while the stream is captured into a graph (an event synchronise there fails and invalidates the capture)
    p.fb = p.spec && S.lanes == 1 && P.host_feedback >= 0 && (P.host_feedback == 1 || B <= 2) && !S.capturing;
    p.fb_poll = p.fb && K.fb_poll != 0;
    p.fast_warp = !P.exact_math && (K.warp_fast > 0 || (K.warp_fast < 0 && P.semantics == MI_SEM_CUDA_COMPAT));
    p.hist_sig = 1469598103934665603ull;
    for (long long v : {(long long)S.W, (long long)S.H, (long long)B, (long long)p.used, (long long)P.warps, (long long)p.iters, (long long)S.type})
        p.hist_sig = (p.hist_sig ^ (unsigned long long)v) * 1099511628211ull;

    // control slots per pair: one per launch (S, P, X) and one error sum per iteration (E); both index spaces fit max(., .)
    const long long sw = (long long)p.used * P.warps;
    p.Q = sw * p.iters;
    std::vector<int> spec_list[4];   // first warp of a large level / of a small one / later warps / levels on the register-tile kernel
    if (p.spec) {
        long long e_max = 0, l_max = 0;
        for (int k = 0; k < 4; ++k) {
            spec_list[k] = tb_spec_plan(p.iters, k, B, K);
            long long t = 0;
            for (int v : spec_list[k]) t += v;
            e_max = std::max(e_max, t);
            l_max = std::max(l_max, (long long)spec_list[k].size() + 1);
        }
        // the cost-model plan (spec_blocks) rounds a warp's total UP to a multiple of its block length, and the settling launch of a
        // warp indexes one more block: a block of slack per warp (the launch loop checks the bound as well)
        e_max += 2 * (long long)std::max(kTileMaxBlock, kTbMaxBlock);
        p.Q = std::max(sw * e_max, sw * l_max);
    }

    const bool blocked = !p.check && !P.exact_math && P.time_block != 1;
    const bool exact_blocked = !p.check && P.exact_math && P.time_block != 1 && !gam && !p.median && K.exact_tb != 0;
    p.warp.resize(p.used);
    for (int s = 0; s < p.used; ++s) {
        const Geo &g = p.geo[s];
        TvWarp w{};
        w.outer = 1;
        if (blocked) {
            // the optional median filter sits between outer iterations, so blocks never span more than inner_iterations
            w.form = TvForm::Blocked;
            w.outer = p.median ? P.iterations : 1;
            w.blocks = tb_plan_level(g, p.median ? P.inner_iterations : p.iters, P.time_block > 0 ? P.time_block : kTbMaxBlock, gam, K);
            // where every pass can form |grad|^2 itself the warp does not store it (the illumination channel's kernels never read the plane)
            w.nograd = !w.blocks.empty();
            for (int v : w.blocks) w.nograd = w.nograd && (gam || tb_nograd_ok(v, g, K));
            for (int v : w.blocks) w.run.push_back(tb_kernel(TbUse::Fixed, v, g, gam, w.nograd, K));
            w.fused = !gam && w.nograd && w.blocks.size() == 1 && !p.median && K.x_skip == 0 && K.warp_lds == 0 &&
                      tb_fused_ok(w.blocks[0], g, P.semantics, p.fast_warp, K);
            if (w.fused) w.run[0].row = tb_select(TbUse::Fixed, w.blocks[0], false, true, K, P.semantics == MI_SEM_CPU_REF ? 1 : 2);
            w.skip_iterations = K.x_skip == 2;
        } else if (exact_blocked) {
            w.form = TvForm::ExactBlocked;
            const int cap = P.time_block > 0 ? std::min(P.time_block, kTbExactMaxBlock) : kTbExactMaxBlock;
            for (int left = p.iters; left > 0; left -= w.blocks.back()) w.blocks.push_back(std::min(left, cap));
            for (int v : w.blocks) w.run.push_back(tb_kernel(TbUse::Exact, v, g, false, false, K));
        } else if (p.spec) {
            w.form = TvForm::Spec;
            w.nograd = gam || tb_spec_nograd_ok(g, K);
        } else
            w.form = TvForm::PerIter;
        p.warp[s].assign(P.warps, w);
        for (int wp = 0; wp < P.warps; ++wp) {
            TvWarp &x = p.warp[s][wp];
            if (x.form == TvForm::Spec) {
                // (all steps of a level run on the tiles or none does: every list's blocks are within the tile margin)
                x.on_tiles = tb_kernel(TbUse::Spec, kTileMaxBlock, g, gam, x.nograd, K).tile;
                x.blocks = spec_list[x.on_tiles ? 3 : wp > 0 ? 2 : ((double)g.w * g.h * B >= kLargeLevel ? 0 : 1)];
                for (int v : x.blocks) x.run.push_back(tb_kernel(TbUse::Spec, v, g, gam, x.nograd, K));
            }
            x.warp_launch = !x.fused && !(K.x_skip == 1 && wp > 0);
            x.skip_p_last = x.form == TvForm::Blocked && K.tb_skip_p && wp == P.warps - 1 && !p.median;
            // the flow straight into the callers' matrices: the fixed-work blocked form whose last pass runs on a streaming row that
            // has the interleaved store (two channels, one pixel per lane); register tiles, the speculative steps, the fused warp and
            // calcs that read the callers' matrices first (use_initial_flow) keep pack_flow
            if (s == 0 && x.skip_p_last && !gam && !x.fused && !x.skip_iterations && !P.use_initial_flow && !x.blocks.empty())
                x.pack_in_pass = K.tb_il != 0 && x.run.back().row && tb_il_form(*x.run.back().row);
        }
    }
    return p;
}

}  // namespace tvl1
}  // namespace mi
