// The plan of one lane's TV-L1 calc (csrc/tvl1_plan.h): levels, arena layout, the calc's control features and slot count, and each
// warp's iteration form, blocks and the kernel of every block; the table of the streaming kernels (csrc/tvl1_tb_table.h) and its
// selection rule against the rules they replaced.  Plain C++, no device (also compiled with -DMIFLOW_EXPERIMENTS: the experiments
// build's rows and switches).  Level sizes follow cudaoptflow/src/tvl1flow.cpp:238-266.
#include "tvl1_plan.h"
#include <cstdio>

using namespace mi::tvl1;

static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); ++fails; } } while (0)

// the release library's knobs (tuning defaults; tile shapes 64 and 48 rows)
static TvKnobs knobs()
{
    TvKnobs k{};
    k.tile_maxpx = 2300000; k.tile_spec = 1; k.tile_variant = -1; k.tile_small_wgs = 1024; k.tile_variants = 2;
    k.tile_rows[0] = 64; k.tile_rows[1] = 48; k.tile_fb_block = 10; k.tile_fb_model = 7;
    k.tb_force = false; k.tb_nograd = 1; k.tb_jw = 2; k.tb_ppl = k.tb_wps = k.tb_pf = -1; k.tb_jw_spec = 1; k.tb_fw = 0; k.tb_il = 1;
    k.tb_skip_p = 1; k.tb_hist = 1; k.spec = 1; k.exact_tb = 1; k.fb_poll = 1; k.fb_ahead = 1; k.warp_fast = -1;
    return k;
}
static mi_tvl1_params params(int iterations = 300, double eps = 0.01)
{
    mi_tvl1_params p{};
    p.tau = 0.25; p.lambda = 0.15; p.theta = 0.3; p.epsilon = eps; p.scale_step = 0.8; p.nscales = 5; p.warps = 5;
    p.iterations = iterations; p.inner_iterations = 1; p.median_filtering = 1; p.semantics = MI_SEM_CPU_REF;
    return p;
}
static TvPlan plan(int W, int H, int B, const mi_tvl1_params &P, const TvKnobs &K = knobs(), int lanes = 1)
{
    return tv_make_plan(TvShape{W, H, B, MI_32FC1, P, lanes, false}, K);
}
static int sum(const std::vector<int> &v) { int t = 0; for (int x : v) t += x; return t; }

// Worst case of the speculative launch loop (lane_calc run_spec): every warp runs all its launches; per launch the error-sum slots
// e_next .. e_next + T and the launch slot q must lie inside Q (the loop's MI_REQUIRE).
static bool spec_slots_fit(const TvPlan &p, const TvKnobs &K, int hprev, int bl)
{
    long long e_next = 0, q = 0;
    for (size_t s = 0; s < p.warp.size(); ++s)
        for (const TvWarp &w : p.warp[s]) {
            const std::vector<int> blocks = spec_blocks(w, p.geo[s], hprev, K, bl);
            for (size_t k = 0; k <= blocks.size(); ++k) {
                const bool last = k == blocks.size();
                const int T = last ? blocks.back() : blocks[k];
                if (e_next + T > p.Q || q >= p.Q) return false;
                ++q;
                if (!last) e_next += T;
            }
        }
    return true;
}

static void check_arena(const TvPlan &p, int B, bool gam, bool med)
{
    std::vector<std::pair<size_t, size_t>> planes;   // [offset, end)
    for (size_t l = 0; l < p.geo.size(); ++l)
        for (int k = 0; k < 8; ++k) {
            const bool u3 = k == 4 || k == 7;
            CHECK((p.arena.lv[l][k] == kNoPlane) == (u3 && !gam));
            if (p.arena.lv[l][k] != kNoPlane) planes.push_back({p.arena.lv[l][k], p.arena.lv[l][k] + (size_t)p.geo[l].ps * B});
        }
    const size_t nfull = (size_t)p.geo[0].ps * B;
    for (int k = 0; k < 6; ++k) {
        CHECK((p.arena.scr[k] == kNoPlane) == (k < 2 && !med));
        if (p.arena.scr[k] != kNoPlane) planes.push_back({p.arena.scr[k], p.arena.scr[k] + nfull});
    }
    for (int k = 0; k < 12; ++k) {
        CHECK((p.arena.p[k] == kNoPlane) == (k % 6 >= 4 && !gam));
        if (p.arena.p[k] != kNoPlane) planes.push_back({p.arena.p[k], p.arena.p[k] + nfull});
    }
    std::sort(planes.begin(), planes.end());
    for (size_t i = 0; i < planes.size(); ++i) {
        CHECK(planes[i].first % 64 == 0);
        CHECK(planes[i].second <= (i + 1 < planes.size() ? planes[i + 1].first : p.arena.total));
    }
    CHECK(p.arena.total % 64 == 0);
}

// ---- the kernel tables and the rules that walked them before there was one table and tb_select (tvl1_tbr_kernels.hip up to round 20:
// g_tbr*, g_spec*, g_exact; tbr_pick, the branches of iterate_tb / iterate_tb_spec / iterate_tb_exact, tb_kernel_exists,
// tb_interleave_mask; the LDS size of launch_tbr and of plan_band_rows, their strip count), restated
namespace old {
struct E { int MODE, T, PPL, WPS, PF, PLAN, JW; bool NG, P16; int FW; bool GAM; };
typedef std::vector<E> Tab;
#ifdef MIFLOW_EXPERIMENTS
static const bool exp_build = true;
#else
static const bool exp_build = false;
#endif
static Tab cat(Tab a, const Tab &b, bool on = true) { if (on) a.insert(a.end(), b.begin(), b.end()); return a; }
static const Tab tbr_jw = cat(cat({}, {{0, 10, 1, 3, 2, 3, 1}, {0, 10, 1, 4, 2, 3, 3}, {0, 10, 1, 4, 2, 3, 4}}, exp_build), {{0, 10, 1, 4, 2, 3, 2}});
static const E tbr_ng = {0, 10, 1, 4, 2, 3, 2, true}, tbr_ng16 = {0, 10, 1, 4, 2, 3, 2, true, true};
static const Tab tbr_fw = {{0, 10, 1, 4, 2, 2, 2, true, false, 1}, {0, 10, 1, 4, 2, 2, 2, true, false, 2}};
static const Tab tbr_gam = {{0, 10, 1, 3, 1, 3, 2, true, false, 0, true}, {0, 5, 1, 4, 2, 3, 2, true, false, 0, true},
                            {0, 2, 1, 6, 2, 6, 0, true, false, 0, true}, {0, 1, 1, 8, 2, 8, 0, true, false, 0, true}};
static const Tab spec_gam = {{1, 10, 1, 2, 2, 2, 2, true, false, 0, true}, {1, 5, 1, 3, 2, 2, 2, true, false, 0, true}};
static const Tab tbr = cat({{0, 10, 1, 4, 2, 3, 0}, {0, 8, 2, 2, 2, 2, 0}, {0, 6, 1, 5, 2, 3, 0}, {0, 5, 2, 3, 2, 3, 0}, {0, 4, 2, 3, 2, 3, 0},
                            {0, 3, 1, 7, 2, 6, 0}, {0, 2, 1, 8, 2, 8, 0}, {0, 1, 1, 8, 2, 8, 0}},
                           {{0, 10, 2, 2, 2, 2, 0}, {0, 8, 1, 4, 2, 2, 0}, {0, 6, 2, 3, 2, 3, 0}}, exp_build);
static const Tab spec = {{1, 10, 1, 3, 2, 2, 0}, {1, 5, 1, 4, 2, 2, 0}}, spec_jw = {{1, 10, 1, 3, 2, 2, 2}, {1, 5, 1, 4, 2, 2, 2}};
static const Tab spec_jw_ng = {{1, 10, 1, 3, 2, 2, 2, true}, {1, 5, 1, 4, 2, 2, 2, true}};
static const Tab exact = {{2, 5, 1, 4, 2, 3, 0}, {2, 4, 1, 4, 2, 3, 0}, {2, 3, 1, 5, 2, 4, 0}, {2, 2, 1, 6, 2, 4, 0}, {2, 1, 1, 8, 2, 4, 0}};

static const E *of_T(const Tab &t, int T) { const E *r = nullptr; for (const E &e : t) if (e.T == T) r = &e; return r; }
static const E *tbr_pick(int T, const TvKnobs &K)
{
    if (K.tb_jw && K.tb_ppl < 0)
        for (const E &e : tbr_jw) if (e.T == T && e.JW == K.tb_jw) return &e;
    const E *def = nullptr;
    for (const E &e : tbr) {
        if (e.T != T) continue;
        if (!def) def = &e;
        if (e.PPL == K.tb_ppl && e.WPS == K.tb_wps && e.PF == K.tb_pf) { def = &e; break; }
    }
    return def;
}
static bool kernel_exists(int kind, int T, bool gam, bool nograd, const TvKnobs &K)
{
    switch (kind) {
    case 0: return gam ? of_T(tbr_gam, T) != nullptr : nograd ? T == tbr_ng.T : tbr_pick(T, K) != nullptr;
    case 1:
        if (nograd) return false;
        if (!gam) return of_T(tbr, T) != nullptr;
        return of_T(tbr_gam, T) && of_T(tbr_gam, T)->JW == 0;
    case 2: return !gam && !nograd && of_T(exact, T);
    default: return gam ? of_T(spec_gam, T) != nullptr : of_T(spec_jw_ng, T) != nullptr;
    }
}
// what the stage-level entry launched for use = fixed / indep / exact / spec (kind 0..3) with the streaming kernels forced: nothing
// where tb_kernel_exists said no, else the entry of the dispatcher's branch
static const E *launched(int kind, int T, bool gam, bool nograd, const TvKnobs &K)
{
    if (!kernel_exists(kind, T, gam, nograd, K)) return nullptr;
    if (kind == 2) return of_T(exact, T);                                   // iterate_tb_exact
    if (kind == 3) {                                                        // iterate_tb_spec
        if (gam) return of_T(spec_gam, T);
        if (nograd || !exp_build) return of_T(spec_jw_ng, T);
        return K.tb_jw >= 2 && K.tb_jw_spec ? of_T(spec_jw, T) : of_T(spec, T);
    }
    if (gam) return of_T(tbr_gam, T);                                       // iterate_tb
    if (kind == 1) { for (const E &e : tbr) if (e.T == T) return &e; return nullptr; }
    if (nograd) return exp_build && K.tb_p16 ? &tbr_ng16 : &tbr_ng;
    return tbr_pick(T, K);
}
static unsigned interleave_mask(const TvKnobs &K)
{
    unsigned m = 0;
    for (int T = 1; T <= kTbMaxBlock; ++T) {
        const E *e = tbr_pick(T, K);
        if (e && e->PPL == 1 && e->JW == 0) m |= 1u << T;
    }
    return m | 1u << 31;   // (tb_il_form of g_tbr_ng)
}
static int nw(const TbRow &r) { return r.JW == 3 ? 8 : 4; }
static int handover_bytes(const TbRow &r)
{
    const int T = r.T, xarea2 = 2 * T * (r.GAM ? 32 : 16);
    return r.JW >= 2 ? nw(r) * xarea2 + (r.JW == 4 ? 64 * 8 + 2 * (2 * T * 16) + 64 : 0) : r.JW ? 4 * (2 * T * 32 + 2 * T * 32 + 64 * 8) : 0;
}
static size_t launch_lds(const TbRow &r)    // launch_tbr (FW_STAGE = 0)
{
    return (size_t)nw(r) * (r.T > 2 ? r.T - 1 : 1) * 256 * r.PPL * sizeof(float) + handover_bytes(r) + (r.FW ? (nw(r) * 4 * 192 + 128) * sizeof(float) : 0);
}
static int planner_wps(const TbRow &r)      // plan_band_rows: no fused-warp term
{
    const int blocks = (160 * 1024) / ((r.T > 2 ? r.T - 1 : 1) * nw(r) * 256 * r.PPL * 4 + handover_bytes(r)) * nw(r) / 4;
    return std::min(r.PLAN, blocks);
}
static int strips(const TbRow &r, int w)
{
    const int M = (r.T + r.PPL - 1) / r.PPL * r.PPL, LW = (r.JW ? 64 * nw(r) : 64) * r.PPL;
    return w <= LW - M ? 1 : 1 + (w - (LW - M) + (LW - 2 * M) - 1) / (LW - 2 * M);
}
}  // namespace old

static bool same(const old::E *e, const TbRow *r)
{
    if (!e || !r) return !e && !r;
    return e->MODE == r->MODE && e->T == r->T && e->PPL == r->PPL && e->WPS == r->WPS && e->PF == r->PF && e->PLAN == r->PLAN && e->JW == r->JW &&
           e->NG == r->NG && e->P16 == r->P16 && e->FW == r->FW && e->GAM == r->GAM;
}
static void check_selection(const TvKnobs &K)
{
    const TbUse use[4] = {TbUse::Fixed, TbUse::Indep, TbUse::Exact, TbUse::Spec};
    for (int kind = 0; kind < 4; ++kind)
        for (int T = 1; T <= 10; ++T)
            for (int gam = 0; gam < 2; ++gam)
                for (int ng = 0; ng < 2; ++ng) {
                    const bool ok = same(old::launched(kind, T, gam, ng, K), tb_select(use[kind], T, gam, ng, K));
                    if (!ok) std::printf("selection differs: kind %d T %d gam %d nograd %d jw %d jw_spec %d variant %d,%d,%d p16 %d\n", kind, T, gam, ng,
                                         K.tb_jw, K.tb_jw_spec, K.tb_ppl, K.tb_wps, K.tb_pf, K.tb_p16);
                    CHECK(ok);
                }
    for (int fw = 1; fw <= 2; ++fw)   // iterate_tb_fused: g_tbr_fw[semantics == MI_SEM_CPU_REF ? 0 : 1], experiments build only
        CHECK(same(old::exp_build ? &old::tbr_fw[fw - 1] : nullptr, tb_select(TbUse::Fixed, 10, false, true, K, fw)));
}
// the plan's choice for the calc's last pass against the mask it was read from; what a warp leaves out, its kernels do not read
static void check_pack_in_pass(const TvPlan &p, const TvKnobs &K, bool may)
{
    for (size_t s = 0; s < p.warp.size(); ++s)
        for (size_t wp = 0; wp < p.warp[s].size(); ++wp) {
            const TvWarp &w = p.warp[s][wp];
            CHECK(w.run.size() == w.blocks.size());
            for (const TbKernel &k : w.run) CHECK(k.tile || k.row);
            if (w.nograd) for (const TbKernel &k : w.run) CHECK(k.tile ? p.arena.lv[0][4] != kNoPlane : k.row->NG);
            bool expect = false;
            if (may && s == 0 && wp + 1 == p.warp[s].size() && w.form == TvForm::Blocked && !w.fused && !w.blocks.empty()) {
                const int tl = w.blocks.back();
                const unsigned mask = K.tb_il ? old::interleave_mask(K) : 0u;
                expect = !runs_on_tiles(p.geo[0], tl, K) && ((w.nograd ? mask >> 31 : mask >> tl) & 1u) != 0;
            }
            CHECK(w.pack_in_pass == expect);
        }
}

int main()
{
    const TvKnobs K = knobs();
    {   // one table, one rule: the same row as the old tables and dispatchers gave, or none on both sides
        check_selection(K);
#ifdef MIFLOW_EXPERIMENTS
        const int variants[][3] = {{-1, -1, -1}, {2, 2, 2}, {1, 4, 2}, {2, 3, 2}, {1, 8, 2}, {1, 4, 3}};
        for (int jw = 0; jw <= 4; ++jw)
            for (int jws = 0; jws < 2; ++jws)
                for (const auto &v : variants)
                    for (int p16 = 0; p16 < 2; ++p16) {
                        TvKnobs X = K;
                        X.tb_jw = jw; X.tb_jw_spec = jws; X.tb_ppl = v[0]; X.tb_wps = v[1]; X.tb_pf = v[2]; X.tb_p16 = p16;
                        check_selection(X);
                    }
#endif
        // every row: the dynamic LDS of its launch, the waves per SIMD its planner fills (the old planner's size lacked the fused warp's
        // inboxes: the cap is the same with them), its strips
        for (const TbRow &r : kTbRows) {
            CHECK(tb_lds_bytes(r) == old::launch_lds(r));
            CHECK(tb_plan_wps(r) == old::planner_wps(r));
            for (int w = 1; w <= 4096; ++w) CHECK(tb_strips(r, w) == old::strips(r, w));
        }
        CHECK(kTbRowCount == (old::exp_build ? 36 : 23));
    }
    {   // the calc's last pass stores the flow interleaved (tests/test_tvl1_interleaved_store.py): scale 0, last warp, fixed work, two
        // channels, a streaming row of one pixel per lane -- 1283 x 961 x 2 pairs, N = 10 (one T = 10 pass without a |grad|^2 plane) and
        // N = 7 (1 + 6, independent waves); a single pair runs on the tiles; every other N against the old mask
        CHECK(plan(1283, 961, 2, params(10, 0.0), K, 2).warp[0][4].pack_in_pass && plan(1283, 961, 2, params(10, 0.0), K, 2).warp[0][4].nograd);
        const TvPlan p7 = plan(1283, 961, 2, params(7, 0.0), K, 2);
        CHECK(p7.warp[0][4].blocks == (std::vector<int>{1, 6}) && p7.warp[0][4].pack_in_pass && !p7.warp[0][4].nograd);
        CHECK(!p7.warp[0][3].pack_in_pass && !p7.warp[1][4].pack_in_pass);
        CHECK(!plan(1283, 961, 1, params(10, 0.0)).warp[0][4].pack_in_pass);
        CHECK(!plan(1283, 961, 2, params(8, 0.0)).warp[0][4].pack_in_pass && !plan(1283, 961, 2, params(5, 0.0)).warp[0][4].pack_in_pass);
        std::vector<TvKnobs> Ks = {K};
        Ks.push_back(K); Ks.back().tb_nograd = 0;
        Ks.push_back(K); Ks.back().tb_il = 0;
        Ks.push_back(K); Ks.back().tb_skip_p = 0;
        Ks.push_back(K); Ks.back().tb_jw = 0;
        Ks.push_back(K); Ks.back().tb_force = true;
        for (const TvKnobs &X : Ks)
            for (int n = 1; n <= 23; ++n)
                for (int B : {1, 2, 16}) {
                    check_pack_in_pass(plan(1283, 961, B, params(n, 0.0), X), X, X.tb_skip_p != 0);
                    mi_tvl1_params P = params(n, 0.0);
                    P.gamma = 1.0;
                    check_pack_in_pass(plan(1283, 961, B, P, X), X, false);
                    P = params(n, 0.0);
                    P.use_initial_flow = 1;
                    check_pack_in_pass(plan(1283, 961, B, P, X), X, false);
                    P = params(n, 0.0);
                    P.median_filtering = 5;
                    check_pack_in_pass(plan(1283, 961, B, P, X), X, false);
                    P = params(n, 0.0);
                    P.exact_math = 1;
                    check_pack_in_pass(plan(1283, 961, B, P, X), X, false);
                    check_pack_in_pass(plan(1283, 961, B, params(n, 0.01), X), X, false);
                }
    }
    {   // level sizes and the usable-scale cut (round half to even of w x 0.8; a level below 16 px is built, not used)
        struct { int W, H, nscales, built, used, w_last, h_last; } cases[] = {
            {1920, 1080, 5, 5, 5, 786, 442}, {3840, 2160, 5, 5, 5, 1573, 885}, {640, 480, 5, 5, 5, 262, 197},
            {77, 101, 5, 5, 5, 32, 42}, {120, 160, 6, 6, 6, 40, 53}, {40, 30, 5, 4, 3, 21, 15}, {20, 20, 5, 3, 2, 13, 13}};
        for (const auto &c : cases) {
            mi_tvl1_params P = params();
            P.nscales = c.nscales;
            const TvPlan p = plan(c.W, c.H, 1, P);
            CHECK((int)p.geo.size() == c.built && p.used == c.used && (int)p.warp.size() == c.used);
            CHECK(p.geo.back().w == c.w_last && p.geo.back().h == c.h_last);
            for (const Geo &g : p.geo) CHECK(g.ld % 64 == 0 && g.ld >= g.w && g.ps == (long long)g.ld * g.h && g.batch == 1);
        }
        const TvPlan p = plan(1920, 1080, 1, params());
        const int w[5] = {1920, 1536, 1229, 983, 786}, h[5] = {1080, 864, 691, 553, 442};
        for (int s = 0; s < 5; ++s) CHECK(p.geo[s].w == w[s] && p.geo[s].h == h[s]);
    }
    {   // arena: planes 64-float aligned, disjoint, u3 / p3x with gamma only, median temporaries with the filter only
        for (int gam = 0; gam < 2; ++gam)
            for (int med = 0; med < 2; ++med) {
                mi_tvl1_params P = params();
                P.gamma = gam; P.median_filtering = med ? 5 : 1;
                for (int B : {1, 3, 16}) check_arena(plan(77 + 640 * gam, 101 + 480 * med, B, P), B, gam, med);
            }
    }
    {   // the headline: N = 10, epsilon = 0, 1080p x 32 per lane -- fixed work, blocked; one pass of T = 10 per warp on the streaming
        // levels (no |grad|^2 plane stored); two pairs: the register-tile kernel below 2.3 Mpx x pairs (the plane is stored)
        const TvPlan p = plan(1920, 1080, 32, params(10, 0.0), K, 2);
        CHECK(!p.check && !p.spec && !p.fb && !p.hist && p.Q == 5 * 5 * 10);
        for (int s = 0; s < 5; ++s)
            for (int wp = 0; wp < 5; ++wp) {
                const TvWarp &w = p.warp[s][wp];
                CHECK(w.form == TvForm::Blocked && w.outer == 1 && w.blocks == std::vector<int>{10});
                CHECK(w.nograd == !tile_eligible(p.geo[s], K) && !w.fused && w.warp_launch && !w.skip_iterations);
                CHECK(w.skip_p_last == (wp == 4));
            }
        CHECK(!tile_eligible(p.geo[4], K));
        const TvPlan p2 = plan(1920, 1080, 2, params(10, 0.0));
        CHECK(p2.warp[0][0].nograd && !tile_eligible(p2.geo[0], K) && !p2.warp[4][0].nograd && tile_eligible(p2.geo[4], K));
        // N = 13: the cost model's passes on the streaming levels, greedy blocks of the margin on tiles
        const TvPlan q = plan(1920, 1080, 2, params(13, 0.0));
        CHECK(sum(q.warp[0][0].blocks) == 13 && !q.warp[0][0].nograd);
        CHECK(q.warp[4][0].blocks == (std::vector<int>{10, 3}));
    }
    {   // class defaults (300 iterations, epsilon 0.01): speculative steps; 1 / 2 pairs with host feedback, 64 pairs without
        for (int B : {1, 2, 64}) {
            const TvPlan p = plan(1920, 1080, B, params());
            CHECK(p.check && p.spec && p.hist && p.fb == (B <= 2) && p.fb_poll == (B <= 2));
            for (int s = 0; s < 5; ++s)
                for (int wp = 0; wp < 5; ++wp) {
                    const TvWarp &w = p.warp[s][wp];
                    CHECK(w.form == TvForm::Spec && w.warp_launch && !w.fused && !w.skip_p_last);
                    CHECK(w.on_tiles == tile_eligible(p.geo[s], K) && w.nograd == !w.on_tiles);
                    CHECK(sum(w.blocks) >= 330);
                    if (w.on_tiles) CHECK(w.blocks == std::vector<int>(33, 10));
                    else if (wp == 0 && (double)p.geo[s].w * p.geo[s].h * B >= kLargeLevel) CHECK(w.blocks == std::vector<int>(33, 10));
                    else CHECK(w.blocks[0] == 5 && w.blocks[11] == 5 && w.blocks[12] == 10);
                }
            for (int hprev = 1; hprev <= 300; ++hprev)
                for (int bl : {0, 4, 7, 10}) CHECK(spec_slots_fit(p, K, hprev, bl));
            CHECK(spec_slots_fit(p, K, 0, 0));
            CHECK(!plan(1920, 1080, B, params(), K, 2).fb);            // two lanes: no host feedback
        }
        mi_tvl1_params P = params();
        P.host_feedback = 1;
        CHECK(plan(640, 480, 8, P).fb);
        P.host_feedback = -1;
        CHECK(!plan(640, 480, 1, P).fb);
        CHECK(!tv_make_plan(TvShape{640, 480, 1, MI_8UC1, params(), 1, true}, K).fb);   // a stream under capture never waits
        // the first read-back: behind the block in which iteration hprev falls; without a count, where the previous warp stopped
        const std::vector<int> b = {5, 5, 5, 10};
        CHECK(spec_first_poll(b, 0, 2) == 2 && spec_first_poll(b, 0, -1) == 1 && spec_first_poll(b, 7, 2) == 2 && spec_first_poll(b, 40, 2) == 3);
        int num, den;
        spec_hist_fraction(0, &num, &den); CHECK(num == 7 && den == 10);
        spec_hist_fraction(1, &num, &den); CHECK(num == 9 && den == 20);
        spec_hist_fraction(3, &num, &den); CHECK(num == 4 && den == 5);
    }
    {   // few iterations: the speculative lists and the slot bound for every small count
        for (int it = 1; it <= 40; ++it)
            for (int B : {1, 2, 64}) {
                const TvPlan p = plan(640, 480, B, params(it));
                for (int hprev = 1; hprev <= it; ++hprev)
                    for (int bl : {4, 7, 10}) CHECK(spec_slots_fit(p, K, hprev, bl));
            }
    }
    {   // gamma 1: fixed work in the channel's block set (10 / 5 / 2 / 1) on streaming levels; speculative steps with defaults
        mi_tvl1_params P = params(17, 0.0);
        P.gamma = 1.0;
        const TvPlan p = plan(1920, 1080, 16, P);
        CHECK(p.warp[0][0].form == TvForm::Blocked && p.warp[0][0].blocks == (std::vector<int>{10, 5, 2}) && p.warp[0][0].nograd);
        P.iterations = 300; P.epsilon = 0.01;
        const TvPlan q = plan(1920, 1080, 16, P);
        CHECK(q.spec && q.warp[0][0].form == TvForm::Spec && q.warp[0][0].nograd && q.warp[4][0].nograd);
    }
    {   // exact math: fixed work in blocks of 5 (time_block caps them); with the check one launch per iteration
        mi_tvl1_params P = params(12, 0.0);
        P.exact_math = 1;
        CHECK(plan(640, 480, 1, P).warp[0][0].form == TvForm::ExactBlocked && plan(640, 480, 1, P).warp[0][0].blocks == (std::vector<int>{5, 5, 2}));
        P.time_block = 3;
        CHECK(plan(640, 480, 1, P).warp[0][0].blocks == (std::vector<int>{3, 3, 3, 3}));
        P.epsilon = 0.01;
        const TvPlan p = plan(640, 480, 1, P);
        CHECK(p.check && !p.spec && p.warp[0][0].form == TvForm::PerIter && p.Q == 5 * 5 * 12);
    }
    {   // time_block = 1: one launch per iteration, with and without the check
        mi_tvl1_params P = params(10, 0.0);
        P.time_block = 1;
        CHECK(plan(1920, 1080, 2, P).warp[0][0].form == TvForm::PerIter);
        P.epsilon = 0.01;
        CHECK(plan(1920, 1080, 2, P).warp[0][0].form == TvForm::PerIter && !plan(1920, 1080, 2, P).spec);
    }
    {   // median 5, inner iterations 3: fixed work in outer iterations of one inner block (the filter between them), p stored everywhere
        mi_tvl1_params P = params(10, 0.0);
        P.median_filtering = 5; P.inner_iterations = 3;
        const TvPlan p = plan(640, 480, 1, P);
        CHECK(p.median == 5 && p.iters == 30);
        const TvWarp &w = p.warp[0][4];
        CHECK(w.form == TvForm::Blocked && w.outer == 10 && w.blocks == std::vector<int>{3} && !w.skip_p_last && !w.nograd);
        P.epsilon = 0.01;
        CHECK(plan(640, 480, 1, P).warp[0][0].form == TvForm::PerIter);
    }
    {   // experiment switches: the warp fused into its single pass (CPU class, tap-by-tap sums), the timing experiments
        TvKnobs X = K;
        X.tb_fw = 1;
        const TvPlan p = plan(1920, 1080, 2, params(10, 0.0), X);
        CHECK(p.warp[0][0].fused && !p.warp[0][0].warp_launch && !p.warp[4][0].fused && p.warp[4][0].warp_launch);
        X = K;
        X.x_skip = 1;
        CHECK(plan(640, 480, 1, params(10, 0.0), X).warp[0][0].warp_launch && !plan(640, 480, 1, params(10, 0.0), X).warp[0][1].warp_launch);
        X.x_skip = 2;
        CHECK(plan(640, 480, 1, params(10, 0.0), X).warp[0][0].skip_iterations);
        X = K;
        X.spec = 0;
        CHECK(plan(640, 480, 1, params()).spec && !plan(640, 480, 1, params(), X).spec);
        X.tile_maxpx = 0;
        CHECK(!plan(160, 120, 1, params(), X).warp[4][0].on_tiles);
    }
    if (fails) return 1;
    std::printf("tvl1_plan_test: ok\n");
    return 0;
}
