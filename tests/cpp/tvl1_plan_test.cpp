// The plan of one lane's TV-L1 calc (csrc/tvl1_plan.h): levels, arena layout, the calc's control features and slot count, and each
// warp's iteration form and blocks.  Plain C++, no device.  Level sizes follow cudaoptflow/src/tvl1flow.cpp:238-266.
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
    k.tb_force = false; k.tb_nograd = 1; k.tb_jw = 2; k.tb_ppl = -1; k.tb_jw_spec = 1; k.tb_fw = 0;
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

int main()
{
    const TvKnobs K = knobs();
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
