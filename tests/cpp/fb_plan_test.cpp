// The plan of a mi_farneback_calc_batch call (csrc/fb_plan.h): levels, geometry, the form rules, the scratch layout and the ordered launch
// list.  Plain C++, no device.
// Geometry follows FarnebackOpticalFlowImpl::calcImpl (cudaoptflow/src/farneback.cpp:330-340 level crop, :374-395 per-level sizes).
#include "fb_plan.h"
#include <cstdio>

using namespace mi::fb;

static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); ++fails; } } while (0)

static FbKnobs knobs(int fuse = -1, int pair = -1, int mb = 240, int chains = 2, bool it2 = true)
{
    FbKnobs k;   // (the switches of the form rules keep their release defaults)
    k.fuse = fuse; k.pair = pair; k.group_mb = mb; k.chains = chains; k.simds = 1024; k.iterate2_ok = it2;
    return k;
}

// ---- (a) exact launch lists: what a list is compared on
struct E { int op, level, form, chain; };
static void rep(std::vector<E> &v, int n, E e) { for (int i = 0; i < n; ++i) v.push_back(e); }
static bool same_list(const FbPlan &p, const std::vector<E> &want, const char *name)
{
    bool ok = p.launches.size() == want.size();
    for (size_t i = 0; ok && i < want.size(); ++i) {
        const FbLaunch &l = p.launches[i];
        ok = l.op == want[i].op && l.level == want[i].level && l.form == want[i].form && l.chain == want[i].chain;
        if (!ok) std::printf("%s: entry %zu is op %d level %d form %d chain %d, expected op %d level %d form %d chain %d\n", name, i, l.op, l.level, l.form,
                             l.chain, want[i].op, want[i].level, want[i].form, want[i].chain);
    }
    if (p.launches.size() != want.size()) std::printf("%s: %zu entries, expected %zu\n", name, p.launches.size(), want.size());
    return ok;
}

// ---- (b) the invariants of one plan.  The host twin of the poison test: every plane kind of every pair carries the level it was last
// written for, by which chain and in which fork / join epoch; an entry may read only what an earlier entry wrote for that level, and
// between a fork and its join only what its own chain wrote there.
enum { P_FRAMES, P_BLURRED, P_LVL, P_R, P_M, P_BUFM, P_FLOW, P_PYR = P_FLOW + 3, P_KINDS = P_PYR + 2 * 40 };
struct Mark { int level = -1, chain = 0, epoch = 0; };
struct Model {
    const FbPlan &p; const FbShape &s;
    std::vector<Mark> m;
    int epoch = 0, bad = 0;
    Model(const FbPlan &p_, const FbShape &s_) : p(p_), s(s_), m((size_t)s_.B * P_KINDS) {}
    int slot(const FbLevel &L) const { for (int a = 0; a < 3; ++a) if (L.flow == p.lay.flow[a]) return P_FLOW + a; return -1; }
    int img(int level, int f) const   // the plane kind behind lv[level].img[f]
    {
        const long long o = p.lv[level].img[f] - f * p.lay.pn;
        if (s.fast_pyramids) return level ? P_PYR + 2 * level + f : P_FRAMES;
        return o == p.lay.blurred ? P_BLURRED : o == p.lay.lvl ? P_LVL : -1;
    }
    void wr(const FbLaunch &l, int kind, int level) { if (kind < 0) { ++bad; return; } for (int b = l.b0; b < l.b0 + l.nb; ++b) m[(size_t)b * P_KINDS + kind] = Mark{level, l.chain, epoch}; }
    void rd(const FbLaunch &l, int kind, int level, bool forked)
    {
        if (kind < 0) { ++bad; return; }
        for (int b = l.b0; b < l.b0 + l.nb; ++b) {
            const Mark &k = m[(size_t)b * P_KINDS + kind];
            if (k.level != level || (forked && k.epoch == epoch && k.chain != l.chain)) ++bad;
        }
    }
};

static void check_invariants(const FbShape &s, const FbKnobs &K)
{
    const FbPlan p = fb_make_plan(s, K);
    const FbLayout &A = p.lay;
    const int before = fails;
    // the layout: 34 planes in this order, nothing past the block; the adjacency the two-frame launches rely on
    const long long start[10] = {A.frames, A.blurred, A.lvl, A.R, A.M, A.bufM, A.flow[0], A.flow[1], A.flow[2], A.pyr}, planes[10] = {2, 2, 2, 10, 5, 5, 2, 2, 2, 2};
    CHECK(A.frames == 0 && A.pn >= (long long)s.W * s.H);
    for (int i = 0; i < 10; ++i) CHECK(start[i] + planes[i] * A.pn == (i < 9 ? start[i + 1] : A.bs));
    long long pyr_end = A.pyr;
    for (int k = 0; k <= p.levels; ++k) {
        const FbLevel &L = p.lv[k];
        const long long n = (long long)L.ld * L.h;
        CHECK(n <= A.pn && L.flow >= A.flow[0] && L.flow + 2 * A.pn <= A.pyr);
        CHECK(L.flow == A.flow[k ? 1 + (k & 1) : 0]);
        for (int f = 0; f < 2; ++f) CHECK(L.img[f] >= 0 && L.img[f] + n <= A.bs);
        if (s.fast_pyramids && k) { CHECK(L.img[0] == pyr_end && L.img[1] == pyr_end + n); pyr_end += 2 * n; }   // packed one behind the other
        else CHECK(L.img[1] == L.img[0] + A.pn);
    }
    CHECK(pyr_end <= A.bs);

    Model M(p, s);
    bool forked = false;
    int nmerged = 0, nmerge = 0;
    std::vector<int> cover;   // per (level, op, iter): the next pair an entry of that kind must start at
    cover.assign((size_t)(p.levels + 1) * (FB_JOIN + 1) * (size_t)(s.num_iters + 2), 0);
    std::vector<int> next_flip((size_t)s.B, -1);   // per pair: the flip the next iteration launch must carry (-1: a matrix update comes first)
    for (size_t i = 0; i < p.launches.size(); ++i) {
        const FbLaunch &l = p.launches[i];
        CHECK(l.level >= 0 && l.level <= p.levels && l.b0 >= 0 && l.nb >= 1 && l.b0 + l.nb <= s.B && l.iter >= 0 && l.iter < s.num_iters + 2);
        if (fails != before) break;
        const FbLevel &L = p.lv[l.level];
        int &c = cover[((size_t)l.level * (FB_JOIN + 1) + l.op) * (size_t)(s.num_iters + 2) + l.iter];
        CHECK(c == l.b0);
        c = l.b0 + l.nb;
        CHECK(l.chain == 0 || (l.chain == 1 && forked));
        const int fl = M.slot(L), fc = l.level < p.levels ? M.slot(p.lv[l.level + 1]) : -1;
        switch (l.op) {
        case FB_CONVERT: CHECK(l.nb <= kFmtPairs && (l.form == 1 || s.B == 1)); M.wr(l, P_FRAMES, 0); break;
        case FB_SPLIT_FLOW: CHECK(s.use_init && l.nb == 1); M.wr(l, P_FLOW, 0); break;
        case FB_PYR_DOWN: CHECK(s.fast_pyramids && l.level >= 1 && l.iter < 2); M.rd(l, M.img(l.level - 1, l.iter), l.level > 1 ? l.level - 1 : 0, forked); M.wr(l, M.img(l.level, l.iter), l.level); break;
        case FB_INIT_RESIZE: CHECK(L.init_resize); M.rd(l, P_FLOW, 0, forked); M.wr(l, fl, l.level); break;
        case FB_CLEAR_FLOW: CHECK(L.clear_flow && (l.form == 1 || l.form == 2)); M.wr(l, fl, l.level); break;
        case FB_ZOOM: CHECK(L.zoom); M.rd(l, fc, l.level + 1, forked); M.wr(l, fl, l.level); break;
        case FB_BLUR: CHECK(!p.direct && l.form != BLUR_AUTO); M.rd(l, P_FRAMES, 0, forked); M.wr(l, P_BLURRED, l.level); break;
        case FB_BLUR_DIRECT: CHECK(p.direct && l.nb <= kFmtPairs); M.wr(l, P_BLURRED, l.level); break;
        case FB_LEVEL_RESIZE: M.rd(l, P_BLURRED, l.level, forked); M.wr(l, P_LVL, l.level); break;
        case FB_POLY_EXP:
            CHECK(l.form == POLY_ROW || l.form == POLY_TILED);
            for (int f = 0; f < 2; ++f) M.rd(l, M.img(l.level, f), s.fast_pyramids && !l.level ? 0 : l.level, forked);
            M.wr(l, P_R, l.level);
            break;
        case FB_POLY_EXP_RESIZED: CHECK(l.form == POLY_ROW && p.fuse_small); M.rd(l, P_BLURRED, l.level, forked); M.wr(l, P_R, l.level); break;
        case FB_UPDATE_MATRICES:
        case FB_UPDATE_MATRICES_ZOOM:
            CHECK((l.op == FB_UPDATE_MATRICES_ZOOM) == L.zoom_fused);
            if (L.zoom_fused) { M.rd(l, fc, l.level + 1, forked); M.wr(l, fl, l.level); }
            else if (!L.zero_flow) M.rd(l, fl, l.level, forked);   // zero_flow: the update takes the flow as zero and reads no plane
            M.rd(l, P_R, l.level, forked);
            M.wr(l, P_M, l.level);
            for (int b = l.b0; b < l.b0 + l.nb; ++b) next_flip[b] = 0;
            break;
        case FB_ITERATE:
        case FB_ITERATE2: {
            const int last = l.iter + (l.op == FB_ITERATE2 ? 1 : 0);
            CHECK(last < s.num_iters && l.update == (last < s.num_iters - 1));
            CHECK(l.op == FB_ITERATE ? l.form >= ITER_ROW && l.form <= ITER_TILE64 : L.pair_it);
            for (int b = l.b0; b < l.b0 + l.nb; ++b) { CHECK(next_flip[b] == (l.flip ? 1 : 0)); next_flip[b] = l.flip ? 0 : 1; }   // M and bufM alternate
            M.rd(l, l.flip ? P_BUFM : P_M, l.level, forked);
            M.rd(l, P_R, l.level, forked);
            M.wr(l, fl, l.level);
            if (l.update) M.wr(l, l.flip ? P_M : P_BUFM, l.level);
            if (l.writes_merged) { ++nmerged; CHECK(l.level == 0 && s.B == 1 && last == s.num_iters - 1 && (l.op == FB_ITERATE2 || l.form != ITER_ROW)); }
        } break;
        case FB_MERGE: CHECK(l.nb <= kFmtPairs && (l.form == 1 || s.B == 1)); ++nmerge; M.rd(l, P_FLOW, 0, forked); break;
        case FB_FORK: CHECK(!forked && L.groups.two); forked = true; ++M.epoch; break;
        case FB_JOIN: CHECK(forked); forked = false; ++M.epoch; break;
        default: CHECK(l.op >= FB_CONVERT && l.op <= FB_JOIN);
        }
        if (l.op != FB_ITERATE && l.op != FB_ITERATE2) CHECK(!l.update && !l.flip && !l.writes_merged);
        if (l.op == FB_MERGE) for (size_t j = i; j < p.launches.size(); ++j) CHECK(p.launches[j].op == FB_MERGE);   // the merges end the list
    }
    CHECK(!forked && M.bad == 0);
    for (int v : cover) CHECK(v == 0 || v == s.B);   // every kind of launch of a level covers the pairs 0 .. B - 1 exactly once
    CHECK(nmerged <= 1 && (nmerged == 1) == (nmerge == 0));
    if (nmerge) CHECK(p.launches.back().op == FB_MERGE && cover[(size_t)FB_MERGE * (size_t)(s.num_iters + 2)] == s.B);
    if (fails != before)
        std::printf("  ... plan of %d x %d x %d, levels %d, scale %g, fast %d, iterations %d, initial flow %d, winSize %d, chains %d, fuse %d\n", s.W, s.H, s.B,
                    s.num_levels, s.pyr_scale, (int)s.fast_pyramids, s.num_iters, (int)s.use_init, s.win_size, K.chains, K.fuse);
}

int main()
{
    {   // the class defaults on one 640 x 480 pair (BASELINE configs[0]'s shape): numLevels 5, pyrScale 0.5 -> 40 x 30 is below MIN_SIZE 32
        const FbShape s = {640, 480, 1, 5, 0.5, false, 10, false};
        const FbPlan p = fb_make_plan(s, knobs());
        CHECK(p.levels == 3 && (int)p.lv.size() == 4 && p.fuse_small);
        const int w[4] = {640, 320, 160, 80}, h[4] = {480, 240, 120, 60};
        for (int k = 0; k <= 3; ++k) {
            CHECK(p.lv[k].w == w[k] && p.lv[k].h == h[k] && p.lv[k].ld % 64 == 0 && p.lv[k].ld >= w[k]);
            CHECK(p.lv[k].coarsest == (k == 3));
            CHECK(p.lv[k].groups.pairs == 1 && !p.lv[k].staged);          // a single pair is never cut into groups
            CHECK(p.lv[k].zoom_fused == (k < 3) && !p.lv[k].zoom);          // every finer level has another size: sampled in the first update
        }
        // sigma = (1 / scale - 1) / 2, smoothSize = max(cvRound(5 sigma) | 1, 3)  (:381-384)
        CHECK(p.lv[0].sigma == 0.0 && p.lv[0].smooth == 3);
        CHECK(p.lv[1].sigma == 0.5 && p.lv[1].smooth == 3);
        CHECK(p.lv[2].sigma == 1.5 && p.lv[2].smooth == 9);               // cvRound(7.5) = 8 (ties to even), | 1 = 9
        CHECK(p.lv[3].sigma == 3.5 && p.lv[3].smooth == 19);              // cvRound(17.5) = 18, | 1 = 19
        // no initial flow, ten iterations: the coarsest flow is never filled
        CHECK(p.lv[3].zero_flow && !p.lv[3].clear_flow && !p.lv[3].init_resize);
        for (int k = 0; k < 3; ++k) CHECK(!p.lv[k].zero_flow && !p.lv[k].clear_flow && !p.lv[k].init_resize);
        // the coarse levels underfill 256 CUs with 64 x 4 tiles: two iterations per launch there, not at level 0 (10 x 120 tiles)
        CHECK(p.lv[3].pair_it && p.lv[2].pair_it && !p.lv[0].pair_it);
    }
    {   // the initial flow of the caller, zero iterations, forced switches
        const FbShape s = {640, 480, 1, 5, 0.5, false, 0, true};
        FbPlan p = fb_make_plan(s, knobs());
        CHECK(p.lv[3].init_resize && !p.lv[3].zero_flow && !p.lv[3].clear_flow);
        const FbShape s0 = {640, 480, 1, 0, 0.5, false, 0, true};         // numLevels 0: level 0 is the coarsest and IS the initial flow
        p = fb_make_plan(s0, knobs());
        CHECK(p.levels == 0 && !p.lv[0].init_resize && !p.lv[0].clear_flow && !p.lv[0].zoom && !p.lv[0].zoom_fused);
        const FbShape s1 = {640, 480, 1, 5, 0.5, false, 0, false};
        p = fb_make_plan(s1, knobs());
        CHECK(p.lv[3].clear_flow && !p.lv[3].zero_flow);
        p = fb_make_plan(s1, knobs(0, 0));                                  // MIFLOW_FB_FUSE=0, MIFLOW_FB_PAIR=0: the plain forms
        CHECK(!p.fuse_small);
        for (int k = 0; k < 3; ++k) CHECK(p.lv[k].zoom && !p.lv[k].zoom_fused && !p.lv[k].pair_it);
        p = fb_make_plan(s1, knobs(-1, 1, 240, 2, false));                  // no two-iteration kernel for this window: never paired
        for (int k = 0; k <= 3; ++k) CHECK(!p.lv[k].pair_it);
        FbShape s11 = s1;
        s11.win_size = 11;
        p = fb_make_plan(s11, knobs(-1, 1));                                // ... and by the window size itself (winSize 11 has none)
        for (int k = 0; k <= 3; ++k) CHECK(!p.lv[k].pair_it);
    }
    {   // the bench's batch: 32 pairs of 640 x 480 -> not a small call; level 0 in 8 groups of 4 on two chains, the coarse levels whole
        const FbShape s = {640, 480, 32, 5, 0.5, false, 10, false};
        FbPlan p = fb_make_plan(s, knobs());
        CHECK(!p.fuse_small);
        CHECK(p.lv[0].groups.pairs == 4 && p.lv[0].groups.groups == 8 && p.lv[0].groups.two && p.lv[0].staged);
        CHECK(p.lv[2].groups.pairs == 32 && !p.lv[2].staged && !p.lv[2].groups.two);
        for (int k = 0; k <= 3; ++k) CHECK(!p.lv[k].pair_it);               // pairing is a small-call form
        for (int k = 0; k < 3; ++k) CHECK(p.lv[k].zoom_fused);               // the zoom inside the first update is for every call (round 5)
        p = fb_make_plan(s, knobs(-1, -1, 240, 1));                          // while the caller's stream is captured: one chain
        CHECK(p.lv[0].groups.pairs == 9 && !p.lv[0].groups.two);
        p = fb_make_plan(s, knobs(-1, -1, 0, 2));                            // MIFLOW_FB_GROUP_MB=0: no groups
        for (int k = 0; k <= 3; ++k) CHECK(p.lv[k].groups.pairs == 32 && !p.lv[k].staged);
    }
    {   // fastPyramids: the pyrDown chain's sizes ((w + 1) / 2), odd sizes; a scale that repeats a size -> copy, not a fused zoom
        const FbShape s = {641, 483, 2, 3, 0.5, true, 3, false};
        FbPlan p = fb_make_plan(s, knobs());
        CHECK(p.levels == 3 && p.lv[1].w == 321 && p.lv[1].h == 242 && p.lv[2].w == 161 && p.lv[2].h == 121 && p.lv[3].w == 81 && p.lv[3].h == 61);
        const FbShape t = {641, 483, 2, 3, 0.5, false, 3, false};          // without: cvRound of the scaled size
        p = fb_make_plan(t, knobs());
        CHECK(p.lv[1].w == 320 && p.lv[1].h == 242 && p.lv[3].w == 80 && p.lv[3].h == 60);
        const FbShape u = {100, 100, 1, 3, 0.999, false, 3, false};        // 100 * 0.999^k rounds to 100 for every level: same size
        p = fb_make_plan(u, knobs());
        CHECK(p.levels == 3);
        for (int k = 0; k < 3; ++k) CHECK(p.lv[k].w == 100 && p.lv[k].zoom && !p.lv[k].zoom_fused);
    }
    // invariants over a sweep
    for (int W : {33, 64, 200, 641, 1920})
        for (int H : {32, 100, 483, 1080})
            for (int B : {1, 3, 32, 70})
                for (int nl : {0, 1, 5, 9})
                    for (double ps : {0.5, 0.8})
                        for (int init = 0; init < 2; ++init) {
                            const FbShape s = {W, H, B, nl, ps, false, 2, init != 0};
                            const FbPlan p = fb_make_plan(s, knobs());
                            CHECK(p.levels >= 0 && p.levels <= nl && (int)p.lv.size() == p.levels + 1);
                            CHECK(p.lv[0].w == W && p.lv[0].h == H);
                            int ncoarsest = 0;
                            for (int k = 0; k <= p.levels; ++k) {
                                const FbLevel &L = p.lv[k];
                                ncoarsest += L.coarsest;
                                CHECK(L.w >= 1 && L.h >= 1 && (L.smooth & 1) && L.smooth >= 3);
                                CHECK((int)L.init_resize + (int)L.zero_flow + (int)L.clear_flow + (int)L.zoom + (int)L.zoom_fused <= 1);   // one way to start
                                CHECK(L.coarsest || L.zoom || L.zoom_fused);
                                CHECK(L.groups.pairs >= 1 && L.groups.pairs <= B && L.staged == (L.groups.pairs < B));
                                CHECK(!(L.pair_it && !p.fuse_small));
                                if (k > 0) CHECK(p.lv[k].w <= p.lv[k - 1].w && p.lv[k].h <= p.lv[k - 1].h);
                            }
                            CHECK(ncoarsest == 1 && p.lv[p.levels].coarsest);
                            if (p.levels < nl) {   // the crop stopped at the first level below MIN_SIZE
                                double sc = 1;
                                for (int i = 0; i <= p.levels; ++i) sc *= ps;
                                CHECK(W * sc < 32 || H * sc < 32);
                            }
                            // (b) the launch list and the layout, over fast pyramids (pyrScale 0.5 only), iteration counts and chains too
                            for (int fast = 0; fast <= (ps == 0.5 ? 1 : 0); ++fast)
                                for (int iters = 0; iters <= 3; ++iters)
                                    for (int chains = 1; chains <= 2; ++chains) {
                                        const FbShape t = {W, H, B, nl, ps, fast != 0, iters, init != 0};
                                        check_invariants(t, knobs(-1, -1, 240, chains));
                                    }
                        }
    for (int win : {5, 9, 11, 21})   // ... and the other kinds of window (no tile; tiles and pairs; tiles without pairs) and the forced switches
        for (int fuse = -1; fuse <= 1; ++fuse)
            for (int B : {1, 5}) {
                FbShape t = {200, 100, B, 3, 0.5, false, 3, false};
                t.win_size = win;
                check_invariants(t, knobs(fuse, fuse));
                FbKnobs k = knobs(fuse, fuse);
                k.fb_direct = 0;
                check_invariants(t, k);
            }
    for (int chains = 1; chains <= 2; ++chains)   // the zoom as a launch of its own inside the pair groups of two chains (MIFLOW_FB_FUSE=0; levels of one size)
        for (int init = 0; init < 2; ++init) {
            const FbShape t = {640, 480, 32, 5, 0.5, false, 3, init != 0}, u = {1920, 1080, 12, 2, 0.9999, false, 2, init != 0};
            FbKnobs k = knobs(0, 0, 240, chains);
            check_invariants(t, k);
            k.fb_direct = 0;
            check_invariants(t, k);
            check_invariants(u, knobs(-1, -1, 240, chains));
        }

    // (a) exact launch lists of four calls (read off the level loop this plan replaced; the kernel traces of the same calls agree)
    {
        const FbShape s = {640, 480, 1, 5, 0.5, false, 10, false};
        std::vector<E> w;   // the class defaults on one pair: 37 launches, no conversion (direct blur), no merge (the last iteration writes it)
        for (int k = 3; k >= 1; --k) {
            w.push_back({FB_BLUR_DIRECT, k, 0, 0}); w.push_back({FB_POLY_EXP_RESIZED, k, POLY_ROW, 0});
            w.push_back({k == 3 ? FB_UPDATE_MATRICES : FB_UPDATE_MATRICES_ZOOM, k, 0, 0});
            rep(w, 5, {FB_ITERATE2, k, 0, 0});
        }
        w.push_back({FB_BLUR_DIRECT, 0, 0, 0}); w.push_back({FB_POLY_EXP, 0, POLY_ROW, 0}); w.push_back({FB_UPDATE_MATRICES_ZOOM, 0, 0, 0});
        rep(w, 10, {FB_ITERATE, 0, ITER_TILE64, 0});
        FbPlan p = fb_make_plan(s, knobs());
        CHECK(w.size() == 37 && same_list(p, w, "defaults"));
        CHECK(p.direct && p.launches.back().writes_merged && !p.launches.back().update && p.launches.back().iter == 9);
        CHECK(p.launches[7].iter == 8 && p.launches[7].flip == false && p.launches[6].flip == true && p.launches[6].update && !p.launches[7].update);

        w.clear();          // MIFLOW_FB_FUSE=0, MIFLOW_FB_PAIR=0, the plain forms: zoom and level resize as launches, one iteration per launch, a merge: 59
        for (int k = 3; k >= 0; --k) {
            if (k < 3) w.push_back({FB_ZOOM, k, 0, 0});
            w.push_back({FB_BLUR_DIRECT, k, 0, 0});
            if (k > 0) w.push_back({FB_LEVEL_RESIZE, k, 0, 0});
            w.push_back({FB_POLY_EXP, k, POLY_ROW, 0}); w.push_back({FB_UPDATE_MATRICES, k, 0, 0});
            rep(w, 10, {FB_ITERATE, k, ITER_TILE64, 0});
        }
        w.push_back({FB_MERGE, 0, 0, 0});
        p = fb_make_plan(s, knobs(0, 0));
        CHECK(w.size() == 59 && same_list(p, w, "plain forms"));
        for (const FbLaunch &l : p.launches) CHECK(!l.writes_merged);

        w.clear();          // winSize 11: no tiled and no two-iteration kernel -> the generic row iteration, which does not write the caller's matrix: 53
        for (int k = 3; k >= 0; --k) {
            w.push_back({FB_BLUR_DIRECT, k, 0, 0}); w.push_back({k ? FB_POLY_EXP_RESIZED : FB_POLY_EXP, k, POLY_ROW, 0});
            w.push_back({k == 3 ? FB_UPDATE_MATRICES : FB_UPDATE_MATRICES_ZOOM, k, 0, 0});
            rep(w, 10, {FB_ITERATE, k, ITER_ROW, 0});
        }
        w.push_back({FB_MERGE, 0, 0, 0});
        FbShape s11 = s;
        s11.win_size = 11;
        p = fb_make_plan(s11, knobs());
        CHECK(w.size() == 53 && same_list(p, w, "winSize 11"));
        for (const FbLaunch &l : p.launches) CHECK(!l.writes_merged);

        w.clear();          // 32 pairs: the coarse levels whole (narrow tiles only where 32 pairs still underfill), level 0 in 8 groups of 4 on two chains: 147 launches + fork + join
        for (int k = 3; k >= 1; --k) {
            w.push_back({FB_BLUR_DIRECT, k, 0, 0}); w.push_back({FB_LEVEL_RESIZE, k, 0, 0}); w.push_back({FB_POLY_EXP, k, k == 1 ? POLY_TILED : POLY_ROW, 0});
            w.push_back({k == 3 ? FB_UPDATE_MATRICES : FB_UPDATE_MATRICES_ZOOM, k, 0, 0});
            rep(w, 10, {FB_ITERATE, k, k == 3 ? ITER_TILE64 : ITER_TILE256, 0});
        }
        w.push_back({FB_FORK, 0, 0, 0});
        for (int g = 0; g < 8; ++g) {
            w.push_back({FB_BLUR_DIRECT, 0, 0, g & 1}); w.push_back({FB_POLY_EXP, 0, POLY_TILED, g & 1}); w.push_back({FB_UPDATE_MATRICES_ZOOM, 0, 0, g & 1});
            rep(w, 10, {FB_ITERATE, 0, ITER_TILE256, g & 1});
        }
        w.push_back({FB_JOIN, 0, 0, 0}); w.push_back({FB_MERGE, 0, 1, 0});
        const FbShape s32 = {640, 480, 32, 5, 0.5, false, 10, false};
        p = fb_make_plan(s32, knobs());
        CHECK(w.size() == 149 && same_list(p, w, "32 pairs"));
        CHECK(p.launches[43].op == FB_BLUR_DIRECT && p.launches[43].b0 == 0 && p.launches[43].nb == 4 && p.launches[56].b0 == 4 && p.launches[56].chain == 1);
        CHECK(p.launches.capacity() >= p.launches.size() && p.launches.capacity() <= 2 * p.launches.size());   // reserved once, about right
    }

    // (c) the form rules against a table (simds = 1024: the narrow threshold is 512 workgroups, the tiled expansion's 1024)
    {
        const FbKnobs K = knobs();
        for (int kh : {2, 5, 13}) CHECK(fb_iter_form(640, 480, 1, kh, K) == ITER_ROW && !fb_iter_has_tile(kh) && !fb_iter2_ok(kh, K));
        for (int kh : {4, 6, 7, 10}) {
            CHECK(fb_iter_has_tile(kh) && fb_iter2_ok(kh, K) == (kh != 10));
            CHECK(fb_iter_form(640, 480, 1, kh, K) == ITER_TILE64);     // 3 x 120 = 360 workgroups of 256 x 4
            CHECK(fb_iter_form(256, 2044, 1, kh, K) == ITER_TILE64);    // 511
            CHECK(fb_iter_form(256, 2048, 1, kh, K) == ITER_TILE256);   // 512: `<`, not narrow
            CHECK(fb_iter_form(257, 1024, 1, kh, K) == ITER_TILE256);   // 2 x 256
            CHECK(fb_iter_form(64, 64, 32, kh, K) == ITER_TILE256 && fb_iter_form(64, 64, 31, kh, K) == ITER_TILE64);   // the batch counts
            FbKnobs k = K;
            k.fb_narrow = 0; CHECK(fb_iter_form(64, 64, 1, kh, k) == ITER_TILE256);
            k.fb_narrow = 1; CHECK(fb_iter_form(1920, 1080, 8, kh, k) == ITER_TILE64);
            k.fb_rows = 8; CHECK(fb_iter_form(64, 64, 1, kh, k) == ITER_TILE256);   // the 64-column tiles have four rows
            k = K; k.fb_tiled = 0; CHECK(fb_iter_form(640, 480, 1, kh, k) == ITER_ROW && !fb_iter2_ok(kh, k));
        }
        // expansion: tiles of 256 - 2 polyN columns x 8 rows
        CHECK(fb_poly_form(246, 4096, 2, 5, false, K) == POLY_TILED && fb_poly_form(246, 4088, 2, 5, false, K) == POLY_ROW);   // 1024 | 1022
        CHECK(fb_poly_form(247, 2048, 2, 5, false, K) == POLY_TILED && fb_poly_form(243, 2048, 2, 7, false, K) == POLY_TILED && fb_poly_form(242, 2048, 2, 7, false, K) == POLY_ROW);
        CHECK(fb_poly_form(640, 480, 8, 5, false, K) == POLY_TILED && fb_poly_form(640, 480, 2, 5, false, K) == POLY_ROW);
        CHECK(fb_poly_form(1920, 1080, 64, 5, true, K) == POLY_ROW);    // the tiles do not sample a resize
        { FbKnobs k = K; k.fb_poly_tiled = 0; CHECK(fb_poly_form(1920, 1080, 64, 5, false, k) == POLY_ROW); }
        // pre-blur
        for (int kh : {1, 4, 9, 19}) CHECK(fb_blur_form(640, 480, kh, K) == BLUR_TILED && fb_blur_direct_ok(640, 480, kh, K));
        for (int kh : {5, 20}) CHECK(fb_blur_form(640, 480, kh, K) == BLUR_GENERIC_FAST && !fb_blur_direct_ok(640, 480, kh, K));
        CHECK(fb_blur_form(20, 100, 19, K) == BLUR_TILED && fb_blur_form(19, 100, 19, K) == BLUR_GENERIC_FULL && fb_blur_form(100, 19, 19, K) == BLUR_GENERIC_FULL);
        CHECK(fb_blur_form(8, 100, 9, K) == BLUR_GENERIC_FULL && !fb_blur_direct_ok(8, 100, 9, K) && fb_blur_form(4, 3, 5, K) == BLUR_GENERIC_FULL);
        CHECK(fb_blur_form(2, 2, 1, K) == BLUR_TILED && fb_blur_form(1, 50, 1, K) == BLUR_GENERIC_FULL && fb_blur_form(21, 21, 20, K) == BLUR_GENERIC_FAST);
        { FbKnobs k = K; k.fb_blur_tiled = 0; CHECK(fb_blur_form(640, 480, 4, k) == BLUR_GENERIC_FAST && !fb_blur_direct_ok(640, 480, 4, k)); }
        // the direct pre-blur needs every level's half size: pyrScale 0.8 has levels of half size 5 and beyond -> converted planes
        const FbShape s8 = {640, 480, 1, 8, 0.8, false, 3, false};
        CHECK(!fb_make_plan(s8, K).direct && fb_make_plan(s8, K).launches[0].op == FB_CONVERT);
    }
    if (fails) { std::printf("fb_plan_test: %d FAILED\n", fails); return 1; }
    std::printf("fb_plan_test: ok\n");
    return 0;
}
