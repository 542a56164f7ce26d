// Stage-level C-ABI entry points of the TV-L1 path (the reference's internal device-layer
// boundary: tvl1flow::centeredGradient / warpBackward / estimateU / estimateDualVariables,
// modules/cudaoptflow/src/tvl1flow.cpp:58-76, and cuda::resize).  Caller planes may be
// arbitrarily pitched; they are staged through dense 256-B-aligned scratch planes.
#include <algorithm>
#include <cstring>
#include "tvl1_dev.h"
#include "mi_selftest.h"
#include <vector>

using namespace mi;
using namespace mi::tvl1;

namespace {

// a dense scratch plane of g (all its pairs)
int plane(DevTmp &S, const Geo &g, float **out) { return S.alloc(out, (size_t)g.ps * g.batch); }

Geo geo_of(int w, int h)
{
    Geo g;
    g.w = w; g.h = h; g.ld = align_up(w, 64); g.ps = (long long)g.ld * h; g.batch = 1;
    return g;
}

int check_f32(const mi_mat *m, const char *name)
{
    MI_REQUIRE(m && m->data, MI_ERR_BAD_ARG, "%s: null matrix", name);
    MI_REQUIRE(m->type == MI_32FC1, MI_ERR_BAD_TYPE, "%s: must be CV_32FC1", name);
    MI_REQUIRE(m->rows > 0 && m->cols > 0, MI_ERR_BAD_SIZE, "%s: empty", name);
    MI_REQUIRE(m->step >= (size_t)m->cols * 4 && m->step % 4 == 0, MI_ERR_BAD_ARG, "%s: bad step", name);
    return MI_OK;
}

// (the g.batch pairs of a plane are its g.batch * g.h rows: pair b's row y is row b * h + y of the caller's plane and of the scratch
// plane, whose pair stride g.ps is g.h rows of g.ld floats)
int stage_in(DevTmp &S, const mi_mat *m, const Geo &g, float **out, hipStream_t st)
{
    float *p;
    MI_TRY(plane(S, g, &p));
    MI_HIP_TRY(hipMemcpy2DAsync(p, (size_t)g.ld * 4, m->data, m->step, (size_t)g.w * 4, (size_t)g.h * g.batch, hipMemcpyDeviceToDevice, st));
    *out = p;
    return MI_OK;
}

int stage_out(const float *p, const Geo &g, mi_mat *m, hipStream_t st)
{
    MI_HIP_TRY(hipMemcpy2DAsync(m->data, m->step, p, (size_t)g.ld * 4, (size_t)g.w * 4, (size_t)g.h * g.batch, hipMemcpyDeviceToDevice, st));
    return MI_OK;
}

}  // namespace

extern "C" {

int mi_tvl1_centered_gradient(const mi_mat *src, mi_mat *dx, mi_mat *dy, void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    MI_TRY(check_f32(src, "src")); MI_TRY(check_f32(dx, "dx")); MI_TRY(check_f32(dy, "dy"));
    MI_REQUIRE(dx->rows == src->rows && dx->cols == src->cols && dy->rows == src->rows && dy->cols == src->cols,
               MI_ERR_BAD_SIZE, "dx/dy size != src size");
    const Geo g = geo_of(src->cols, src->rows);
    DevTmp S;
    float *s, *ox, *oy;
    MI_TRY(plane(S, g, &ox)); MI_TRY(plane(S, g, &oy));
    MI_TRY(stage_in(S, src, g, &s, st));
    MI_TRY(gradient(s, ox, oy, g, st));
    MI_TRY(stage_out(ox, g, dx, st)); MI_TRY(stage_out(oy, g, dy, st));
    MI_HIP_TRY(hipStreamSynchronize(st));
    return MI_OK;
}

int mi_tvl1_warp_backward(int semantics, const mi_mat *I0, const mi_mat *I1, const mi_mat *I1x, const mi_mat *I1y,
                          const mi_mat *u1, const mi_mat *u2, mi_mat *I1w, mi_mat *I1wx, mi_mat *I1wy, mi_mat *grad,
                          mi_mat *rho)
{
    hipStream_t st = nullptr;
    // test hook: semantics | MI_WARP_STAGE_FAST runs the fast-math form of the fused-gradient kernel (separable bicubic sums)
    const bool fast = (semantics & MI_WARP_STAGE_FAST) != 0;
    const int lds = (semantics & MI_WARP_STAGE_LDS) ? 1 : (semantics & MI_WARP_STAGE_GATHER) ? 0 : -1;
    semantics &= ~(MI_WARP_STAGE_FAST | MI_WARP_STAGE_LDS | MI_WARP_STAGE_GATHER);
    MI_REQUIRE(semantics == MI_SEM_CPU_REF || semantics == MI_SEM_CUDA_COMPAT, MI_ERR_BAD_ARG, "bad semantics");
    // I1x == I1y == NULL: the derivative planes are the centred differences of I1, formed inside the warp kernel (the
    // kernel calc() runs, tvl1_warp_kernels.hip); otherwise the caller's planes are gathered (any planes, k_warp)
    const bool fused = !I1x && !I1y;
    MI_REQUIRE(fused || (I1x && I1y), MI_ERR_BAD_ARG, "I1x and I1y must be both given or both NULL");
    MI_REQUIRE(I0 && I1, MI_ERR_BAD_ARG, "null matrix");
    const mi_mat *ins[6] = {I0, I1, fused ? I1 : I1x, fused ? I1 : I1y, u1, u2};
    mi_mat *outs[5] = {I1w, I1wx, I1wy, grad, rho};
    for (int i = 0; i < 6; ++i) { MI_TRY(check_f32(ins[i], "input")); MI_REQUIRE(ins[i]->rows == I0->rows && ins[i]->cols == I0->cols, MI_ERR_BAD_SIZE, "input size mismatch"); }
    for (int i = 0; i < 5; ++i) { MI_TRY(check_f32(outs[i], "output")); MI_REQUIRE(outs[i]->rows == I0->rows && outs[i]->cols == I0->cols, MI_ERR_BAD_SIZE, "output size mismatch"); }
    const Geo g = geo_of(I0->cols, I0->rows);
    DevTmp S;
    float *in[6], *out[5];
    for (int i = 0; i < 6; ++i) MI_TRY(stage_in(S, ins[i], g, &in[i], st));
    for (int i = 0; i < 5; ++i) MI_TRY(plane(S, g, &out[i]));
    float tabh[128], *tabd = nullptr;
    host_cubic_table(tabh);
    MI_TRY(S.alloc(&tabd, 128));
    MI_HIP_TRY(hipMemcpyAsync(tabd, tabh, sizeof(tabh), hipMemcpyHostToDevice, st));
    const float *u1v[2] = {in[4], in[4]}, *u2v[2] = {in[5], in[5]};
    if (fused) {
        MI_TRY(warp_fused(semantics, fast, lds, in[0], in[1], u1v, u2v, out[0], out[1], out[2], out[3], out[4], tabd, g, nullptr, 0, st));
    } else {
        float *pk = nullptr;   // {I1, I1x, I1y, 0} per pixel, the layout the gather kernel reads
        MI_TRY(S.alloc(&pk, 4 * (size_t)g.ps));
        MI_TRY(pack3(in[1], in[2], in[3], pk, g, st));
        MI_TRY(warp(semantics, in[0], pk, u1v, u2v, out[0], out[1], out[2], out[3], out[4], tabd, g, nullptr, 0, st));
    }
    for (int i = 0; i < 5; ++i) MI_TRY(stage_out(out[i], g, outs[i], st));
    MI_HIP_TRY(hipStreamSynchronize(st));
    return MI_OK;
}

int mi_tvl1_iterate(int exact_math, int time_block, int niter, const mi_mat *I1wx, const mi_mat *I1wy, const mi_mat *grad,
                    const mi_mat *rho_c, const mi_mat *u_in, const mi_mat *p_in, mi_mat *u_out, mi_mat *p_out, float l_t,
                    float theta, float taut, double *err_host, void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    MI_REQUIRE(niter >= 1, MI_ERR_BAD_ARG, "niter must be >= 1");
    // test hook: time_block = 100 + T runs the INDEPENDENT-wave kernel of block length T (every wave its own 64-column strip) where
    // T alone runs the kernel of record (T = 10: four joined waves per 256-column strip) -- the two must agree bit for bit
    const bool indep = !exact_math && time_block >= 100;
    if (indep) time_block -= 100;
    const bool tiled = !exact_math && time_block < 0;   // test hook: register-tile kernel, variant -time_block - 1
    MI_REQUIRE(!tiled || -time_block - 1 < tile_variants(), MI_ERR_BAD_ARG, "no such register-tile variant");
    const bool blocked = (!exact_math && time_block > 0) || tiled;
    MI_REQUIRE(!(blocked && err_host), MI_ERR_BAD_ARG, "per-iteration error sums are not available from the blocked kernel");
    MI_REQUIRE(u_in && p_in && u_out && p_out, MI_ERR_BAD_ARG, "null plane array");
    const mi_mat *stat[4] = {I1wx, I1wy, grad, rho_c};
    for (int i = 0; i < 4; ++i) { MI_TRY(check_f32(stat[i], "static plane")); MI_REQUIRE(stat[i]->rows == I1wx->rows && stat[i]->cols == I1wx->cols, MI_ERR_BAD_SIZE, "size mismatch"); }
    for (int i = 0; i < 2; ++i) { MI_TRY(check_f32(&u_in[i], "u_in")); MI_TRY(check_f32(&u_out[i], "u_out")); }
    for (int i = 0; i < 4; ++i) { MI_TRY(check_f32(&p_in[i], "p_in")); MI_TRY(check_f32(&p_out[i], "p_out")); }
    const Geo g = geo_of(I1wx->cols, I1wx->rows);
    DevTmp S;
    float *sp[4];
    for (int i = 0; i < 4; ++i) MI_TRY(stage_in(S, stat[i], g, &sp[i], st));
    IterPlanes pl;
    memset(&pl, 0, sizeof(pl));
    pl.ix = sp[0]; pl.iy = sp[1]; pl.g = sp[2]; pl.rc = sp[3];
    for (int i = 0; i < 2; ++i) { MI_TRY(stage_in(S, &u_in[i], g, &pl.u[0][i], st)); MI_TRY(plane(S, g, &pl.u[1][i])); }
    for (int i = 0; i < 4; ++i) { MI_TRY(stage_in(S, &p_in[i], g, &pl.p[0][i], st)); MI_TRY(plane(S, g, &pl.p[1][i])); }
    Ctl ctl;
    memset(&ctl, 0, sizeof(ctl));
    if (err_host) {
        MI_TRY(S.alloc(&ctl.S, niter));
        MI_TRY(S.alloc(&ctl.E, niter));
        MI_HIP_TRY(hipMemsetAsync(ctl.E, 0, sizeof(unsigned long long) * niter, st));
        ctl.Q = niter;
        ctl.thr = -1.0;  // always active
    }
    int cur = 0;
    for (int it = 0; it < niter;) {
        if (tiled) {
            const int T = std::min(niter - it, kTileMaxBlock);
            MI_TRY(iterate_tile(-time_block - 1, T, pl, g, l_t, theta, taut, false, cur, st));
            it += T;
            cur ^= 1;
            continue;
        }
        if (blocked) {
            const int T = greedy_blocks(std::min(niter - it, 10), time_block, {1, 2, 3, 4, 5, 6, 8, 10})[0];   // the largest supported block
            // always the streaming kernel (the tile kernel is compared against it)
            MI_TRY(iterate_tb(tb_kernel(TbUse::Fixed, T, g, false, false, tv_knobs(), TbOverride{true, 0, indep}), T, pl, g, l_t, theta, taut, false, cur, st));
            it += T;
            cur ^= 1;
            continue;
        }
        ++it;
        if (err_host) {
            const int it0 = it - 1;
            Ctl c = ctl;
            c.q = it0; c.q_prev = it0 - 1; c.first_of_warp = (it0 == 0); c.reset_cur = (it0 == 0);
            MI_TRY(iterate(exact_math != 0, pl, g, l_t, theta, taut, false, &c, 0, st));
        } else {
            MI_TRY(iterate(exact_math != 0, pl, g, l_t, theta, taut, false, nullptr, cur, st));
        }
        cur ^= 1;
    }
    for (int i = 0; i < 2; ++i) MI_TRY(stage_out(pl.u[cur][i], g, &u_out[i], st));
    for (int i = 0; i < 4; ++i) MI_TRY(stage_out(pl.p[cur][i], g, &p_out[i], st));
    MI_HIP_TRY(hipStreamSynchronize(st));
    if (err_host) {
        std::vector<unsigned long long> e(niter);
        MI_HIP_TRY(hipMemcpy(e.data(), ctl.E, sizeof(unsigned long long) * niter, hipMemcpyDeviceToHost));
        for (int i = 0; i < niter; ++i) err_host[i] = (double)e[i] / 16777216.0;
    }
    return MI_OK;
}

// The iterations in the forms calc() runs them (c_api.h, mi_tvl1_stage_desc).  Everything the descriptor asks for is checked before
// the first byte is staged; the launches are those of lane_calc's executors (tvl1_api.cpp run_blocked, run_per_iteration, run_spec) with
// the streaming kernels forced where a form names them (TbOverride).
int mi_tvl1_iterate_stage(const mi_tvl1_stage_desc *d, void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    MI_REQUIRE(d, MI_ERR_BAD_ARG, "null descriptor");
    const int form = d->form, niter = d->niter, B = d->batch;
    MI_REQUIRE(form >= MI_TVL1_STAGE_ONE && form <= MI_TVL1_STAGE_SPEC_TILE, MI_ERR_BAD_ARG, "unknown form %d", form);
    MI_REQUIRE(niter >= 1 && niter <= 100000, MI_ERR_BAD_ARG, "niter must be in 1..100000");
    MI_REQUIRE(B >= 1, MI_ERR_BAD_ARG, "batch must be >= 1");
    const bool gam = d->gamma != 0.f, ng = d->grad == nullptr, pz = d->p_zero != 0;
    const bool spec = form == MI_TVL1_STAGE_SPEC || form == MI_TVL1_STAGE_SPEC_TILE;
    const bool tiles = form == MI_TVL1_STAGE_TILE || form == MI_TVL1_STAGE_SPEC_TILE;
    const bool streaming = form == MI_TVL1_STAGE_BLOCKED || form == MI_TVL1_STAGE_INDEP || form == MI_TVL1_STAGE_EXACT_BLOCKED ||
                           form == MI_TVL1_STAGE_SPEC;
    MI_REQUIRE(d->rows_per_band == 0 || (streaming && d->rows_per_band >= 8), MI_ERR_BAD_ARG,
               "rows_per_band: 0 (the planner) or >= 8, streaming forms only");
    MI_REQUIRE(!tiles || (d->variant >= 0 && d->variant < tile_variants() && (!gam || d->variant < 2)), MI_ERR_BAD_ARG,
               "no register-tile variant %d%s", d->variant, gam ? " with the illumination channel" : "");
    MI_REQUIRE(!ng || form == MI_TVL1_STAGE_BLOCKED || form == MI_TVL1_STAGE_SPEC || gam, MI_ERR_BAD_ARG,
               "no |grad|^2 plane: only the blocked and speculative streaming forms form it themselves");
    MI_REQUIRE(!d->err_fix || form == MI_TVL1_STAGE_ONE || spec, MI_ERR_BAD_ARG, "error sums: one-iteration and speculative forms only");
    MI_REQUIRE(!(spec && pz), MI_ERR_BAD_ARG, "the speculative steps never take p = 0 (a replay re-reads the input set)");
    MI_REQUIRE(!(form == MI_TVL1_STAGE_ONE && ng), MI_ERR_BAD_ARG, "the one-iteration kernel needs the |grad|^2 plane");
    MI_REQUIRE(!(form == MI_TVL1_STAGE_ONE && d->blocks), MI_ERR_BAD_ARG, "blocks: blocked forms only");
    MI_REQUIRE(!(spec && d->blocks), MI_ERR_BAD_ARG, "the speculative steps run blocks of time_block");

    // the passes: the caller's block list, or greedy blocks of at most time_block over the lengths the form's table holds
    const TbUse use = form == MI_TVL1_STAGE_EXACT_BLOCKED ? TbUse::Exact : spec ? TbUse::Spec : TbUse::Fixed;
    const TbOverride forced{true, d->rows_per_band, form == MI_TVL1_STAGE_INDEP};   // the streaming forms: never the tile, the caller's band height
    Geo g{};   // (a forced kernel does not depend on the level)
    auto kernel = [&](int T) { return tb_kernel(use, T, g, gam, ng, tv_knobs(), forced); };
    auto exists = [&](int T) {
        if (form == MI_TVL1_STAGE_ONE) return T == 1;
        if (tiles) return T >= 1 && T <= kTileMaxBlock;
        return kernel(T).row != nullptr;
    };
    std::vector<int> blocks;
    if (form == MI_TVL1_STAGE_ONE) {
        blocks.assign(niter, 1);
    } else if (spec) {
        MI_REQUIRE(exists(d->time_block) && (form != MI_TVL1_STAGE_SPEC || d->time_block <= kTbMaxBlock), MI_ERR_BAD_ARG,
                   "no speculative kernel for block %d", d->time_block);
        blocks.assign((size_t)((niter + d->time_block - 1) / d->time_block), d->time_block);
    } else if (d->blocks) {
        MI_REQUIRE(d->nblocks >= 1 && d->nblocks <= niter, MI_ERR_BAD_ARG, "nblocks must be in 1..niter");
        long long sum = 0;
        for (int k = 0; k < d->nblocks; ++k) {
            MI_REQUIRE(exists(d->blocks[k]), MI_ERR_BAD_ARG, "no kernel of this form for a block of %d", d->blocks[k]);
            sum += d->blocks[k];
            blocks.push_back(d->blocks[k]);
        }
        MI_REQUIRE(sum == niter, MI_ERR_BAD_ARG, "the blocks sum to %lld, not niter = %d", sum, niter);
    } else {
        const int cap = d->time_block > 0 ? d->time_block : tiles ? kTileMaxBlock : form == MI_TVL1_STAGE_EXACT_BLOCKED ? kTbExactMaxBlock
                                                                                                                          : kTbMaxBlock;
        for (int left = niter; left > 0; left -= blocks.back()) {
            int t = 0;
            for (int c = std::min(cap, left); c >= 1 && !t; --c) if (exists(c)) t = c;
            MI_REQUIRE(t, MI_ERR_BAD_ARG, "no kernel of this form for blocks of at most %d", cap);
            blocks.push_back(t);
        }
    }

    // the planes: h rows per pair
    MI_REQUIRE(d->I1wx && d->I1wy && d->rho_c && d->u_in && d->u_out && d->p_out && (d->p_in || pz), MI_ERR_BAD_ARG, "null plane");
    MI_TRY(check_f32(d->I1wx, "I1wx"));
    MI_REQUIRE(d->I1wx->rows % B == 0, MI_ERR_BAD_SIZE, "rows (%d) must be batch (%d) x the pair height", d->I1wx->rows, B);
    const int nu = gam ? 3 : 2, np = gam ? 6 : 4;
    std::vector<const mi_mat *> ins = {d->I1wx, d->I1wy, d->rho_c};
    if (!ng) ins.push_back(d->grad);
    for (int i = 0; i < nu; ++i) ins.push_back(&d->u_in[i]);
    if (!pz) for (int i = 0; i < np; ++i) ins.push_back(&d->p_in[i]);
    std::vector<const mi_mat *> all = ins;
    for (int i = 0; i < nu; ++i) all.push_back(&d->u_out[i]);
    for (int i = 0; i < np; ++i) all.push_back(&d->p_out[i]);
    for (const mi_mat *m : all) {
        MI_TRY(check_f32(m, "plane"));
        MI_REQUIRE(m->rows == d->I1wx->rows && m->cols == d->I1wx->cols, MI_ERR_BAD_SIZE, "plane size mismatch");
    }
    g = geo_of(d->I1wx->cols, d->I1wx->rows / B);
    g.batch = B;

    DevTmp S;
    IterPlanes pl;
    memset(&pl, 0, sizeof(pl));
    float *stat[4] = {nullptr, nullptr, nullptr, nullptr};
    const mi_mat *statm[4] = {d->I1wx, d->I1wy, d->grad, d->rho_c};
    for (int i = 0; i < 4; ++i) if (statm[i]) MI_TRY(stage_in(S, statm[i], g, &stat[i], st));
    pl.ix = stat[0]; pl.iy = stat[1]; pl.g = stat[2]; pl.rc = stat[3];
    pl.gamma = d->gamma;
    pl.err_u3 = d->err_u3 ? 1 : 0;
    for (int i = 0; i < nu; ++i) {
        MI_TRY(stage_in(S, &d->u_in[i], g, &pl.u[0][i], st));
        MI_TRY(plane(S, g, &pl.u[1][i]));
    }
    for (int i = 0; i < np; ++i) {
        if (pz) {   // never read: NaN, so that a kernel reading them shows
            MI_TRY(plane(S, g, &pl.p[0][i]));
            MI_HIP_TRY(hipMemsetAsync(pl.p[0][i], 0xff, sizeof(float) * (size_t)g.ps * B, st));
        } else {
            MI_TRY(stage_in(S, &d->p_in[i], g, &pl.p[0][i], st));
        }
        MI_TRY(plane(S, g, &pl.p[1][i]));
    }

    // control slots: the checked one-iteration launches use slot `it` and error sum `it`; the speculative steps slot k and the error
    // sums of the blocks from e0 = k * T on (a block runs all its T iterations but the last, which runs what is left)
    const int nb = (int)blocks.size();
    const bool check = form == MI_TVL1_STAGE_ONE && d->err_fix;
    Ctl ctl;
    memset(&ctl, 0, sizeof(ctl));
    if (check || spec) {
        const long long Q = spec ? (long long)(nb + 1) * d->time_block + nb + 2 : niter;
        const size_t n = (size_t)Q * B;
        MI_TRY(S.alloc(&ctl.S, n)); MI_TRY(S.alloc(&ctl.E, n)); MI_TRY(S.alloc(&ctl.P, n));
        MI_HIP_TRY(hipMemsetAsync(ctl.S, 0, sizeof(int2) * n, st));
        MI_HIP_TRY(hipMemsetAsync(ctl.E, 0, sizeof(unsigned long long) * n, st));
        MI_HIP_TRY(hipMemsetAsync(ctl.P, 0, sizeof(double) * n, st));
        ctl.Q = (int)Q;
        ctl.thr = -1.0;   // the CPU class's rule, a threshold no iteration passes: every launch active, no block cut short
    }
    std::vector<int> cur_b(B, 0);   // per pair: the set the result is in
    if (spec) {
        // run_spec (tvl1_api.cpp) without history and host feedback: blocks of T, then the launch that settles the last of them
        int4 *X;
        MI_TRY(S.alloc(&X, (size_t)ctl.Q * B));
        MI_HIP_TRY(hipMemsetAsync(X, 0, sizeof(int4) * (size_t)ctl.Q * B, st));
        SpecK sk;
        memset(&sk, 0, sizeof(sk));
        sk.X = X; sk.iters = niter; sk.q_hist = -1; sk.hist_num = 1; sk.hist_den = 1;
        const int T = d->time_block;
        int t_after = nb * T, e_next = 0, e_prev = 0;
        for (int k = 0; k <= nb; ++k) {
            const bool last = k == nb;
            if (!last) t_after -= T;
            Ctl a = ctl;
            a.q = k; a.q_prev = k - 1; a.first_of_warp = (k == 0); a.reset_cur = (k == 0); a.n = 0;
            sk.e0_prev = e_prev; sk.final_launch = last ? 1 : 0; sk.t_after = t_after;
            MI_TRY(tiles ? iterate_tile_spec(T, pl, g, d->l_t, d->theta, d->taut, a, sk, e_next, st, d->variant)
                      : iterate_tb_spec(kernel(T), T, pl, g, d->l_t, d->theta, d->taut, a, sk, e_next, st));
            e_prev = e_next;
            if (!last) e_next += T;
        }
        std::vector<int2> sl(B);
        MI_HIP_TRY(hipMemcpy2DAsync(sl.data(), sizeof(int2), ctl.S + nb, sizeof(int2) * (size_t)ctl.Q, sizeof(int2), (size_t)B,
                                    hipMemcpyDeviceToHost, st));
        MI_HIP_TRY(hipStreamSynchronize(st));
        for (int b = 0; b < B; ++b) {
            cur_b[b] = sl[b].x ^ (sl[b].y & MI_SLOT_FLIP);
            MI_REQUIRE((sl[b].y & MI_SLOT_DONE) && MI_SLOT_ITERS(sl[b].y) == niter - (nb - 1) * T, MI_ERR_HIP,
                       "speculative steps: pair %d settled as {%d, %#x}, not done after %d iterations", b, sl[b].x, sl[b].y, niter);
        }
    } else {
        int cur = 0;
        for (int k = 0; k < nb; ++k) {
            const int T = blocks[k];
            const bool pzk = pz && k == 0;
            switch (form) {
            case MI_TVL1_STAGE_ONE:
                if (check) {
                    Ctl c = ctl;
                    c.q = k; c.q_prev = k - 1; c.first_of_warp = (k == 0); c.reset_cur = (k == 0);
                    MI_TRY(iterate(d->exact_math != 0, pl, g, d->l_t, d->theta, d->taut, pzk, &c, 0, st));
                } else {
                    MI_TRY(iterate(d->exact_math != 0, pl, g, d->l_t, d->theta, d->taut, pzk, nullptr, cur, st));
                }
                break;
            case MI_TVL1_STAGE_BLOCKED:
            case MI_TVL1_STAGE_INDEP:
            case MI_TVL1_STAGE_EXACT_BLOCKED:
                MI_TRY(iterate_tb(kernel(T), T, pl, g, d->l_t, d->theta, d->taut, pzk, cur, st));
                break;
            case MI_TVL1_STAGE_TILE:
                MI_TRY(iterate_tile(d->variant, T, pl, g, d->l_t, d->theta, d->taut, pzk, cur, st));
                break;
            }
            cur ^= 1;
        }
        std::fill(cur_b.begin(), cur_b.end(), cur);
    }

    // the result planes, per pair from the set it ended in
    for (int b = 0; b < B; ++b) {
        Geo g1 = g;
        g1.batch = 1;
        const long long o = (long long)b * g.ps;
        for (int i = 0; i < nu + np; ++i) {
            const float *src = (i < nu ? pl.u[cur_b[b]][i] : pl.p[cur_b[b]][i - nu]) + o;
            mi_mat m = i < nu ? d->u_out[i] : d->p_out[i - nu];
            m.data = (char *)m.data + (size_t)b * g.h * m.step;
            m.rows = g.h;
            MI_TRY(stage_out(src, g1, &m, st));
        }
    }
    MI_HIP_TRY(hipStreamSynchronize(st));
    if (d->err_fix) {
        MI_HIP_TRY(hipMemcpy2D(d->err_fix, sizeof(unsigned long long) * niter, ctl.E, sizeof(unsigned long long) * (size_t)ctl.Q,
                               sizeof(unsigned long long) * niter, (size_t)B, hipMemcpyDeviceToHost));
    }
    return MI_OK;
}

int mi_resize_linear(int semantics, const mi_mat *src, mi_mat *dst, double fx, double fy, int explicit_dsize, float post_scale,
                     void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    MI_REQUIRE(semantics == MI_SEM_CPU_REF || semantics == MI_SEM_CUDA_COMPAT, MI_ERR_BAD_ARG, "bad semantics");
    MI_TRY(check_f32(src, "src")); MI_TRY(check_f32(dst, "dst"));
    const Geo gs = geo_of(src->cols, src->rows), gd = geo_of(dst->cols, dst->rows);
    double isx = fx, isy = fy;
    if (explicit_dsize) { isx = (double)gd.w / gs.w; isy = (double)gd.h / gs.h; }
    MI_REQUIRE(isx > 0 && isy > 0, MI_ERR_BAD_ARG, "fx, fy must be > 0 when dsize is not explicit");
    DevTmp S;
    float *s, *d;
    MI_TRY(plane(S, gd, &d));
    MI_TRY(stage_in(S, src, gs, &s, st));
    const float *srcs[3][2] = {{s, nullptr}, {nullptr, nullptr}, {nullptr, nullptr}};
    float *dsts[3] = {d, nullptr, nullptr};
    const float post[3] = {post_scale, 1.f, 1.f};
    if (semantics == MI_SEM_CUDA_COMPAT && gd.w == gs.w && gd.h == gs.h) {
        // dsize == src.size(): plain copy (cudawarping/src/resize.cpp:89-93)
        MI_HIP_TRY(hipMemcpyAsync(d, s, sizeof(float) * (size_t)gs.ps, hipMemcpyDeviceToDevice, st));
    } else {
        MI_TRY(resize(semantics, 1, srcs, 1, dsts, gs, gd, isx, isy, post, nullptr, 0, st));
    }
    MI_TRY(stage_out(d, gd, dst, st));
    MI_HIP_TRY(hipStreamSynchronize(st));
    return MI_OK;
}

int miflow_selftest_lane_shift(int *out_host)
{
    MI_REQUIRE(out_host, MI_ERR_BAD_ARG, "null out");
    int *d = nullptr;
    DevTmp tmp;
    MI_TRY(tmp.alloc(&d, 128));
    MI_TRY(dbg_lane_shift(d, nullptr));
    MI_HIP_TRY(hipMemcpy(out_host, d, 128 * sizeof(int), hipMemcpyDeviceToHost));
    return MI_OK;
}

int miflow_selftest_jw_fault(int *fault)
{
    MI_REQUIRE(fault, MI_ERR_BAD_ARG, "null out");
    return tb_jw_fault(fault);
}

}  // extern "C"
