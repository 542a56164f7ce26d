// Dual TV-L1: handle, scratch arena, pyramid orchestration and the C-ABI entry points.
// Host-side twin of OpticalFlowDual_TVL1_Impl::calcImpl / procOneScale
// (modules/cudaoptflow/src/tvl1flow.cpp:185-382; CPU modules/optflow/src/tvl1flow.cpp:402-533,
// 1313-1408) -- but fully stream-ordered: no host read-back inside the iteration loop.
#include "tvl1_dev.h"
#include "mi_selftest.h"
#include <cfloat>
#include <algorithm>
#include <cmath>
#include <vector>
#include <chrono>
#include <sched.h>
#include <time.h>

using namespace mi;
using namespace mi::tvl1;

namespace {

constexpr double kFeedbackWaitLimitUs = 30e6;   // polled host feedback: a decision word that has not arrived after 30 s never will

struct LevelBuf {
    Geo g;
    float *I0 = nullptr, *I1 = nullptr;
    float *u[2][3] = {{nullptr, nullptr, nullptr}, {nullptr, nullptr, nullptr}};  // [set][u1,u2,u3]
};

struct SlotInfo { int scale, warp; };

}  // namespace

// What a lane's arena was carved for: kept while the frame, the pyramid and the optional planes stay (and the batch does not grow)
struct ArenaKey {
    int W = 0, H = 0, scales = 0;
    double step = 0;
    bool gamma = false, median = false;
    bool operator==(const ArenaKey &o) const { return W == o.W && H == o.H && scales == o.scales && step == o.step && gamma == o.gamma && median == o.median; }
};

// Everything one sub-batch needs: its own arena, pointer table, control slots and profiling events, so that two lanes can
// run concurrently on two internal streams (the warp kernel is bound by the vector-memory path, the blocked iteration
// kernel by VALU issue: they overlap, profiles/r02*).
struct Lane {
    // the arena: a block out of the process-wide cache (mi_own.h) and what it was carved for; below it, the planes carved out of it
    struct { HipArena blk{&big_cache()}; ArenaKey key; int capB = 0; } arena;
    std::vector<LevelBuf> L;
    // full-resolution-capacity scratch planes (re-laid-out densely per level)
    float *scr[6] = {};    // scr[0..1]: median-filter temporaries; I1wx, I1wy, grad, rho_c
    float *pbuf[2][6] = {};   // [set][p11,p12,p21,p22,p31,p32]
    DevBuf<PtrTab> tab;
    std::vector<PtrTab> tab_host;   // source of the asynchronous upload: must outlive the call
    // device loop control
    struct {
        DevBuf<int2> S;
        DevBuf<unsigned long long> E;
        DevBuf<double> Pd;   // per slot prevError (cv::cuda check schedule)
        DevBuf<int4> X;      // per slot state of the speculative steps (SpecK::X)
        long long Q = 0;
        int B = 0;
        std::vector<SlotInfo> slots;   // (scale, warp) of every launch slot the last calc used
    } loop;
    // history: iteration counts per (scale, warp, pair slot) of the previous calc, two parities (SpecK::h_in / h_out)
    struct {
        DevBuf<int> H;
        unsigned long long sig = 0; // geometry / batch / loop shape the counts belong to (0: none)
        int par = 0;                // parity the NEXT calc writes
    } hist;
    // host feedback (mi_tvl1_params.host_feedback): pinned landing area of the control slots read back between launches
    struct {
        PinnedBuf<int2, hipHostMallocDefault> host;
        Event ev;
        PinnedBuf<int, hipHostMallocCoherent | hipHostMallocMapped> flag;   // polled form (SpecK::fb_flag): {decision word, count} per pair
        int seq = 0;
        std::vector<int> hist;        // polled form: most iterations a (scale, warp) of the previous calc needed over its pairs (0: unknown)
        unsigned long long hist_sig = 0;
    } fb;
    // profiling (mi_tvl1_set_profiling)
    struct Region { int e0, e1; long long launches; double bytes; int kind; int level; };   // kind 0: iteration launches, 1: warp launch; level = pyramid scale
    struct { std::vector<TimingEvent> events; std::vector<Region> regions; } prof;
    // internal stream of a concurrent lane + its completion event
    struct { Stream stream; Event done; } internal;

    // THE destruction order of a lane.  Profiling events first (nothing waits for them).  Then the arena goes back to the cache, which
    // takes the idle event with it where that is valid.  Then the remaining events, while the stream they were recorded on is alive,
    // then that stream (the last join made the caller's stream wait for its work).  The buffers go last, as members: hipFree /
    // hipHostFree synchronise the device, so nothing still running reads freed control slots or a freed pointer table.
    ~Lane()
    {
        prof.events.clear();
        arena.blk.reset();
        internal.done.reset();
        fb.ev.reset();
        internal.stream.reset();
    }
};

struct mi_tvl1 {
    mi_tvl1_params P;
    int device = 0;
    DevBuf<float> cubic_tab;
    Event fork;   // one for all internal lanes; declared before them: it goes after them
    static const int kMaxLanes = 4;
    Lane lane[kMaxLanes];
    int last_nscales = 0, last_batch = 0, last_lanes = 1;
    int last_first[kMaxLanes + 1] = {};   // pairs [last_first[i], last_first[i + 1]) ran on lane i
    bool last_check = false;
    bool profiling = false;
};

void mi_tvl1_default_params(mi_tvl1_params *p)
{
    if (!p) return;
    // cv::cuda::OpticalFlowDual_TVL1::create defaults, cudaoptflow.hpp:375-385
    p->tau = 0.25; p->lambda = 0.15; p->theta = 0.3; p->epsilon = 0.01; p->scale_step = 0.8; p->gamma = 0.0;
    p->nscales = 5; p->warps = 5; p->iterations = 300; p->use_initial_flow = 0;
    p->inner_iterations = 1; p->median_filtering = 1;
    // SEMANTICS OF A DEFAULT-CONSTRUCTED OBJECT (read this before dropping the class in).  The acceptance reference of this
    // path is the CPU class cv::optflow::DualTVL1OpticalFlow ("EPE vs CPU ref", BASELINE.json), so the default arithmetic is
    // the CPU class's: cv::remap(INTER_CUBIC, a = -0.75, 1/32-px phases, constant-0 border) warp, cv::resize pyramid
    // (half-pixel centres), convergence test after every iteration with a float threshold.  cv::cuda's own kernels differ from
    // that -- normalised a = -0.5 bicubic with clamp addressing, cuda::resize without the half-pixel shift, a sparse check
    // schedule -- by 0.07-0.14 px mean EPE on the synthetic pairs used here (mostly at image borders the flow leaves);
    // semantics = MI_SEM_CUDA_COMPAT selects exactly that arithmetic (pinned bit for bit on the reference's OpenCL twins of the
    // CUDA kernels, tests/test_ref_pin.py) for callers validated against cv::cuda.  Math: fast device math (v_rcp / v_sqrt /
    // fma, iterations fused per HBM pass) by default, which the reference's own test tolerates (CUDA vs CPU |1 - CCORR| <= 4e-3,
    // test_optflow.cpp:465; here <= 1e-4 and mean EPE <= 5e-3 px against the oracle); exact_math = 1 performs the separately
    // rounded IEEE operations of the reference in its order.
    p->semantics = MI_SEM_CPU_REF; p->exact_math = 0; p->time_block = 0; p->lanes = 0; p->stop_slack = 0; p->host_feedback = 0;
}

// upper bound of control slots per pair (scales x warps x iterations) a convergence-checked calc may enqueue
static const long long kMaxSlots = 4000000;

static int validate_params(const mi_tvl1_params *p)
{
    MI_REQUIRE(p, MI_ERR_BAD_ARG, "null params");
    MI_REQUIRE(p->nscales > 0 && p->nscales <= 32, MI_ERR_BAD_ARG, "nscales must be in [1,32] (CV_Assert nscales_ > 0)");
    MI_REQUIRE(p->warps >= 0 && p->warps <= 64, MI_ERR_BAD_ARG, "warps must be in [0,64]");
    MI_REQUIRE(p->iterations >= 0 && p->inner_iterations >= 0, MI_ERR_BAD_ARG, "negative iteration count");
    MI_REQUIRE((long long)p->iterations * p->inner_iterations <= kMaxSlots, MI_ERR_BAD_ARG,
               "iterations x inner_iterations must not exceed %lld", kMaxSlots);
    MI_REQUIRE(p->scale_step > 0 && p->scale_step < 1, MI_ERR_BAD_ARG, "scale_step must be in (0,1)");
    MI_REQUIRE(p->theta != 0, MI_ERR_BAD_ARG, "theta must be non-zero");
    MI_REQUIRE(p->semantics == MI_SEM_CPU_REF || p->semantics == MI_SEM_CUDA_COMPAT, MI_ERR_BAD_ARG, "bad semantics");
    MI_REQUIRE(p->median_filtering <= 1 || p->median_filtering == 3 || p->median_filtering == 5, MI_ERR_BAD_ARG,
               "medianFiltering must be 1 (off), 3 or 5 (cv::medianBlur on CV_32F)");
    MI_REQUIRE(p->lanes >= 0 && p->lanes <= 4, MI_ERR_BAD_ARG, "lanes must be 0 (automatic) or 1..4");
    MI_REQUIRE(p->stop_slack >= 0 && p->stop_slack <= 8, MI_ERR_BAD_ARG, "stop_slack must be in 0..8");
    MI_REQUIRE(p->host_feedback >= -1 && p->host_feedback <= 1, MI_ERR_BAD_ARG, "host_feedback must be -1, 0 or 1");
    return MI_OK;
}

int mi_tvl1_create(const mi_tvl1_params *p, mi_tvl1 **out)
{
    MI_REQUIRE(out, MI_ERR_BAD_ARG, "null out");
    *out = nullptr;
    mi_tvl1_params d;
    if (!p) { mi_tvl1_default_params(&d); p = &d; }
    int rc = validate_params(p);
    if (rc) return rc;
    MI_TRY(require_device());
    mi_tvl1 *h = new mi_tvl1();
    h->P = *p;
    float tab[128];
    host_cubic_table(tab);
    auto upload = [&]() -> int {
        MI_HIP_TRY(hipGetDevice(&h->device));
        MI_TRY(h->cubic_tab.ensure(128));
        MI_HIP_TRY(hipMemcpy(h->cubic_tab.p, tab, sizeof(tab), hipMemcpyHostToDevice));
        return MI_OK;
    };
    if (const int rc = upload()) { delete h; return rc; }
    *out = h;
    return MI_OK;
}

int mi_tvl1_set_params(mi_tvl1 *h, const mi_tvl1_params *p)
{
    MI_REQUIRE(h, MI_ERR_BAD_ARG, "null handle");
    int rc = validate_params(p);
    if (rc) return rc;
    h->P = *p;
    return MI_OK;
}

int mi_tvl1_get_params(const mi_tvl1 *h, mi_tvl1_params *p)
{
    MI_REQUIRE(h && p, MI_ERR_BAD_ARG, "null argument");
    *p = h->P;
    return MI_OK;
}

int mi_tvl1_query_plan(int width, int height, int pairs_per_lane, int iterations_per_launch, int *kernel, int *rows_per_band)
{
    MI_REQUIRE(kernel && rows_per_band, MI_ERR_BAD_ARG, "null output");
    MI_REQUIRE(width > 0 && height > 0 && pairs_per_lane > 0 && iterations_per_launch > 0, MI_ERR_BAD_ARG, "bad plan query");
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) { set_error("no HIP device"); return MI_ERR_NO_DEVICE; }
    const Geo g{width, height, (width + 63) / 64 * 64, (long long)((width + 63) / 64 * 64) * height, pairs_per_lane};
    const TbKernel k = tb_kernel(TbUse::Fixed, iterations_per_launch, g, false, false, tv_knobs(), TbOverride{});   // the planner's own choice
    if (!k.tile && !k.row) { set_error("unsupported time block %d", iterations_per_launch); return MI_ERR_BAD_ARG; }
    *kernel = k.tile ? 1 : 0;
    *rows_per_band = k.tile ? tile_owned_rows() : plan_band_rows(*k.row, g);
    return MI_OK;
}

int mi_tvl1_set_profiling(mi_tvl1 *h, int enable)
{
    MI_REQUIRE(h, MI_ERR_BAD_ARG, "null handle");
    h->profiling = enable != 0;
    return MI_OK;
}

int mi_tvl1_get_profile(mi_tvl1 *h, double *ms_total, long long *launches, double *algo_bytes)
{
    return mi_tvl1_get_profile_kind(h, 0, ms_total, launches, algo_bytes);
}

int mi_tvl1_get_profile_kind(mi_tvl1 *h, int kind, double *ms_total, long long *launches, double *algo_bytes)
{
    return mi_tvl1_get_profile_level(h, kind, -1, ms_total, launches, algo_bytes);
}

int mi_tvl1_get_profile_level(mi_tvl1 *h, int kind, int level, double *ms_total, long long *launches, double *algo_bytes)
{
    MI_REQUIRE(h && ms_total && launches && algo_bytes, MI_ERR_BAD_ARG, "null argument");
    MI_REQUIRE(kind == 0 || kind == 1, MI_ERR_BAD_ARG, "kind must be 0 (iteration launches) or 1 (warp launches)");
    *ms_total = 0; *launches = 0; *algo_bytes = 0;
    for (int li = 0; li < h->last_lanes; ++li) {
        Lane &ln = h->lane[li];
        for (const auto &r : ln.prof.regions) {
            if (r.kind != kind || (level >= 0 && r.level != level)) continue;
            MI_HIP_TRY(hipEventSynchronize(ln.prof.events[r.e1].get()));
            float ms = 0.f;
            MI_HIP_TRY(hipEventElapsedTime(&ms, ln.prof.events[r.e0].get(), ln.prof.events[r.e1].get()));
            *ms_total += ms; *launches += r.launches; *algo_bytes += r.bytes;
        }
    }
    return MI_OK;
}

void mi_tvl1_destroy(mi_tvl1 *h) { delete h; }

// The lane's arena in the plan's layout (kept while the frame, the pyramid and the optional planes stay and the batch does not grow)
static int ensure_arena(const mi_tvl1_params &P, Lane &ln, const TvPlan &pl, int W, int H, int B)
{
    const ArenaKey key{W, H, P.nscales, P.scale_step, P.gamma != 0.0, pl.median != 0};
    if (!(ln.arena.blk.get() && ln.arena.key == key && ln.arena.capB >= B)) {
        ln.L.clear();
        if (const int rc = ln.arena.blk.acquire(pl.arena.total * sizeof(float))) return rc;
        float *const base = (float *)ln.arena.blk.get();
        const auto at = [&](size_t o) { return o == kNoPlane ? nullptr : base + o; };
        ln.L.resize(pl.geo.size());
        for (size_t l = 0; l < pl.geo.size(); ++l) {
            ln.L[l].I0 = at(pl.arena.lv[l][0]); ln.L[l].I1 = at(pl.arena.lv[l][1]);
            for (int k = 0; k < 6; ++k) ln.L[l].u[k / 3][k % 3] = at(pl.arena.lv[l][2 + k]);
        }
        for (int k = 0; k < 6; ++k) ln.scr[k] = at(pl.arena.scr[k]);
        for (int k = 0; k < 12; ++k) ln.pbuf[k / 6][k % 6] = at(pl.arena.p[k]);
        ln.arena.key = key; ln.arena.capB = B;
    }
    for (size_t l = 0; l < pl.geo.size(); ++l) ln.L[l].g = pl.geo[l];   // (this calc's batch)
    return MI_OK;
}

static int check_pair(const mi_mat *I0, const mi_mat *I1, const mi_mat *flow, const mi_mat *I0ref)
{
    MI_REQUIRE(I0 && I1 && flow, MI_ERR_BAD_ARG, "null matrix");
    MI_REQUIRE(I0->data && I1->data && flow->data, MI_ERR_BAD_ARG, "null data pointer");
    // CV_Assert( I0.type() == CV_8UC1 || I0.type() == CV_32FC1 )  tvl1flow.cpp:187
    MI_REQUIRE(I0->type == MI_8UC1 || I0->type == MI_32FC1, MI_ERR_BAD_TYPE, "I0 must be CV_8UC1 or CV_32FC1");
    MI_REQUIRE(I0->rows == I1->rows && I0->cols == I1->cols, MI_ERR_BAD_SIZE, "I0.size() != I1.size()");  // :188
    MI_REQUIRE(I0->type == I1->type, MI_ERR_BAD_TYPE, "I0.type() != I1.type()");                          // :189
    MI_REQUIRE(flow->type == MI_32FC2, MI_ERR_BAD_TYPE, "flow must be CV_32FC2");
    MI_REQUIRE(flow->rows == I0->rows && flow->cols == I0->cols, MI_ERR_BAD_SIZE, "flow.size() != I0.size()");  // :190
    MI_REQUIRE(I0->rows >= 3 && I0->cols >= 3, MI_ERR_BAD_SIZE, "image must be at least 3x3");
    // the dense float planes are addressed with 32-bit byte offsets from a per-pair base (buffer loads of the warp's border windows)
    MI_REQUIRE((long long)((I0->cols + 63) / 64 * 64) * I0->rows * 4 < (1LL << 32), MI_ERR_BAD_SIZE,
               "image too large: a float plane of it must stay below 4 GiB");
    const size_t es = I0->type == MI_8UC1 ? 1 : 4;
    MI_REQUIRE(I0->step >= (size_t)I0->cols * es && I1->step >= (size_t)I1->cols * es, MI_ERR_BAD_ARG, "step < cols*elemSize");
    MI_REQUIRE(flow->step >= (size_t)flow->cols * 8, MI_ERR_BAD_ARG, "flow step < cols*8");
    if (es == 4) MI_REQUIRE(I0->step % 4 == 0 && I1->step % 4 == 0 && ((uintptr_t)I0->data % 4) == 0 && ((uintptr_t)I1->data % 4) == 0,
                            MI_ERR_BAD_ARG, "float images must be 4-byte aligned");
    MI_REQUIRE(flow->step % 8 == 0 && ((uintptr_t)flow->data % 8) == 0, MI_ERR_BAD_ARG, "flow must be 8-byte aligned");
    MI_REQUIRE(I0->rows == I0ref->rows && I0->cols == I0ref->cols && I0->type == I0ref->type, MI_ERR_BAD_SIZE,
               "all pairs of a batch must share size and type");
    return MI_OK;
}

const TvKnobs &mi::tvl1::tv_knobs()
{
    static const TvKnobs k = [] {
        const Tuning &t = tuning();
        TvKnobs v{};
        v.tile_maxpx = t.tile_maxpx; v.tile_spec = t.tile_spec; v.tile_variant = t.tile_variant; v.tile_small_wgs = t.tile_small_wgs;
        v.tile_variants = std::min(tile_variants(), (int)(sizeof(v.tile_rows) / sizeof(v.tile_rows[0])));
        for (int i = 0; i < v.tile_variants; ++i) v.tile_rows[i] = tile_shape_rows(i);
        v.tile_fb_block = t.tile_fb_block; v.tile_fb_model = t.tile_fb_model;
        v.tb_force = t.tb_force != 0; v.tb_nograd = t.tb_nograd; v.tb_jw = t.tb_jw; v.tb_jw_spec = t.tb_jw_spec;
        v.tb_ppl = t.tb_ppl; v.tb_wps = t.tb_wps; v.tb_pf = t.tb_pf; v.tb_p16 = t.tb_p16; v.tb_il = t.tb_il;
        v.tb_fw = t.tb_fw; v.tb_skip_p = t.tb_skip_p; v.tb_hist = t.tb_hist; v.spec = t.spec; v.exact_tb = t.exact_tb;
        v.fb_poll = t.fb_poll; v.fb_ahead = t.fb_ahead; v.warp_fast = t.warp_fast; v.warp_lds = t.warp_lds; v.x_skip = t.x_skip;
        return v;
    }();
    return k;
}

// The lane's pointer table, control slots, history and host-feedback buffers for plan pl (stream-ordered uploads and clears).
static int ensure_buffers(const TvPlan &pl, Lane &ln, int B, const mi_mat *I0s, const mi_mat *I1s, mi_mat *flows, hipStream_t st)
{
    int rc;
    if ((rc = ln.tab.ensure(B))) return rc;
    ln.tab_host.resize(B);
    for (int i = 0; i < B; ++i)
        ln.tab_host[i] = PtrTab{I0s[i].data, I1s[i].data, flows[i].data, (long long)I0s[i].step, (long long)I1s[i].step, (long long)flows[i].step};
    // pageable source: a few KB, staged by the runtime before the call returns; kept in the lane anyway
    MI_HIP_TRY(hipMemcpyAsync(ln.tab.p, ln.tab_host.data(), sizeof(PtrTab) * B, hipMemcpyHostToDevice, st));
    if (pl.check) {
        MI_REQUIRE(pl.Q <= kMaxSlots, MI_ERR_BAD_ARG, "scales x warps x iterations = %lld control slots exceed the limit of %lld", pl.Q, kMaxSlots);
        if (ln.loop.Q < pl.Q || ln.loop.B < B) {
            const size_t n = (size_t)pl.Q * B;
            if ((rc = ln.loop.S.ensure(n)) || (rc = ln.loop.E.ensure(n)) || (rc = ln.loop.Pd.ensure(n)) || (rc = ln.loop.X.ensure(n))) return rc;
            ln.loop.Q = pl.Q; ln.loop.B = B;
        }
        MI_HIP_TRY(hipMemsetAsync(ln.loop.E.p, 0, sizeof(unsigned long long) * (size_t)ln.loop.Q * B, st));
        MI_HIP_TRY(hipMemsetAsync(ln.loop.S.p, 0, sizeof(int2) * (size_t)ln.loop.Q * B, st));
    }
    if (pl.hist) {   // counts of the previous calc of this lane
        const int nw = (int)pl.warp[0].size();
        const size_t h_n = (size_t)pl.used * nw * B;
        if (ln.hist.H.n < 2 * h_n) ln.hist.sig = 0;
        if ((rc = ln.hist.H.ensure(2 * h_n))) return rc;
        if (ln.hist.sig != pl.hist_sig) {   // counts of another geometry say nothing: start from none (0 = no estimate)
            MI_HIP_TRY(hipMemsetAsync(ln.hist.H.p, 0, sizeof(int) * ln.hist.H.n, st));
            ln.hist.sig = pl.hist_sig;
        }
        if (ln.fb.hist_sig != pl.hist_sig || ln.fb.hist.size() != (size_t)pl.used * nw) {
            ln.fb.hist.assign((size_t)pl.used * nw, 0);
            ln.fb.hist_sig = pl.hist_sig;
        }
        ln.hist.par ^= 1;
    }
    if (pl.fb) {
        const bool fresh = ln.fb.flag.n < 2 * (size_t)B;
        if ((rc = ln.fb.host.ensure(2 * (size_t)B)) || (rc = ln.fb.flag.ensure(2 * (size_t)B))) return rc;
        if (fresh) memset(ln.fb.flag.p, 0, sizeof(int) * ln.fb.flag.n);
        MI_TRY(ln.fb.ev.ensure());
    }
    return MI_OK;
}

namespace {

// What one lane's calc carries from launch to launch; the executors below advance it.
struct Run {
    mi_tvl1 *h;
    Lane &ln;
    const TvPlan &pl;
    const TvKnobs &K;
    hipStream_t st;
    int B;
    size_t ev_used = 0;
    Ctl ctl;                 // the device loop control every launch starts from (thr: the current scale's)
    IterPlanes planes;       // the current scale's (planes.g = grad)
    float *grad = nullptr;   // the current warp's |grad|^2 plane (nullptr: the warp does not store it)
    float l_t, theta, taut;
    int q = 0, q_last = -1, e_next = 0;   // device-control slot counters; next per-iteration error-sum index (speculative steps)
    int q_settle_prev = -1, q_settle_scale = -1;   // settling launches of the previous warp / of the coarser scale's first warp
    int fb_prev_warp = 2, fb_prev_scale = 2;       // launch index at which the previous warp / the coarser scale's first warp was found stopped
    int cur = 0;             // host-known buffer set (fixed work)
    bool first_of_scale = true;
    bool pre_warped = false; // this warp's kernel was enqueued ahead, behind the previous warp's last launch (host feedback)
};

// records a profiling event on the lane's stream
int record(Run &r, int *idx)
{
    if (r.ev_used == r.ln.prof.events.size()) {
        TimingEvent e;
        MI_TRY(e.ensure());
        r.ln.prof.events.push_back(std::move(e));
    }
    *idx = (int)r.ev_used++;
    MI_HIP_TRY(hipEventRecord(r.ln.prof.events[*idx].get(), r.st));
    return MI_OK;
}

// level 0: convertTo(CV_32F, 8U ? 1 : 255) (tvl1flow.cpp:200-201); the scales (:238-266); the coarsest flow's start
int enqueue_pyramid(Run &r, int type)
{
    const mi_tvl1_params &P = r.h->P;
    Lane &ln = r.ln;
    const int ns = r.pl.used, B = r.B;
    int rc = convert(ln.tab.p, type, ln.L[0].I0, ln.L[0].I1, ln.L[0].g, r.st);
    if (rc) return rc;
    // CPU behaviour (optflow/src/tvl1flow.cpp:435-439); the CUDA calc() never splits the caller's flow (latent reference bug,
    // SURVEY Appendix B Q8)
    if (P.use_initial_flow && (rc = unpack_flow(ln.tab.p, ln.L[0].u[0][0], ln.L[0].u[0][1], ln.L[0].g, r.st))) return rc;
    const float one3[3] = {1.f, 1.f, 1.f};
    for (size_t s = 1; s < ln.L.size(); ++s) {
        const LevelBuf &c = ln.L[s - 1];
        const float *src[3][2] = {{c.I0, nullptr}, {c.I1, nullptr}, {nullptr, nullptr}};
        float *dst[3] = {ln.L[s].I0, ln.L[s].I1, nullptr};
        rc = resize(P.semantics, 2, src, 1, dst, c.g, ln.L[s].g, P.scale_step, P.scale_step, one3, nullptr, 0, r.st);
        if (rc) return rc;
        if ((int)s >= ns) break;
        if (P.use_initial_flow) {
            const float *us[3][2] = {{c.u[0][0], nullptr}, {c.u[0][1], nullptr}, {nullptr, nullptr}};
            float *ud[3] = {ln.L[s].u[0][0], ln.L[s].u[0][1], nullptr};
            const float post[3] = {(float)P.scale_step, (float)P.scale_step, 1.f};
            rc = resize(P.semantics, 2, us, 1, ud, c.g, ln.L[s].g, P.scale_step, P.scale_step, post, nullptr, 0, r.st);
            if (rc) return rc;
        }
    }
    const LevelBuf &Lc = ln.L[ns - 1];
    const size_t bytes = sizeof(float) * (size_t)Lc.g.ps * B;
    if (!P.use_initial_flow) {
        MI_HIP_TRY(hipMemsetAsync(Lc.u[0][0], 0, bytes, r.st));
        MI_HIP_TRY(hipMemsetAsync(Lc.u[0][1], 0, bytes, r.st));
    }
    if (P.gamma != 0.0) MI_HIP_TRY(hipMemsetAsync(Lc.u[0][2], 0, bytes, r.st));   // u3 starts at 0 on the coarsest scale (tvl1flow.cpp:273-275)
    return MI_OK;
}

// the warp of the current scale (warpBackward + centeredGradient, tvl1flow.cpp:325-340); ahead: enqueued before the host knows whether
// the previous warp has stopped, it runs only for pairs whose slot q_last says so (Ctl::need_done)
int launch_warp(Run &r, const LevelBuf &Lv, bool ahead)
{
    const float *u1v[2] = {Lv.u[0][0], Lv.u[1][0]}, *u2v[2] = {Lv.u[0][1], Lv.u[1][1]};
    Ctl c = r.ctl;
    c.q_prev = r.q_last;
    c.need_done = ahead ? 1 : 0;
    const bool dev_cur = ahead || (r.pl.check && !r.first_of_scale);   // at the first warp of a scale u lives in set 0 (host-known)
    return warp_fused(r.h->P.semantics, r.pl.fast_warp, -1, Lv.I0, Lv.I1, u1v, u2v, nullptr, r.ln.scr[2], r.ln.scr[3],
                      r.grad, r.ln.scr[5], r.h->cubic_tab.p, Lv.g, dev_cur ? &c : nullptr, r.cur, r.st);
}

// Fixed work: T iterations per HBM pass (tvl1_tbr_kernels.hip), the optional median filter between outer iterations; in exact math
// blocks of up to 5 fused iterations (k_iterate_tbr MODE 2), bit-identical to one launch per iteration
int run_blocked(Run &r, LevelBuf &Lv, const TvWarp &w, long long *nlaunch)
{
    float *const mu1[2] = {Lv.u[0][0], Lv.u[1][0]}, *const mu2[2] = {Lv.u[0][1], Lv.u[1][1]};
    const int nb = (int)w.blocks.size();
    int rc;
    for (int no = 0; no < w.outer; ++no) {
        if (r.pl.median && (rc = median_flow(r.pl.median, mu1, mu2, r.ln.scr[0], r.ln.scr[1], Lv.g, nullptr, r.cur, r.st))) return rc;
        for (int k = 0; k < nb; ++k) {
            ++*nlaunch;
            if (w.skip_iterations) { r.first_of_scale = false; continue; }
            const bool last_pass = w.skip_p_last && no == w.outer - 1 && k == nb - 1;
            rc = w.fused ? iterate_tb_fused(w.run[k], Lv.I0, Lv.I1, r.h->cubic_tab.p, r.planes, Lv.g, r.l_t, r.theta, r.taut, r.first_of_scale, r.cur,
                                            r.st, last_pass)
                         : iterate_tb(w.run[k], w.blocks[k], r.planes, Lv.g, r.l_t, r.theta, r.taut, r.first_of_scale, r.cur, r.st, last_pass,
                                      last_pass && w.pack_in_pass ? r.ln.tab.p : nullptr);
            if (rc) return rc;
            r.cur ^= 1;
            r.first_of_scale = false;
        }
    }
    return MI_OK;
}

// One launch per iteration, with the convergence check on the device where epsilon > 0
int run_per_iteration(Run &r, LevelBuf &Lv, int s, int wp, long long *nlaunch)
{
    const mi_tvl1_params &P = r.h->P;
    const int mf = r.pl.median;
    float *const mu1[2] = {Lv.u[0][0], Lv.u[1][0]}, *const mu2[2] = {Lv.u[0][1], Lv.u[1][1]};
    int rc;
    for (int it = 0; it < r.pl.iters; ++it) {
        ++*nlaunch;
        if (mf && it % P.inner_iterations == 0) {   // cv::medianBlur before each outer iteration (optflow tvl1flow.cpp:1381-1384)
            Ctl mc = r.ctl;
            mc.q_prev = r.q_last; mc.first_of_warp = (it == 0); mc.reset_cur = r.first_of_scale;
            if ((rc = median_flow(mf, mu1, mu2, r.ln.scr[0], r.ln.scr[1], Lv.g, r.pl.check ? &mc : nullptr, r.cur, r.st))) return rc;
        }
        if (r.pl.check) {
            Ctl ic = r.ctl;
            ic.q = r.q; ic.q_prev = r.q_last; ic.first_of_warp = (it == 0); ic.reset_cur = r.first_of_scale; ic.n = it;
            rc = iterate(P.exact_math != 0, r.planes, Lv.g, r.l_t, r.theta, r.taut, r.first_of_scale, &ic, 0, r.st);
            r.ln.loop.slots.push_back({s, wp});
            r.q_last = r.q++;
        } else {
            rc = iterate(P.exact_math != 0, r.planes, Lv.g, r.l_t, r.theta, r.taut, r.first_of_scale, nullptr, r.cur, r.st);
            r.cur ^= 1;
        }
        if (rc) return rc;
        r.first_of_scale = false;
    }
    return MI_OK;
}

struct Feedback { bool all = true, all_before = true; int n_most = 0; };

// Polled host feedback: the launch just enqueued publishes its decision word (sequence seq) when it starts -- wait for that word, not
// for the launch.  Bare spin (pause) for the first ~20 us -- the flag normally lands within a few microseconds of the launch starting --
// then the core is handed back between looks (sched_yield; a sleep of 50 us once 2 ms have passed: earlier work queued on the caller's
// stream, or many handles waiting in many threads), so a waiting calc() does not hold a core.  The stream is queried on the slow path
// only; a wall-clock bound ends a wait no launch will ever answer.
int poll_feedback(Run &r, int seq, Feedback *f)
{
    const int *flag = r.ln.fb.flag.p;
    for (int b = 0; b < r.B; ++b) {
        int v = 0;
        const auto t_wait0 = std::chrono::steady_clock::now();
        for (long long spin = 0;; ++spin) {
            v = __atomic_load_n(flag + 2 * b, __ATOMIC_ACQUIRE);
            if ((v >> 2) == seq) break;
            if ((spin & 63) != 63) {
#if defined(__x86_64__) || defined(__i386__)
                __builtin_ia32_pause();
#endif
                continue;
            }
            const double waited_us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t_wait0).count();
            if (waited_us < 20.0) continue;
            // a failed launch never writes: the stream is idle (or in error) and the word is not there
            const hipError_t qe = hipStreamQuery(r.st);
            if (qe != hipErrorNotReady) {
                v = __atomic_load_n(flag + 2 * b, __ATOMIC_ACQUIRE);
                if ((v >> 2) == seq) break;
                MI_HIP_TRY(qe);
                MI_REQUIRE(false, MI_ERR_HIP, "host feedback: launch finished without publishing its decision");
            }
            MI_REQUIRE(waited_us < kFeedbackWaitLimitUs, MI_ERR_HIP, "host feedback: no decision from the device within %.0f s", kFeedbackWaitLimitUs * 1e-6);
            if (waited_us < 2000.0) sched_yield();
            else { struct timespec ts_ = {0, 50000}; nanosleep(&ts_, nullptr); }
        }
        f->all_before = f->all_before && (v & 2);
        f->all = f->all && (v & 1);
        f->n_most = std::max(f->n_most, flag[2 * b + 1]);
    }
    return MI_OK;
}

// Copied host feedback: the slots of the last launch and of the one before it, per pair
int copy_feedback(Run &r, Feedback *f)
{
    Lane &ln = r.ln;
    MI_HIP_TRY(hipMemcpy2DAsync(ln.fb.host.p, 2 * sizeof(int2), ln.loop.S.p + (r.q_last - 1), sizeof(int2) * (size_t)ln.loop.Q, 2 * sizeof(int2),
                                (size_t)r.B, hipMemcpyDeviceToHost, r.st));
    MI_HIP_TRY(hipEventRecord(ln.fb.ev.get(), r.st));
    MI_HIP_TRY(hipEventSynchronize(ln.fb.ev.get()));
    for (int b = 0; b < r.B; ++b) {
        f->all_before = f->all_before && (ln.fb.host.p[2 * b].y & MI_SLOT_DONE);
        f->all = f->all && (ln.fb.host.p[2 * b + 1].y & MI_SLOT_DONE);
    }
    return MI_OK;
}

// Speculative steps (k_iterate_tbr MODE 1): a launch runs a block of iterations recording their error sums; the next launch applies the
// reference's stopping rule to them and either builds on the block or replays the exact count from its input.  One settling launch
// ends the warp.  After convergence the remaining launches end at once.
// Host feedback (mi_tvl1_params.host_feedback): a call of one or two pairs reads the pairs' control slots back between launches and
// stops enqueuing for this warp once every pair's slot says DONE -- the state is then settled (a replay, if one was due, ran inside the
// launch that wrote the flag) and the slot is the one the following kernels look at.  First read-back at spec_first_poll, then after
// every second launch.  The host waits like the reference's class does at each of its checks (cudaoptflow/src/tvl1flow.cpp:362-368);
// the flows do not depend on any of it.
int run_spec(Run &r, LevelBuf &Lv, const TvWarp &w, int s, int wp, long long *nlaunch)
{
    const TvPlan &pl = r.pl;
    Lane &ln = r.ln;
    const int nw = (int)pl.warp[s].size();
    int rc, hprev = 0;   // the previous calc's count for this warp, where the host has seen it (polled host feedback)
    if (pl.fb_poll && pl.hist) {
        int &hc = ln.fb.hist[(size_t)s * nw + wp];
        hprev = hc;
        hc = 0;   // known again once this warp's stop has been seen
    }
    const std::vector<int> plan = spec_blocks(w, Lv.g, hprev, r.K);
    int t_after = 0;
    for (int v : plan) t_after += v;
    SpecK sk;
    memset(&sk, 0, sizeof(sk));
    sk.X = ln.loop.X.p; sk.iters = pl.iters;
    sk.q_hist = wp > 0 ? r.q_settle_prev : r.q_settle_scale;
    spec_hist_fraction(wp, &sk.hist_num, &sk.hist_den);
    sk.slack = r.h->P.stop_slack;
    if (pl.hist) {
        const size_t o = ((size_t)s * nw + wp) * r.B, half = ln.hist.H.n / 2;
        sk.h_in = ln.hist.H.p + (size_t)(ln.hist.par ^ 1) * half + o;
        sk.h_out = ln.hist.H.p + (size_t)ln.hist.par * half + o;
    }
    if (r.first_of_scale) {   // a replay of the scale's first block must see p = 0 in the input set as well
        const size_t n = (size_t)Lv.g.ps * r.B;
        if ((rc = zero_planes4(ln.pbuf[0], n, r.st))) return rc;
        float *const p3[4] = {ln.pbuf[0][4], ln.pbuf[0][5], ln.pbuf[0][4], ln.pbuf[0][5]};
        if (r.h->P.gamma != 0.0 && (rc = zero_planes4(p3, n, r.st))) return rc;
    }
    int e_prev = 0;
    int fb_next = pl.fb ? spec_first_poll(plan, hprev, wp > 0 ? r.fb_prev_warp : r.fb_prev_scale) : -1;
    int fb_done_at = (int)plan.size();
    for (size_t k = 0; k <= plan.size(); ++k) {
        const bool last = k == plan.size();
        const int T = last ? plan.back() : plan[k];
        if (!last) t_after -= T;
        Ctl a = r.ctl;
        a.q = r.q; a.q_prev = r.q_last; a.first_of_warp = (k == 0); a.reset_cur = (k == 0 && r.first_of_scale); a.n = 0;
        sk.e0_prev = e_prev; sk.final_launch = last ? 1 : 0; sk.t_after = t_after;
        if (pl.fb_poll) {
            ln.fb.seq = (ln.fb.seq + 1) & 0x0fffffff;
            sk.fb_flag = ln.fb.flag.p; sk.fb_seq = ln.fb.seq;
        }
        MI_REQUIRE((long long)r.e_next + T <= ln.loop.Q && r.q < ln.loop.Q, MI_ERR_BAD_ARG,
                   "speculative steps: error-sum slot %d + %d or launch slot %d beyond the %lld slots sized for this calc", r.e_next, T, r.q, ln.loop.Q);
        // (the host feedback's cost model may have changed the block lengths: the same rule picks their kernel)
        const TbKernel kern = tb_kernel(TbUse::Spec, T, Lv.g, r.h->P.gamma != 0.0, w.nograd, r.K);
        if ((rc = iterate_tb_spec(kern, T, r.planes, Lv.g, r.l_t, r.theta, r.taut, a, sk, r.e_next, r.st))) return rc;
        ln.loop.slots.push_back({s, wp});
        r.q_last = r.q++;
        ++*nlaunch;
        e_prev = r.e_next;
        if (!last) r.e_next += T;
        if (!pl.fb || last || (int)k != fb_next) continue;
        // The next warp's kernel goes in BEHIND this launch before the host knows whether the warp has stopped (Ctl::need_done) and is
        // enqueued again, unconditionally, where one did not.  With the estimate right the device never waits for the host between
        // two warps of a scale.
        const bool ahead = pl.fb_poll && r.K.fb_ahead != 0 && r.K.x_skip == 0 && !r.h->profiling && wp + 1 < nw;
        if (ahead && (rc = launch_warp(r, Lv, true))) return rc;
        Feedback f;
        if ((rc = pl.fb_poll ? poll_feedback(r, ln.fb.seq, &f) : copy_feedback(r, &f))) return rc;
        if (f.all) {
            r.pre_warped = ahead;
            if (pl.fb_poll && pl.hist) ln.fb.hist[(size_t)s * nw + wp] = f.n_most;
            fb_done_at = f.all_before ? (int)k - 1 : (int)k;   // where the next warp's first read-back goes
            break;
        }
        fb_next = (int)k + 2;
    }
    if (pl.fb) {
        r.fb_prev_warp = fb_done_at;
        if (wp == 0) r.fb_prev_scale = fb_done_at;
    }
    r.q_settle_prev = r.q_last;
    if (wp == 0) r.q_settle_scale = r.q_last;
    r.first_of_scale = false;
    return MI_OK;
}

// The warp wp of scale s and its iterations, in the plan's form (with their profiling regions)
int run_warp(Run &r, LevelBuf &Lv, int s, int wp)
{
    const TvWarp &w = r.pl.warp[s][wp];
    const Geo &g = Lv.g;
    const bool prof = r.h->profiling;
    int rc, w0 = -1, w1 = -1, e0 = -1, e1 = -1;
    r.planes.g = r.grad = w.nograd ? nullptr : r.ln.scr[4];
    if (prof && (rc = record(r, &w0))) return rc;
    if (r.pre_warped) r.pre_warped = false;
    else if (w.warp_launch && (rc = launch_warp(r, Lv, false))) return rc;
    if (prof && !w.fused) {
        if ((rc = record(r, &w1))) return rc;
        r.ln.prof.regions.push_back({w0, w1, 1, 44.0 * g.w * g.h * r.B, 1, s});   // 44 B/px per warp
    }
    if (prof && r.pl.iters > 0 && (rc = record(r, &e0))) return rc;
    long long nlaunch = 0;
    switch (w.form) {
    case TvForm::Blocked:
    case TvForm::ExactBlocked: rc = run_blocked(r, Lv, w, &nlaunch); break;
    case TvForm::Spec: rc = run_spec(r, Lv, w, s, wp, &nlaunch); break;
    case TvForm::PerIter: rc = run_per_iteration(r, Lv, s, wp, &nlaunch); break;
    }
    if (rc) return rc;
    if (e0 >= 0) {
        if ((rc = record(r, &e1))) return rc;
        r.ln.prof.regions.push_back({e0, e1, nlaunch, 64.0 * g.w * g.h * r.B * r.pl.iters, 0, s});
    }
    return MI_OK;
}

// scale s done: the flow to the caller (s = 0) or zoomed to the next finer scale and rescaled (tvl1flow.cpp:291-300; u3 is zoomed too
// but NOT rescaled, optflow tvl1flow.cpp:524-528)
int zoom_or_pack(Run &r, int s)
{
    const mi_tvl1_params &P = r.h->P;
    const LevelBuf &Lv = r.ln.L[s];
    Ctl ec = r.ctl;
    ec.q_prev = r.q_last;
    const Ctl *dev = r.pl.check && !r.first_of_scale ? &ec : nullptr;
    if (s == 0) {
        if (!r.pl.warp[0].empty() && r.pl.warp[0].back().pack_in_pass) return MI_OK;   // the last pass wrote the callers' matrices itself
        const float *u1v[2] = {Lv.u[0][0], Lv.u[1][0]}, *u2v[2] = {Lv.u[0][1], Lv.u[1][1]};
        return pack_flow(r.ln.tab.p, u1v, u2v, Lv.g, dev, r.cur, r.st);
    }
    const LevelBuf &Lf = r.ln.L[s - 1];
    const bool gam = P.gamma != 0.0;
    const float *us[3][2] = {{Lv.u[0][0], Lv.u[1][0]}, {Lv.u[0][1], Lv.u[1][1]}, {gam ? Lv.u[0][2] : nullptr, gam ? Lv.u[1][2] : nullptr}};
    float *ud[3] = {Lf.u[0][0], Lf.u[0][1], gam ? Lf.u[0][2] : nullptr};
    const float post[3] = {(float)(1.0 / P.scale_step), (float)(1.0 / P.scale_step), 1.f};
    return resize(P.semantics, gam ? 3 : 2, us, 2, ud, Lv.g, Lf.g, (double)Lf.g.w / Lv.g.w, (double)Lf.g.h / Lv.g.h, post, dev, r.cur, r.st);
}

}  // namespace

// The whole coarse-to-fine computation of n pairs on one stream (OpticalFlowDual_TVL1_Impl::calcImpl + procOneScale): the plan of the
// calc (tvl1_plan.h), executed.
static int lane_calc(mi_tvl1 *h, Lane &ln, int n, const mi_mat *I0s, const mi_mat *I1s, mi_mat *flows, hipStream_t st, int *ns_out)
{
    // behind everything this call enqueues for the lane (also on an error return: part of the calc may be in flight): the event the
    // arena cache waits for before it hands the lane's block to somebody else
    struct Mark { HipArena &a; hipStream_t s; ~Mark() { a.mark(s); } } mark{ln.arena.blk, st};
    const mi_tvl1_params &P = h->P;
    hipStreamCaptureStatus cap_st = hipStreamCaptureStatusNone;
    const bool capturing = hipStreamIsCapturing(st, &cap_st) == hipSuccess && cap_st != hipStreamCaptureStatusNone;
    const TvPlan pl = tv_make_plan(TvShape{I0s[0].cols, I0s[0].rows, n, I0s[0].type, P, h->last_lanes, capturing}, tv_knobs());
    int rc = ensure_arena(P, ln, pl, I0s[0].cols, I0s[0].rows, n);
    if (rc || (rc = ensure_buffers(pl, ln, n, I0s, I1s, flows, st))) return rc;
    if (!pl.warp.empty() && !pl.warp[0].empty() && pl.warp[0].back().pack_in_pass)   // the pass keeps the matrices' pitch in 32 bits
        for (int i = 0; i < n; ++i) MI_REQUIRE(flows[i].step < (1ll << 31), MI_ERR_BAD_ARG, "flow matrix pitch of %lld bytes", (long long)flows[i].step);
    *ns_out = pl.used;
    ln.loop.slots.clear();
    ln.prof.regions.clear();

    Run r{h, ln, pl, tv_knobs(), st, n};
    memset(&r.ctl, 0, sizeof(r.ctl));
    r.ctl.S = ln.loop.S.p; r.ctl.E = ln.loop.E.p; r.ctl.Q = (int)ln.loop.Q; r.ctl.P = ln.loop.Pd.p;
    r.ctl.sched = P.semantics == MI_SEM_CUDA_COMPAT ? 1 : 0;   // cv::cuda's check schedule vs the CPU class's every-iteration check
    r.l_t = (float)(P.lambda * P.theta); r.taut = (float)(P.tau / P.theta); r.theta = (float)P.theta;
    if ((rc = enqueue_pyramid(r, I0s[0].type))) return rc;
    for (int s = pl.used - 1; s >= 0; --s) {
        LevelBuf &Lv = ln.L[s];
        IterPlanes &ip = r.planes;
        ip.ix = ln.scr[2]; ip.iy = ln.scr[3]; ip.rc = ln.scr[5]; ip.gamma = (float)P.gamma;
        for (int k = 0; k < 2; ++k) { for (int j = 0; j < 3; ++j) ip.u[k][j] = Lv.u[k][j]; for (int j = 0; j < 6; ++j) ip.p[k][j] = ln.pbuf[k][j]; }
        ip.err_u3 = P.semantics == MI_SEM_CPU_REF ? 1 : 0;   // optflow tvl1flow.cpp:1110 vs cuda tvl1flow.cu:276-283
        r.cur = 0; r.first_of_scale = true; r.pre_warped = false;
        // scaledEpsilon: float in the CPU class (optflow tvl1flow.cpp:1315), double in cv::cuda (:310)
        const double se = P.epsilon * P.epsilon * (double)(Lv.g.w * Lv.g.h);
        r.ctl.thr = P.semantics == MI_SEM_CPU_REF ? (double)(float)se : se;
        for (int wp = 0; wp < P.warps; ++wp)
            if ((rc = run_warp(r, Lv, s, wp))) return rc;
        if ((rc = zoom_or_pack(r, s))) return rc;
    }
    return MI_OK;
}

int mi_tvl1_calc_batch(mi_tvl1 *h, int n, const mi_mat *I0s, const mi_mat *I1s, mi_mat *flows, void *stream_)
{
    MI_REQUIRE(h, MI_ERR_BAD_ARG, "null handle");
    MI_REQUIRE(n > 0 && I0s && I1s && flows, MI_ERR_BAD_ARG, "empty batch");
    hipStream_t st = (hipStream_t)stream_;
    for (int i = 0; i < n; ++i) {
        int rc = check_pair(&I0s[i], &I1s[i], &flows[i], &I0s[0]);
        if (rc) return rc;
    }
    // Lanes: a batch of >= 4 pairs is split into contiguous sub-batches that run concurrently, forked from and joined to the
    // caller's stream with events (stream-ordered for the caller exactly like the single-stream form).  The pairs are
    // independent, so the result is bit-identical to running them in one lane.
    int lanes = h->P.lanes > 0 ? h->P.lanes : (tuning().lanes > 0 ? tuning().lanes : (n >= 4 ? 2 : 1));
    if (lanes > mi_tvl1::kMaxLanes) lanes = mi_tvl1::kMaxLanes;
    if (lanes > n) lanes = n;
    int ns = 0;
    h->last_check = h->P.epsilon > 0.0 && h->P.iterations * h->P.inner_iterations > 0;
    h->last_batch = n; h->last_lanes = lanes;
    for (int i = 0; i <= lanes; ++i) h->last_first[i] = (int)((long long)n * i / lanes);   // contiguous, sizes differ by at most one
    if (lanes == 1) {
        int rc = lane_calc(h, h->lane[0], n, I0s, I1s, flows, st, &ns);
        if (rc) return rc;
    } else {
        // Lane 0 runs on the caller's own stream, every further lane on ONE internal stream each: a handle adds lanes - 1 streams
        // to the process.  (HIP multiplexes streams onto a few hardware queues -- 4 by default, GPU_MAX_HW_QUEUES; two lanes that
        // land on one queue run back to back: measured 400 instead of 520 pairs/s when enough streams of other handles were alive.)
        // every stream and event the fork / join needs exists BEFORE anything is enqueued, so no failure between the fork and the
        // join can leave an internal lane un-joined
        MI_TRY(h->fork.ensure());
        for (int li = 1; li < lanes; ++li) {
            Lane &ln = h->lane[li];
            MI_TRY(ln.internal.stream.ensure());
            MI_TRY(ln.internal.done.ensure());
        }
        MI_HIP_TRY(hipEventRecord(h->fork.get(), st));
        int rc_first = MI_OK;
        auto note = [&](hipError_t e) {
            if (e != hipSuccess && !rc_first) { set_error("HIP error in the lane fork / join: %s", hipGetErrorString(e)); rc_first = MI_ERR_HIP; }
            return e == hipSuccess;
        };
        for (int li = lanes - 1; li >= 0; --li) {   // the internal lanes first: they start while lane 0 is still being enqueued
            Lane &ln = h->lane[li];
            const int off = h->last_first[li], cnt = h->last_first[li + 1] - off;
            hipStream_t ls = li > 0 ? ln.internal.stream.get() : st;
            // a lane that could not be forked behind the caller's stream must not run at all (it would read inputs too early)
            const bool forked = li == 0 || note(hipStreamWaitEvent(ln.internal.stream.get(), h->fork.get(), 0));
            if (forked && !rc_first) {
                const int rc = lane_calc(h, ln, cnt, I0s + off, I1s + off, flows + off, ls, &ns);
                if (rc && !rc_first) rc_first = rc;
            }
        }
        // always join, also after an error: the caller's stream must not run ahead of work already enqueued.  If the join itself
        // fails, fall back to blocking the host until the lane has drained.
        for (int li = 1; li < lanes; ++li) {
            auto &in = h->lane[li].internal;
            if (!(note(hipEventRecord(in.done.get(), in.stream.get())) && note(hipStreamWaitEvent(st, in.done.get(), 0)))) (void)hipStreamSynchronize(in.stream.get());
        }
        if (rc_first) return rc_first;
    }
    h->last_nscales = ns;
    // the reference shrinks nscales_ for good when a level falls below 16 px (tvl1flow.cpp:243-247: `nscales_ = s; break;`)
    if (ns < h->P.nscales) h->P.nscales = ns;
    return MI_OK;
}

int mi_tvl1_calc(mi_tvl1 *h, const mi_mat *I0, const mi_mat *I1, mi_mat *flow, void *stream)
{
    return mi_tvl1_calc_batch(h, 1, I0, I1, flow, stream);
}

// the control slots (and the speculative steps' state) of the last calc's launches for one pair, after the stream has drained
static int read_slots(mi_tvl1 *h, int pair, hipStream_t stream, const Lane **lane, std::vector<int2> *S, std::vector<int4> *X,
                      int cap_launches = -1)
{
    int li = 0;
    while (li + 1 < h->last_lanes && pair >= h->last_first[li + 1]) ++li;
    const Lane &ln = h->lane[li];
    const size_t off = (size_t)(pair - h->last_first[li]) * ln.loop.Q;
    const int nq = (int)ln.loop.slots.size();
    MI_REQUIRE(cap_launches < 0 || nq <= cap_launches, MI_ERR_BAD_ARG, "capacity too small");
    *lane = &ln;
    S->resize(nq);
    MI_HIP_TRY(hipStreamSynchronize(stream));
    MI_HIP_TRY(hipMemcpy(S->data(), ln.loop.S.p + off, sizeof(int2) * nq, hipMemcpyDeviceToHost));
    if (X) {
        X->resize(nq);
        if (ln.loop.X.p) MI_HIP_TRY(hipMemcpy(X->data(), ln.loop.X.p + off, sizeof(int4) * nq, hipMemcpyDeviceToHost));
    }
    return MI_OK;
}

int mi_tvl1_last_iterations(mi_tvl1 *h, int pair, int *nscales_used, int *iters, int cap, void *stream)
{
    MI_REQUIRE(h && iters && nscales_used, MI_ERR_BAD_ARG, "null argument");
    MI_REQUIRE(pair >= 0 && pair < h->last_batch, MI_ERR_BAD_ARG, "pair index out of range");
    const int ns = h->last_nscales, nw = h->P.warps;
    MI_REQUIRE(cap >= ns * nw, MI_ERR_BAD_ARG, "iters capacity too small");
    *nscales_used = ns;
    for (int i = 0; i < ns * nw; ++i) iters[i] = 0;
    if (!h->last_check) {
        for (int i = 0; i < ns * nw; ++i) iters[i] = h->P.iterations * h->P.inner_iterations;
        return MI_OK;
    }
    const Lane *ln = nullptr;
    std::vector<int2> S;
    if (const int rc = read_slots(h, pair, (hipStream_t)stream, &ln, &S, nullptr)) return rc;
    for (size_t i = 0; i < S.size(); ++i) {
        // one-iteration launches: bit 0 = the iteration was executed; speculative launches: bits 8..15 = iterations kept
        const int k = (S[i].y >> 8) & 0xff;
        iters[ln->loop.slots[i].scale * nw + ln->loop.slots[i].warp] += k ? k : (S[i].y & 1);
    }
    return MI_OK;
}

int miflow_selftest_tvl1_slots(mi_tvl1 *h, int pair, int *out_host, int cap_launches, void *stream)
{
    MI_REQUIRE(h && out_host, MI_ERR_BAD_ARG, "null argument");
    MI_REQUIRE(pair >= 0 && pair < h->last_batch, MI_ERR_BAD_ARG, "pair out of range");
    if (!h->last_check) return 0;
    const Lane *ln = nullptr;
    std::vector<int2> S;
    std::vector<int4> X;
    if (const int rc = read_slots(h, pair, (hipStream_t)stream, &ln, &S, &X, cap_launches)) return rc;
    const int nq = (int)S.size();
    for (int i = 0; i < nq; ++i) {
        int *o = out_host + 8 * i;
        o[0] = ln->loop.slots[i].scale; o[1] = ln->loop.slots[i].warp; o[2] = S[i].x; o[3] = S[i].y;
        o[4] = X[i].x; o[5] = X[i].y; o[6] = X[i].z; o[7] = X[i].w;
    }
    return nq;
}
