// cv::cuda::ORB: handle + C-ABI entry points.  Host-side twin of ORB_Impl (modules/cudafeatures2d/src/orb.cpp:340-913): validation, the
// plan (orb_plan.h), scratch, the plan's launches in order on the caller's stream, and ONE read-back of the per-level counts at the end of
// a call (the reference waits at every level: FAST's two, and every null-stream kernel wrapper's cudaDeviceSynchronize).
#include <cstring>
#include "fast_dev.h"
#include "orb_dev.h"
#include "mi_buf.h"

using namespace mi;

static_assert(sizeof(orb::OrbLevelDev) <= orb::ORB_LEVEL_DEV_BYTES, "the plan reserves ORB_LEVEL_DEV_BYTES per level of the device table");

struct mi_orb {
    mi_orb_params P;
    bool has_pool = false;
    int pool[2 * orb::ORB_NPOINTS];                // the caller's pattern0
    int pattern[2 * orb::ORB_NPOINTS];             // the 2 x N matrix the reference uploads
    int pattern_cols = 0, pattern_reach = 0;
    int u_max[orb::ORB_UMAX_N];
    orb::OrbTaps taps;
    DevBuf<int> consts;                            // pattern, then u_max
    DevBuf<unsigned char> scratch;                 // orb_plan.h
    PinnedBuf<unsigned char, hipHostMallocDefault> stage;   // the level table and provided keypoints on their way up, the counts on their way down
};

namespace {

// getGaussianKernel(7, 2, CV_32F) (main repository imgproc): exp and the normalisation in double, stored as f32
orb::OrbTaps gaussian_taps()
{
    const int n = 7;
    const double sigma = 2.0, scale2x = -0.5 / (sigma * sigma);
    double t[7], sum = 0;
    for (int i = 0; i < n; ++i) { const double x = i - (n - 1) * 0.5; t[i] = std::exp(scale2x * x * x); sum += t[i]; }
    const double inv = 1.0 / sum;
    orb::OrbTaps k;
    for (int i = 0; i < n; ++i) k.k[i] = (float)(t[i] * inv);
    return k;
}

int check_pool(const mi_mat *pattern0)
{
    MI_REQUIRE(pattern0->data, MI_ERR_BAD_ARG, "pattern0: null data");
    MI_REQUIRE(pattern0->type == MI_32SC1, MI_ERR_BAD_TYPE, "pattern0.type() == CV_32SC1");
    MI_REQUIRE(pattern0->rows == orb::ORB_NPOINTS && pattern0->cols == 2, MI_ERR_BAD_SIZE, "pattern0 must be 512 x 2 {x, y}");
    MI_REQUIRE(pattern0->step >= 8 && pattern0->step % 4 == 0, MI_ERR_BAD_ARG, "pattern0: bad step");
    return MI_OK;
}

void read_pool(const mi_mat *pattern0, int *pool)
{
    for (int i = 0; i < orb::ORB_NPOINTS; ++i) std::memcpy(pool + 2 * i, (const char *)pattern0->data + (size_t)i * pattern0->step, 8);
}

// host-side state that follows the parameters: pattern, its reach, u_max
void derive(mi_orb *h)
{
    orb::orb_make_pattern(h->P.patch_size, h->P.wta_k, h->has_pool ? h->pool : nullptr, h->pattern);
    h->pattern_cols = orb::orb_pattern_cols(h->P.wta_k);
    h->pattern_reach = orb::orb_pattern_reach(h->pattern, h->pattern_cols);
    orb::orb_u_max(h->P.patch_size, h->u_max);
    h->taps = gaussian_taps();
}

int upload_consts(mi_orb *h)
{
    MI_TRY(h->consts.ensure((size_t)2 * orb::ORB_NPOINTS + orb::ORB_UMAX_N));
    MI_HIP_TRY(hipMemcpy(h->consts.p, h->pattern, sizeof(int) * 2 * h->pattern_cols, hipMemcpyHostToDevice));
    MI_HIP_TRY(hipMemcpy(h->consts.p + 2 * orb::ORB_NPOINTS, h->u_max, sizeof(h->u_max), hipMemcpyHostToDevice));
    return MI_OK;
}

int check_u8(const mi_mat *m, const char *what)
{
    MI_REQUIRE(m && m->data, MI_ERR_BAD_ARG, "%s: null", what);
    MI_REQUIRE(m->type == MI_8UC1, MI_ERR_BAD_TYPE, "%s.type() == CV_8UC1", what);
    MI_REQUIRE(m->rows >= 1 && m->cols >= 1 && m->rows <= fast::FAST_MAX_SIDE && m->cols <= fast::FAST_MAX_SIDE, MI_ERR_BAD_SIZE,
               "%s: 1 .. 32767 rows and cols", what);
    MI_REQUIRE(m->step >= (size_t)m->cols && m->step < ((size_t)1 << 31), MI_ERR_BAD_ARG, "%s: bad step", what);
    return MI_OK;
}

// a keyPointsPyr_-style matrix: >= min_rows rows, >= n columns of 4-byte elements
int check_kp(const mi_mat *m, int min_rows, int n, const char *what)
{
    MI_REQUIRE(m && m->data, MI_ERR_BAD_ARG, "%s: null", what);
    MI_REQUIRE(m->type == MI_32FC1 || m->type == MI_32SC1, MI_ERR_BAD_TYPE, "%s.elemSize() == 4", what);
    MI_REQUIRE(m->rows >= min_rows && n >= 0 && m->cols >= n, MI_ERR_BAD_SIZE, "%s must be (at least %d) x (at least n)", what, min_rows);
    MI_REQUIRE(m->step % 4 == 0 && m->step >= (size_t)m->cols * 4, MI_ERR_BAD_ARG, "%s: bad step", what);
    return MI_OK;
}

template <class T> T *row_of(const mi_mat *m, int r) { return (T *)((unsigned char *)m->data + (size_t)r * m->step); }

fast::FastScratch fast_scratch(unsigned char *area, const fast::FastPlan &fp, int *counts)
{
    const fast::FastFrame &f = fp.frames[0];
    unsigned char *a = area + fp.counts_bytes;
    return {a + f.off_plane, (unsigned long long *)(a + f.off_cand), (unsigned long long *)(a + f.off_surv), (unsigned long long *)(a + f.off_emit),
            (int *)(a + f.off_pos), counts};
}

// the device table of a plan's levels over `base`
void fill_table(const orb::OrbPlan &plan, unsigned char *base, orb::OrbLevelDev *tab)
{
    for (int l = 0; l < plan.nlevels; ++l) {
        const orb::OrbLevel &v = plan.levels[l];
        orb::OrbLevelDev &d = tab[l];
        d.img = base + v.off_img;
        d.dimg = plan.blur ? base + v.off_blur : d.img;
        for (int k = 0; k < 3; ++k) { d.loc[k] = (int *)(base + v.off_kp[k]); d.resp[k] = (float *)(d.loc[k] + v.cap[k]); }
        d.keys = (unsigned *)(base + v.off_key);
        d.angle = (float *)(base + v.off_angle);
        d.counts = (int *)(base + plan.off_counts) + 4 * l;
        d.pitch = v.pitch; d.rows = v.rows; d.cols = v.cols; d.quota = v.quota;
        d.loc_scale = v.loc_scale; d.size = v.size;
    }
}

struct Provided {   // keypoints on their way up, grouped by level
    std::vector<int> count, loc;
    std::vector<float> angle;
};

int run_plan_body(mi_orb *h, const orb::OrbPlan &plan, const mi_mat *img, const mi_mat *mask, mi_mat *kp, mi_mat *desc, const Provided *pv, int *n,
             hipStream_t st)
{
    const mi_orb_params &P = h->P;
    const bool masked = mask && mask->data;
    MI_TRY(h->scratch.ensure(plan.scratch_bytes));
    const size_t tab_bytes = sizeof(orb::OrbLevelDev) * orb::ORB_MAX_LEVELS, cnt_bytes = sizeof(int) * 4 * orb::ORB_MAX_LEVELS;
    const size_t npv = pv ? pv->loc.size() : 0;
    MI_TRY(h->stage.ensure(tab_bytes + cnt_bytes + npv * 8));
    unsigned char *base = h->scratch.p;
    orb::OrbLevelDev *tab = (orb::OrbLevelDev *)h->stage.p;
    int *hcounts = (int *)(h->stage.p + tab_bytes);
    const orb::OrbLevelDev *dtab = (const orb::OrbLevelDev *)(base + plan.off_table);
    fill_table(plan, base, tab);
    int *hist = (int *)(base + plan.off_hist);
    unsigned *state = (unsigned *)(base + plan.off_state);
    const int *dpattern = h->consts.p, *dumax = h->consts.p + 2 * orb::ORB_NPOINTS;

    for (const orb::OrbLaunch &k : plan.launches) {
        const orb::OrbLevel *v = k.level >= 0 ? &plan.levels[k.level] : nullptr;
        switch (k.kernel) {
        case orb::ORB_K_CLEAR: {
            MI_HIP_TRY(hipMemsetAsync(base, 0, plan.head_bytes, st));
            MI_HIP_TRY(hipMemcpyAsync(base + plan.off_table, tab, sizeof(orb::OrbLevelDev) * plan.nlevels, hipMemcpyHostToDevice, st));
            if (pv) {
                std::memset(hcounts, 0, cnt_bytes);
                int *sloc = (int *)(h->stage.p + tab_bytes + cnt_bytes);
                float *sang = (float *)(sloc + npv);
                size_t o = 0;
                for (int l = 0; l < plan.nlevels; ++l) {
                    const int c = pv->count[l];
                    hcounts[4 * l + 3] = c;
                    if (!c) continue;
                    std::memcpy(sloc + o, pv->loc.data() + o, sizeof(int) * c);
                    std::memcpy(sang + o, pv->angle.data() + o, sizeof(float) * c);
                    MI_HIP_TRY(hipMemcpyAsync(tab[l].loc[2], sloc + o, sizeof(int) * c, hipMemcpyHostToDevice, st));
                    MI_HIP_TRY(hipMemcpyAsync(tab[l].angle, sang + o, sizeof(float) * c, hipMemcpyHostToDevice, st));
                    o += c;
                }
                MI_HIP_TRY(hipMemcpyAsync(base + plan.off_counts, hcounts, cnt_bytes, hipMemcpyHostToDevice, st));
            }
            break;
        }
        case orb::ORB_K_LEVEL: {
            orb::OrbPlaneSrc src, msrc = {nullptr, 0, 0, 0};
            if (v->src < 0) {
                src = {(const unsigned char *)img->data, (long long)img->step, img->rows, img->cols};
                if (masked) msrc = {(const unsigned char *)mask->data, (long long)mask->step, mask->rows, mask->cols};
            } else {
                const orb::OrbLevel &s = plan.levels[v->src];
                src = {base + s.off_img, s.pitch, s.rows, s.cols};
                if (masked) msrc = {base + s.off_mask, s.pitch, s.rows, s.cols};
            }
            MI_TRY(orb::level(k, src, msrc, v->mask_mode, v->fx, v->fy, P.edge_threshold, base + v->off_img, v->pitch,
                              plan.detect ? base + v->off_mask : nullptr, v->pitch, v->rows, v->cols, st));
            break;
        }
        case orb::ORB_K_FAST: {
            const fast::FastPlan &fp = v->fast;
            const fast::FastLaunch &fk = fp.launches[k.arg];
            const fast::FastFrame &f = fp.frames[0];
            const fast::FastImage im = {base + v->off_img, v->pitch, base + v->off_mask, v->pitch, v->rows, v->cols};
            const fast::FastScratch s = fast_scratch(base + v->off_fast, fp, tab[k.level].counts);
            switch (fk.kernel) {
            case fast::FAST_K_SCORE: MI_TRY(fast::score(fk, f, im, fp.threshold, s, st)); break;
            case fast::FAST_K_NMS: MI_TRY(fast::nms(fk, f, s, st)); break;
            case fast::FAST_K_SCAN: MI_TRY(fast::scan(fk, f, s, true, fp.max_npoints, st)); break;
            case fast::FAST_K_EMIT: MI_TRY(fast::emit(fk, f, s, true, tab[k.level].loc[0], tab[k.level].resp[0], st)); break;
            }
            break;
        }
        case orb::ORB_K_HIST: MI_TRY(orb::hist(k, dtab, hist, state, plan.ncull, st)); break;
        case orb::ORB_K_RANK: MI_TRY(orb::rank(k, dtab, hist, state, plan.ncull, st)); break;
        case orb::ORB_K_HARRIS: MI_TRY(orb::harris(k, dtab, 1, st)); break;
        case orb::ORB_K_ANGLE: MI_TRY(orb::angle(k, dtab, dumax, P.patch_size / 2, nullptr, nullptr, st)); break;
        case orb::ORB_K_BLUR: MI_TRY(orb::blur(k, base + v->off_img, v->pitch, base + v->off_blur, v->pitch, v->rows, v->cols, h->taps, st)); break;
        case orb::ORB_K_DESC:
            MI_TRY(orb::descriptors(k, dtab, dpattern, h->pattern_cols, P.wta_k, (unsigned char *)desc->data, (long long)desc->step, desc->rows, st));
            break;
        case orb::ORB_K_MERGE: MI_TRY(orb::merge(k, dtab, (unsigned char *)kp->data, (long long)kp->step, kp->cols, st)); break;
        case orb::ORB_K_READBACK:
            MI_HIP_TRY(hipMemcpyAsync(hcounts, base + plan.off_counts, sizeof(int) * 4 * plan.nlevels, hipMemcpyDeviceToHost, st));
            break;
        }
    }
    MI_HIP_TRY(hipStreamSynchronize(st));   // the one wait: the counts are down, and the staging area is free for the next call
    if (!pv) {
        *n = 0;
        for (int l = 0; l < plan.nlevels; ++l) *n += hcounts[4 * l + 3];
    }
    return MI_OK;
}

// a call that fails half way still waits for what it enqueued: the copies out of the pinned staging area must not outlive the call
int run_plan(mi_orb *h, const orb::OrbPlan &plan, const mi_mat *img, const mi_mat *mask, mi_mat *kp, mi_mat *desc, const Provided *pv, int *n,
             hipStream_t st)
{
    const int rc = run_plan_body(h, plan, img, mask, kp, desc, pv, n, st);
    if (rc) (void)hipStreamSynchronize(st);
    return rc;
}

int detect(mi_orb *h, const mi_mat *img, const mi_mat *mask, mi_mat *kp, mi_mat *desc, int *n, hipStream_t st)
{
    const orb::OrbPlan plan = orb::orb_make_plan(h->P, h->pattern_reach, img->rows, img->cols, true, desc != nullptr);
    MI_TRY(orb::orb_fail(plan.err));
    MI_REQUIRE(kp && kp->data, MI_ERR_BAD_ARG, "keypoints: null");
    MI_REQUIRE(kp->type == MI_32FC1, MI_ERR_BAD_TYPE, "keypoints.type() == CV_32FC1");
    MI_REQUIRE(kp->rows == orb::ORB_ROWS_COUNT && kp->cols >= plan.max_total, MI_ERR_BAD_SIZE, "keypoints must be 6 x (at least %d)", plan.max_total);
    MI_REQUIRE(kp->step % 4 == 0 && kp->step >= (size_t)kp->cols * 4, MI_ERR_BAD_ARG, "keypoints: bad step");
    if (desc) {
        MI_REQUIRE(desc->data || plan.max_total == 0, MI_ERR_BAD_ARG, "descriptors: null data");
        MI_REQUIRE(desc->type == MI_8UC1, MI_ERR_BAD_TYPE, "descriptors.type() == CV_8UC1");
        MI_REQUIRE(desc->rows >= plan.max_total && desc->cols >= orb::ORB_DESC_BYTES && desc->step >= (size_t)desc->cols, MI_ERR_BAD_SIZE,
                   "descriptors must be (at least %d) x 32", plan.max_total);
    }
    return run_plan(h, plan, img, mask, kp, desc, nullptr, n, st);
}

int compute_provided(mi_orb *h, const mi_mat *img, mi_mat *kp, mi_mat *desc, int *n, hipStream_t st)
{
    MI_REQUIRE(kp && kp->data && *n >= 0, MI_ERR_BAD_ARG, "provided keypoints: a host 6 x n matrix");
    MI_REQUIRE(kp->type == MI_32FC1 && kp->rows == orb::ORB_ROWS_COUNT && kp->cols >= *n, MI_ERR_BAD_SIZE, "provided keypoints must be 6 x n CV_32FC1");
    MI_REQUIRE(kp->step % 4 == 0 && kp->step >= (size_t)kp->cols * 4, MI_ERR_BAD_ARG, "keypoints: bad step");
    const int N = *n;
    if (N == 0) return MI_OK;   // orb.cpp:601,793-797: nothing to describe
    MI_REQUIRE(desc && desc->data, MI_ERR_BAD_ARG, "descriptors: null");
    MI_REQUIRE(desc->type == MI_8UC1, MI_ERR_BAD_TYPE, "descriptors.type() == CV_8UC1");
    MI_REQUIRE(desc->rows >= N && desc->cols >= orb::ORB_DESC_BYTES && desc->step >= (size_t)desc->cols, MI_ERR_BAD_SIZE, "descriptors must be (at least n) x 32");
    float *rows[orb::ORB_ROWS_COUNT];
    for (int r = 0; r < orb::ORB_ROWS_COUNT; ++r) rows[r] = row_of<float>(kp, r);
    int L = 0;
    for (int j = 0; j < N; ++j) {
        const int level = (int)rows[4][j];
        MI_REQUIRE(level >= 0 && level < orb::ORB_MAX_LEVELS, MI_ERR_BAD_ARG, "0 <= octave < 32");   // orb.cpp:591
        L = std::max(L, level + 1);
    }
    // validate first: the order by octave (stable, orb.cpp:595-600), the plan and every location; a rejected call changes nothing
    std::vector<int> order;
    Provided pv;
    pv.count.assign(L, 0);
    for (int t = 0; t < L; ++t)
        for (int j = 0; j < N; ++j)
            if ((int)rows[4][j] == t) { order.push_back(j); ++pv.count[t]; }
    mi_orb_params P = h->P;
    P.nlevels = L;   // orb.cpp:587-594
    const orb::OrbPlan plan = orb::orb_make_plan(P, h->pattern_reach, img->rows, img->cols, false, true, pv.count.data(), L);
    MI_TRY(orb::orb_fail(plan.err));
    pv.loc.resize(N); pv.angle.resize(N);
    for (int i = 0; i < N; ++i) {
        const int j = order[i];
        const orb::OrbLevel &v = plan.levels[(int)rows[4][j]];
        const float scale = 1.f / v.loc_scale;   // orb.cpp:612-625
        const int x = orb::cv_round(rows[0][j] * scale), y = orb::cv_round(rows[1][j] * scale);
        MI_REQUIRE(x >= plan.reach && x < v.cols - plan.reach && y >= plan.reach && y < v.rows - plan.reach, MI_ERR_BAD_ARG,
                   "provided keypoint %d is nearer than R = %d to the border of its level (the reference reads out of bounds)", j, plan.reach);
        pv.loc[i] = (int)((unsigned)(x & 0xffff) | ((unsigned)(y & 0xffff) << 16));
        pv.angle[i] = rows[3][j];
    }
    // the object's nlevels is overwritten for the run (run_plan reads h->P) and put back if the run fails; the caller's columns are
    // regrouped only after it succeeded: a failed call, at validation or at run time, changes neither
    const mi_orb_params before = h->P;
    h->P = P;
    if (const int rc = run_plan(h, plan, img, nullptr, nullptr, desc, &pv, n, st)) { h->P = before; return rc; }
    for (int r = 0; r < orb::ORB_ROWS_COUNT; ++r) {
        std::vector<float> tmp(N);
        for (int i = 0; i < N; ++i) tmp[i] = rows[r][order[i]];
        std::memcpy(rows[r], tmp.data(), sizeof(float) * N);
    }
    return MI_OK;
}

// ---- the stage entries' one-level plumbing: a table of one level over temporaries
struct Stage {
    DevTmp tmp;
    unsigned char *head = nullptr;   // counts, hist, state as the plan lays them out, then the table
    orb::OrbLevelDev *dtab = nullptr;
    orb::OrbLevelDev lv = {};
    size_t off_hist = 0, off_state = 0, off_table = 0;
    int init(hipStream_t st)
    {
        off_hist = orb::orb_align((size_t)orb::ORB_MAX_LEVELS * 4 * sizeof(int));
        off_state = off_hist + orb::orb_align((size_t)2 * orb::ORB_MAX_LEVELS * orb::ORB_DIGITS * orb::ORB_BINS * sizeof(int));
        off_table = off_state + orb::orb_align((size_t)2 * orb::ORB_MAX_LEVELS * 2 * (orb::ORB_DIGITS + 1) * sizeof(unsigned));
        MI_TRY(tmp.alloc(&head, off_table + sizeof(orb::OrbLevelDev)));
        MI_HIP_TRY(hipMemsetAsync(head, 0, off_table, st));
        dtab = (orb::OrbLevelDev *)(head + off_table);
        lv.counts = (int *)head;
        return MI_OK;
    }
    // counts[1 + area] = n, and the table
    int upload(int area, int n, hipStream_t st)
    {
        MI_HIP_TRY(hipMemcpyAsync(lv.counts + 1 + area, &n, sizeof(int), hipMemcpyHostToDevice, st));
        MI_HIP_TRY(hipMemcpyAsync(dtab, &lv, sizeof(lv), hipMemcpyHostToDevice, st));
        MI_HIP_TRY(hipStreamSynchronize(st));   // both sources are on this frame
        return MI_OK;
    }
    void image(const mi_mat *img)
    {
        lv.img = lv.dimg = (const unsigned char *)img->data;
        lv.pitch = (int)img->step; lv.rows = img->rows; lv.cols = img->cols;
    }
};

// every location of keypoints[0, :n] at least `reach` inside the image: the stage entries read nothing outside it
int check_locations(const mi_mat *kp, int n, const mi_mat *img, int reach, hipStream_t st)
{
    std::vector<int> loc(n);
    MI_HIP_TRY(hipMemcpyAsync(loc.data(), kp->data, sizeof(int) * n, hipMemcpyDeviceToHost, st));
    MI_HIP_TRY(hipStreamSynchronize(st));
    for (int i = 0; i < n; ++i) {
        const int x = (short)(loc[i] & 0xffff), y = (short)(loc[i] >> 16);
        MI_REQUIRE(x >= reach && x < img->cols - reach && y >= reach && y < img->rows - reach, MI_ERR_BAD_ARG,
                   "keypoint %d (%d, %d) is nearer than %d to the image border", i, x, y, reach);
    }
    return MI_OK;
}

unsigned per_kp(int n) { return (unsigned)((n + orb::ORB_KP_PER_BLOCK - 1) / orb::ORB_KP_PER_BLOCK); }

}  // namespace

extern "C" {

void mi_orb_default_params(mi_orb_params *p)
{
    if (!p) return;
    *p = {500, 1.2f, 8, 31, 0, 2, orb::ORB_HARRIS_SCORE, 31, 20, 0};   // cudafeatures2d.hpp:463-472
}

int mi_orb_create(const mi_orb_params *p, const mi_mat *pattern0, mi_orb **out)
{
    MI_REQUIRE(out, MI_ERR_BAD_ARG, "null out");
    *out = nullptr;
    mi_orb_params P;
    if (p) P = *p; else mi_orb_default_params(&P);
    MI_TRY(orb::orb_fail(orb::orb_check_params(P)));
    if (pattern0) MI_TRY(check_pool(pattern0));
    MI_TRY(require_device());
    mi_orb *h = new mi_orb();
    h->P = P;
    if (pattern0) { read_pool(pattern0, h->pool); h->has_pool = true; }
    derive(h);
    if (const int rc = upload_consts(h)) { delete h; return rc; }
    *out = h;
    return MI_OK;
}

int mi_orb_set_params(mi_orb *h, const mi_orb_params *p)
{
    MI_REQUIRE(h && p, MI_ERR_BAD_ARG, "null argument");
    MI_TRY(orb::orb_fail(orb::orb_check_params(*p)));
    const mi_orb_params old = h->P;
    h->P = *p;
    derive(h);
    const int rc = upload_consts(h);
    if (rc) {   // a rejected or failed set leaves the object as it was: the host state is derived again, the device copy follows it
        h->P = old;
        derive(h);
        (void)upload_consts(h);
    }
    return rc;
}

int mi_orb_get_params(const mi_orb *h, mi_orb_params *p)
{
    MI_REQUIRE(h && p, MI_ERR_BAD_ARG, "null argument");
    *p = h->P;
    return MI_OK;
}

void mi_orb_destroy(mi_orb *h)
{
    delete h;
}

int mi_orb_scratch_bytes(const mi_orb *h, size_t *bytes)
{
    MI_REQUIRE(h && bytes, MI_ERR_BAD_ARG, "null argument");
    *bytes = h->scratch.n;
    return MI_OK;
}

int mi_orb_pattern_source(const mi_orb *h, int *source)
{
    MI_REQUIRE(h && source, MI_ERR_BAD_ARG, "null argument");
    *source = h->has_pool ? 1 : 0;
    return MI_OK;
}

int mi_orb_reach(const mi_orb *h, int *reach)
{
    MI_REQUIRE(h && reach, MI_ERR_BAD_ARG, "null argument");
    *reach = orb::orb_reach(h->P, h->pattern_reach, true);
    return MI_OK;
}

int mi_orb_make_pattern(int patch_size, int wta_k, const mi_mat *pattern0, mi_mat *out)
{
    MI_REQUIRE(patch_size >= 2, MI_ERR_BAD_ARG, "patchSize >= 2");
    MI_REQUIRE(wta_k == 2 || wta_k == 3 || wta_k == 4, MI_ERR_BAD_ARG, "WTA_K == 2 || WTA_K == 3 || WTA_K == 4");
    if (pattern0) MI_TRY(check_pool(pattern0));
    const int n = orb::orb_pattern_cols(wta_k);
    MI_REQUIRE(out && out->data, MI_ERR_BAD_ARG, "null out");
    MI_REQUIRE(out->type == MI_32SC1, MI_ERR_BAD_TYPE, "out.type() == CV_32SC1");
    MI_REQUIRE(out->rows == 2 && out->cols == n && out->step >= (size_t)n * 4, MI_ERR_BAD_SIZE, "out must be 2 x %d", n);
    int pool[2 * orb::ORB_NPOINTS], pat[2 * orb::ORB_NPOINTS];
    if (pattern0) read_pool(pattern0, pool);
    orb::orb_make_pattern(patch_size, wta_k, pattern0 ? pool : nullptr, pat);
    std::memcpy(row_of<int>(out, 0), pat, sizeof(int) * n);
    std::memcpy(row_of<int>(out, 1), pat + n, sizeof(int) * n);
    return MI_OK;
}

int mi_orb_features_per_level(const mi_orb_params *p, int *quota)
{
    MI_REQUIRE(p && quota, MI_ERR_BAD_ARG, "null argument");
    MI_TRY(orb::orb_fail(orb::orb_check_params(*p)));
    orb::orb_features_per_level(p->nfeatures, p->scale_factor, p->nlevels, quota);
    return MI_OK;
}

int mi_orb_u_max(int patch_size, int *u_max, int *n_u_max)
{
    MI_REQUIRE(u_max && n_u_max, MI_ERR_BAD_ARG, "null argument");
    MI_REQUIRE(patch_size >= 2 && patch_size / 2 + 2 < orb::ORB_UMAX_N, MI_ERR_BAD_ARG, "patchSize >= 2 && u_max.size() < 32");
    *n_u_max = orb::orb_u_max(patch_size, u_max);
    return MI_OK;
}

int mi_orb_detect_and_compute(mi_orb *h, const mi_mat *img, const mi_mat *mask, mi_mat *keypoints, mi_mat *descriptors, int *n, int use_provided,
                              void *stream)
{
    MI_REQUIRE(h && n, MI_ERR_BAD_ARG, "null argument");
    MI_TRY(check_u8(img, "image"));   // orb.cpp:666-667
    if (mask && mask->data) {
        MI_TRY(check_u8(mask, "mask"));
        MI_REQUIRE(mask->rows == img->rows && mask->cols == img->cols, MI_ERR_BAD_SIZE, "mask.size() == image.size()");
    }
    if (use_provided) return compute_provided(h, img, keypoints, descriptors, n, (hipStream_t)stream);
    *n = 0;
    return detect(h, img, mask, keypoints, descriptors, n, (hipStream_t)stream);
}

int mi_orb_pyramid_level(const mi_mat *src, const mi_mat *src_mask, int mask_mode, int edge_threshold, mi_mat *dst_img, mi_mat *dst_mask, void *stream)
{
    MI_TRY(check_u8(src, "src"));
    MI_TRY(check_u8(dst_img, "dst_img"));
    MI_REQUIRE(mask_mode >= 0 && mask_mode <= 2 && edge_threshold >= 0, MI_ERR_BAD_ARG, "mask_mode in 0 .. 2, edge_threshold >= 0");
    const bool masked = src_mask && src_mask->data;
    if (masked) {
        MI_TRY(check_u8(src_mask, "src_mask"));
        MI_REQUIRE(src_mask->rows == src->rows && src_mask->cols == src->cols, MI_ERR_BAD_SIZE, "src_mask.size() == src.size()");
        MI_REQUIRE(mask_mode != 0 || (src->rows == dst_img->rows && src->cols == dst_img->cols), MI_ERR_BAD_SIZE, "a copied mask needs dst.size() == src.size()");
    }
    if (dst_mask) {
        MI_TRY(check_u8(dst_mask, "dst_mask"));
        MI_REQUIRE(dst_mask->rows == dst_img->rows && dst_mask->cols == dst_img->cols, MI_ERR_BAD_SIZE, "dst_mask.size() == dst_img.size()");
    }
    hipStream_t st = (hipStream_t)stream;
    const int rows = dst_img->rows, cols = dst_img->cols;
    const float fx = (float)(1.0 / ((double)cols / src->cols)), fy = (float)(1.0 / ((double)rows / src->rows));   // resize.cpp:82-83,105
    const orb::OrbLaunch k = {orb::ORB_K_LEVEL, 0, 0, (unsigned)((cols + 63) / 64), (unsigned)((rows + 3) / 4), orb::ORB_BLOCK};
    const orb::OrbPlaneSrc s = {(const unsigned char *)src->data, (long long)src->step, src->rows, src->cols};
    orb::OrbPlaneSrc m = {nullptr, 0, 0, 0};
    if (masked) m = {(const unsigned char *)src_mask->data, (long long)src_mask->step, src_mask->rows, src_mask->cols};
    MI_TRY(orb::level(k, s, m, mask_mode, fx, fy, edge_threshold, (unsigned char *)dst_img->data, (long long)dst_img->step,
                      dst_mask ? (unsigned char *)dst_mask->data : nullptr, dst_mask ? (long long)dst_mask->step : 0, rows, cols, st));
    MI_HIP_TRY(hipStreamSynchronize(st));
    return MI_OK;
}

int mi_orb_cull(const mi_mat *in, int count, int n_points, mi_mat *out, int *count_out, void *stream)
{
    MI_REQUIRE(count_out && count >= 0 && n_points >= 0 && n_points <= (1 << 29), MI_ERR_BAD_ARG, "count >= 0, 0 <= n_points, non-null count_out");
    *count_out = 0;
    if (count == 0) return MI_OK;
    const int kept = count <= n_points ? count : n_points;
    MI_TRY(check_kp(in, 2, count, "in"));
    if (kept) MI_TRY(check_kp(out, 2, kept, "out"));
    hipStream_t st = (hipStream_t)stream;
    Stage S;
    MI_TRY(S.init(st));
    MI_TRY(S.tmp.alloc(&S.lv.keys, (size_t)count));
    S.lv.loc[0] = row_of<int>(in, 0); S.lv.resp[0] = row_of<float>(in, 1);
    S.lv.loc[1] = S.lv.loc[0]; S.lv.resp[1] = S.lv.resp[0];
    S.lv.loc[2] = kept ? row_of<int>(out, 0) : S.lv.loc[0]; S.lv.resp[2] = kept ? row_of<float>(out, 1) : S.lv.resp[0];
    S.lv.quota = n_points;
    MI_TRY(S.upload(0, count, st));
    const unsigned gx = (unsigned)((count + orb::ORB_BLOCK - 1) / orb::ORB_BLOCK);
    int *hist = (int *)(S.head + S.off_hist);
    unsigned *state = (unsigned *)(S.head + S.off_state);
    for (int d = 0; d < orb::ORB_DIGITS; ++d) MI_TRY(orb::hist({orb::ORB_K_HIST, -1, d, gx, 1, orb::ORB_BLOCK}, S.dtab, hist, state, 1, st));
    MI_TRY(orb::rank({orb::ORB_K_RANK, -1, 0, gx, 1, orb::ORB_BLOCK}, S.dtab, hist, state, 1, st));
    MI_HIP_TRY(hipMemcpyAsync(count_out, S.lv.counts + 3, sizeof(int), hipMemcpyDeviceToHost, st));
    MI_HIP_TRY(hipStreamSynchronize(st));
    return MI_OK;
}

int mi_orb_harris(const mi_mat *img, mi_mat *keypoints, int n, void *stream)
{
    MI_TRY(check_u8(img, "image"));
    MI_TRY(check_kp(keypoints, 2, n, "keypoints"));
    if (n == 0) return MI_OK;
    hipStream_t st = (hipStream_t)stream;
    MI_TRY(check_locations(keypoints, n, img, orb::ORB_HARRIS_BLOCK / 2 + 1, st));
    Stage S;
    MI_TRY(S.init(st));
    S.image(img);
    S.lv.loc[1] = row_of<int>(keypoints, 0); S.lv.resp[1] = row_of<float>(keypoints, 1);
    MI_TRY(S.upload(1, n, st));
    MI_TRY(orb::harris({orb::ORB_K_HARRIS, -1, 0, per_kp(n), 1, orb::ORB_BLOCK}, S.dtab, 1, st));
    MI_HIP_TRY(hipStreamSynchronize(st));
    return MI_OK;
}

int mi_orb_angle(const mi_mat *img, mi_mat *keypoints, int n, int patch_size, mi_mat *m01, mi_mat *m10, void *stream)
{
    MI_TRY(check_u8(img, "image"));
    MI_TRY(check_kp(keypoints, 3, n, "keypoints"));
    MI_REQUIRE(patch_size >= 2 && patch_size / 2 + 2 < orb::ORB_UMAX_N, MI_ERR_BAD_ARG, "patchSize >= 2 && u_max.size() < 32");
    MI_REQUIRE(!m01 == !m10, MI_ERR_BAD_ARG, "m01 and m10: both or none");
    if (m01) {
        MI_TRY(check_kp(m01, 1, n, "m01"));
        MI_TRY(check_kp(m10, 1, n, "m10"));
    }
    if (n == 0) return MI_OK;
    hipStream_t st = (hipStream_t)stream;
    MI_TRY(check_locations(keypoints, n, img, patch_size / 2, st));
    Stage S;
    MI_TRY(S.init(st));
    int u_max[orb::ORB_UMAX_N], *d_umax;
    orb::orb_u_max(patch_size, u_max);
    MI_TRY(S.tmp.alloc(&d_umax, (size_t)orb::ORB_UMAX_N));
    MI_HIP_TRY(hipMemcpyAsync(d_umax, u_max, sizeof(u_max), hipMemcpyHostToDevice, st));
    S.image(img);
    S.lv.loc[2] = row_of<int>(keypoints, 0); S.lv.angle = row_of<float>(keypoints, 2);
    MI_TRY(S.upload(2, n, st));
    MI_TRY(orb::angle({orb::ORB_K_ANGLE, -1, 0, per_kp(n), 1, orb::ORB_BLOCK}, S.dtab, d_umax, patch_size / 2, m01 ? row_of<int>(m01, 0) : nullptr,
                      m10 ? row_of<int>(m10, 0) : nullptr, st));
    MI_HIP_TRY(hipStreamSynchronize(st));
    return MI_OK;
}

int mi_orb_blur(const mi_mat *src, mi_mat *dst, void *stream)
{
    MI_TRY(check_u8(src, "src"));
    MI_TRY(check_u8(dst, "dst"));
    MI_REQUIRE(dst->rows == src->rows && dst->cols == src->cols, MI_ERR_BAD_SIZE, "dst.size() == src.size()");
    MI_REQUIRE(dst->data != src->data, MI_ERR_BAD_ARG, "blur is not in place");
    hipStream_t st = (hipStream_t)stream;
    const orb::OrbLaunch k = {orb::ORB_K_BLUR, 0, 0, (unsigned)((src->cols + orb::ORB_BLUR_TILE - 1) / orb::ORB_BLUR_TILE),
                              (unsigned)((src->rows + orb::ORB_BLUR_TILE - 1) / orb::ORB_BLUR_TILE), orb::ORB_BLOCK};
    MI_TRY(orb::blur(k, (const unsigned char *)src->data, (long long)src->step, (unsigned char *)dst->data, (long long)dst->step, src->rows, src->cols,
                     gaussian_taps(), st));
    MI_HIP_TRY(hipStreamSynchronize(st));
    return MI_OK;
}

int mi_orb_descriptors(const mi_mat *img, const mi_mat *keypoints, int n, const mi_mat *pattern, int wta_k, mi_mat *descriptors, void *stream)
{
    MI_TRY(check_u8(img, "image"));
    MI_TRY(check_kp(keypoints, 3, n, "keypoints"));
    MI_REQUIRE(wta_k == 2 || wta_k == 3 || wta_k == 4, MI_ERR_BAD_ARG, "WTA_K == 2 || WTA_K == 3 || WTA_K == 4");
    const int pc = orb::orb_pattern_cols(wta_k);
    MI_REQUIRE(pattern && pattern->data, MI_ERR_BAD_ARG, "pattern: null");
    MI_REQUIRE(pattern->type == MI_32SC1, MI_ERR_BAD_TYPE, "pattern.type() == CV_32SC1");
    MI_REQUIRE(pattern->rows == 2 && pattern->cols == pc && pattern->step >= (size_t)pc * 4, MI_ERR_BAD_SIZE, "pattern must be 2 x %d", pc);
    if (n == 0) return MI_OK;
    MI_REQUIRE(descriptors && descriptors->data, MI_ERR_BAD_ARG, "descriptors: null");
    MI_REQUIRE(descriptors->type == MI_8UC1, MI_ERR_BAD_TYPE, "descriptors.type() == CV_8UC1");
    MI_REQUIRE(descriptors->rows >= n && descriptors->cols >= orb::ORB_DESC_BYTES && descriptors->step >= (size_t)descriptors->cols, MI_ERR_BAD_SIZE,
               "descriptors must be (at least n) x 32");
    hipStream_t st = (hipStream_t)stream;
    int pat[2 * orb::ORB_NPOINTS];
    std::memcpy(pat, row_of<int>(pattern, 0), sizeof(int) * pc);
    std::memcpy(pat + pc, row_of<int>(pattern, 1), sizeof(int) * pc);
    MI_TRY(check_locations(keypoints, n, img, orb::orb_pattern_reach(pat, pc), st));
    Stage S;
    MI_TRY(S.init(st));
    int *d_pat;
    MI_TRY(S.tmp.alloc(&d_pat, (size_t)2 * pc));
    MI_HIP_TRY(hipMemcpyAsync(d_pat, pat, sizeof(int) * 2 * pc, hipMemcpyHostToDevice, st));
    S.image(img);
    S.lv.loc[2] = row_of<int>(keypoints, 0); S.lv.angle = row_of<float>(keypoints, 2);
    MI_TRY(S.upload(2, n, st));
    MI_TRY(orb::descriptors({orb::ORB_K_DESC, -1, 0, per_kp(n), 1, orb::ORB_BLOCK}, S.dtab, d_pat, pc, wta_k, (unsigned char *)descriptors->data,
                            (long long)descriptors->step, descriptors->rows, st));
    MI_HIP_TRY(hipStreamSynchronize(st));
    return MI_OK;
}

}  // extern "C"
