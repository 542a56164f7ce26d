// cv::cuda::DescriptorMatcher (brute force): handle + C-ABI entry points.  Every entry point describes its call, builds the plan
// (bf_plan.h: validation of both descriptor families, kernel shape, splits, scratch size, launch list) and runs the plan's launches in
// order on the caller's stream.
#include "bf_dispatch.h"
#include <cstdlib>

using namespace mi;

struct mi_bfmatcher {
    int norm = MI_NORM_L2;
    DevBuf<unsigned char> part;   // knn: [segment][query][K] {distance, index}; radius: [segment][query] count -> offset
};

namespace {

// MIFLOW_BF_W, read on every call (tests and sweeps switch it inside one process): 1 = the single-wave shapes of kBfRows
int w_knob() { const char *e = getenv("MIFLOW_BF_W"); return e && atoi(e) == 1 ? 1 : 4; }

bfint::Desc desc_of(const mi_mat &m) { return bfint::Desc{m.data, (long long)m.step, m.rows, m.cols, m.type}; }      // single channel: type == depth
bfint::Mask mask_of(const mi_mat *masks, int m)
{
    return masks && masks[m].data ? bfint::Mask{(const unsigned char *)masks[m].data, (long long)masks[m].step} : bfint::Mask{nullptr, 0};
}

int run(mi_bfmatcher *h, int kind, const mi_mat *query, const mi_mat *trains, const mi_mat *masks, int n_trains, int k, float max_distance,
        mi_mat *train_idx, mi_mat *img_idx, mi_mat *distance, mi_mat *n_matches, void *stream)
{
    hipStream_t st = (hipStream_t)stream;
    const bf::BfCall c = {kind, h != nullptr, h ? h->norm : 0, query, trains, masks, n_trains, k, train_idx, img_idx, distance, n_matches};
    const bf::BfPlan p = bf::bf_make_plan(c, w_knob());
    MI_REQUIRE(p.err.code == MI_OK, p.err.code, "%s", p.err.msg);
    // the n_q x cols outputs as base pointers and per-query element strides; the fixed shapes pack a query's k entries into one element
    const bool packed = kind == bf::BF_CALL_MATCH || kind == bf::BF_CALL_KNN2;
    const auto stride = [&](const mi_mat *m) { return !m ? 0 : packed ? (long long)p.k : (long long)(m->step / 4); };
    const bfint::Lists o = {(int *)train_idx->data, stride(train_idx), img_idx ? (int *)img_idx->data : nullptr, stride(img_idx),
                         (float *)distance->data, stride(distance)};
    int *nm = n_matches ? (int *)n_matches->data : nullptr;
    MI_TRY(h->part.ensure(p.part_bytes));
    // Float family: ONE argument struct per call.  A pass overwrites its train set's fields, write and, from the first continuation pass
    // on, lo_* (col0 only grows along the list, so lo_* is never stale); merge, scan and assign image read q / nq / part / cnt only, so what
    // the last pass left in the other fields does not matter to them.  part and cnt name the one scratch buffer of both call kinds.
    bf::Args A = {};
    A.q = (const float *)query->data; A.qstep = query->step; A.nq = p.nq; A.d = p.d;
    A.part = reinterpret_cast<float2 *>(h->part.p); A.cnt = reinterpret_cast<int *>(h->part.p);
    if (!p.k) {
        A.max_dist = max_distance; A.cols = p.cols;
        A.r_idx = o.idx; A.r_istep = (size_t)o.istep; A.r_img = o.img; A.r_mstep = (size_t)o.mstep; A.r_dist = o.dist; A.r_dstep = (size_t)o.dstep;
    }
    for (const bf::BfLaunch &l : p.launches) {
        switch (l.op) {
        case bf::BF_OP_INT_KNN: case bf::BF_OP_INT_RADIUS:
            bfint::launch(l, desc_of(*query), desc_of(trains[l.m]), mask_of(masks, l.m), p.norm, p.k, max_distance, p.cols, o, nm, st);
            continue;
        case bf::BF_OP_KNN_PASS: case bf::BF_OP_RADIUS_COUNT: case bf::BF_OP_RADIUS_WRITE: {
            const mi_mat &t = trains[l.m];
            const bfint::Mask mk = mask_of(masks, l.m);
            const bf::BfSeg &s = p.segs[l.m];
            A.t = (const float *)t.data; A.tstep = t.step; A.nt = t.rows; A.mask = mk.p; A.mstep = (size_t)mk.step;
            A.rows_per_split = s.rows_per_split; A.t_base = s.t_base; A.seg0 = s.seg0;
            A.write = l.op == bf::BF_OP_RADIUS_WRITE;
            if (l.col0) { A.lo_idx = o.idx + l.col0 - 1; A.lo_istep = (size_t)o.istep; A.lo_dist = o.dist + l.col0 - 1; A.lo_dstep = (size_t)o.dstep; }
            break;
        }
        }
        bf::launch(p, l, A, o, nm, st);
    }
    MI_HIP_TRY(hipGetLastError());
    return MI_OK;
}

}  // namespace

extern "C" {

int mi_bf_create(int norm_type, mi_bfmatcher **out)
{
    MI_REQUIRE(out, MI_ERR_BAD_ARG, "null out");
    *out = nullptr;
    MI_REQUIRE(bf::bf_type_norm_ok(MI_32FC1, norm_type) || bf::bf_type_norm_ok(MI_8UC1, norm_type), MI_ERR_BAD_ARG,   // a column of the table
               "norm == NORM_L1 || norm == NORM_L2 || norm == NORM_HAMMING");   // BFMatcher_Impl constructor
    MI_TRY(require_device());
    *out = new mi_bfmatcher();
    (*out)->norm = norm_type;
    return MI_OK;
}

void mi_bf_destroy(mi_bfmatcher *h)
{
    delete h;
}

int mi_bf_match(mi_bfmatcher *h, const mi_mat *query, const mi_mat *train, const mi_mat *mask, mi_mat *train_idx, mi_mat *distance, void *stream)
{
    return run(h, bf::BF_CALL_MATCH, query, train, mask, 1, 1, 0.f, train_idx, nullptr, distance, nullptr, stream);
}

int mi_bf_knn_match2(mi_bfmatcher *h, const mi_mat *query, const mi_mat *train, const mi_mat *mask, mi_mat *train_idx, mi_mat *distance,
                     void *stream)
{
    return run(h, bf::BF_CALL_KNN2, query, train, mask, 1, 2, 0.f, train_idx, nullptr, distance, nullptr, stream);
}

int mi_bf_knn_match(mi_bfmatcher *h, const mi_mat *query, const mi_mat *trains, const mi_mat *masks, int n_trains, int k, mi_mat *train_idx,
                    mi_mat *img_idx, mi_mat *distance, void *stream)
{
    return run(h, bf::BF_CALL_KNN, query, trains, masks, n_trains, k, 0.f, train_idx, img_idx, distance, nullptr, stream);
}

int mi_bf_radius_match(mi_bfmatcher *h, const mi_mat *query, const mi_mat *trains, const mi_mat *masks, int n_trains, float max_distance,
                       mi_mat *train_idx, mi_mat *img_idx, mi_mat *distance, mi_mat *n_matches, void *stream)
{
    return run(h, bf::BF_CALL_RADIUS, query, trains, masks, n_trains, 0, max_distance, train_idx, img_idx, distance, n_matches, stream);
}

}  // extern "C"
