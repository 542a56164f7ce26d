// The PLAN of the brute-force matcher (bfmatch_kernels.hip: float descriptors; bfint_kernels.hip: integer descriptors): ONE validator
// for both families and the four entry points, the table of kernel shapes, the train splits, the scratch size and the ordered launch
// list.  bf_api.cpp only EXECUTES the list.  Pure arithmetic, no HIP types: of a matrix it reads type, rows, cols and data == NULL.
// tests/cpp/bf_plan_test.cpp holds it to the expressions it replaced.
#pragma once
#include <algorithm>
#include <climits>
#include <cstddef>
#include <vector>
#include "miflow/c_api.h"
#include "bf_shared.h"   // the integer family's limits (MAX_D, MAX_K), its workgroup (T) and Lists

namespace mi {
namespace bf {

// ---- the shapes a build contains: matchDispatcher (bf_match.cu:563-570) by descriptor length; long descriptors trade tile height for
// the query area.  Four waves per workgroup measured 2.8-3.5 x faster than one (profiles/r01y: 12 564^2 pairs, D = 64: 0.69 vs
// 1.95 ms); MIFLOW_BF_W=1 keeps the single-wave shape reachable (column W1).  The kernel file instantiates k_knn<D, TT, W | W1> and
// k_radius<D, TT> (one wave) of exactly these rows, the plan picks among them.
struct BfRow { int D, TT, W, W1; };   // descriptor class, tile height, waves of k_knn, waves under MIFLOW_BF_W=1
inline constexpr BfRow kBfRows[] = {{64, 32, 4, 1}, {128, 32, 4, 1}, {256, 16, 4, 4}, {512, 8, 2, 2}};
constexpr int kBfRowCount = (int)(sizeof(kBfRows) / sizeof(kBfRows[0]));
constexpr int bf_row_of(int d, int i = 0) { return i + 1 == kBfRowCount || d <= kBfRows[i].D ? i : bf_row_of(d, i + 1); }
constexpr int bf_list_len(int k) { return k <= 2 ? 2 : 8; }   // K: the per-lane list of k_knn / k_merge; k > K runs further passes

// ---- the reference's (depth, norm) table, brute_force_matcher.cpp:336-356 (single channel: type == depth)
inline bool bf_type_norm_ok(int type, int norm)
{
    const bool hamming_row = type == MI_8UC1 || type == MI_16UC1 || type == MI_32SC1;
    if (norm == MI_NORM_L1) return hamming_row || type == MI_16SC1 || type == MI_32FC1;
    return norm == MI_NORM_L2 ? type == MI_32FC1 : norm == MI_NORM_HAMMING && hamming_row;
}

enum BfCallKind { BF_CALL_MATCH = 0, BF_CALL_KNN2, BF_CALL_KNN, BF_CALL_RADIUS };   // mi_bf_match, _knn_match2 (fixed shapes), _knn_match, _radius_match
// handle: the caller's handle is not NULL, norm: its norm; k: BF_CALL_KNN only (the fixed shapes are k = 1 and k = 2)
struct BfCall {
    int kind; bool handle; int norm;
    const mi_mat *query, *trains, *masks; int n_trains, k;
    const mi_mat *train_idx, *img_idx, *distance, *n_matches;
};

// BF_OP_KNN_PASS      k_knn           lists of one train set's splits; col0 > 0: only candidates after column col0 - 1
// BF_OP_MERGE         k_merge         the segment lists -> columns [col0, col0 + ncol)
// BF_OP_ASSIGN_IMAGE  k_assign_image  collection index -> (image m, train index)
// BF_OP_RADIUS_COUNT / _SCAN / _WRITE k_radius with write = 0, k_radius_scan (counts -> first output slots, n_matches), k_radius with write = 1
// BF_OP_INT_KNN / _INT_RADIUS         bfint::k_knn / k_radius: continue the lists in the output matrices; first = (m == 0)
enum BfOp { BF_OP_KNN_PASS = 0, BF_OP_MERGE, BF_OP_ASSIGN_IMAGE, BF_OP_RADIUS_COUNT, BF_OP_RADIUS_SCAN, BF_OP_RADIUS_WRITE, BF_OP_INT_KNN, BF_OP_INT_RADIUS };

struct BfErr { int code; const char *msg; };
struct BfSeg { int nsplit, rows_per_split, seg0, t_base; };   // seg0: first split, t_base: first row of the train set in the collection
struct BfLaunch { int op, m, gx, gy, block, col0, ncol; };   // m: the train set (-1: none)
// What the launchers need of the call travels with the plan (they do not see the BfCall).
struct BfPlan {
    BfErr err;                   // the validator's verdict; nothing below is set when it rejects
    bool flt;                    // float family (CV_32F) or integer family
    int norm, nq, d, n_trains, k, cols;   // cols: columns of the outputs = k of a k-nearest call (k = 0: radius match)
    int K, row, tt, w, nseg;     // float family: list length (0: radius), row of kBfRows, its tile height, waves per workgroup; splits
    size_t part_bytes;           // knn: [segment][query][K] {distance, index}; radius: [segment][query] count -> offset
    std::vector<BfSeg> segs;
    std::vector<BfLaunch> launches;
};

inline int bf_div_up(long long a, int b) { return (int)((a + b - 1) / b); }

inline bool bf_is_rows(const mi_mat *m, int type, int rows, int cols) { return m && m->data && m->type == type && m->rows == rows && m->cols == cols; }

#define BF_REQUIRE(cond, code, text) do { if (!(cond)) return BfErr{(code), (text)}; } while (0)

// Every requirement of the four entry points, in the order the calls have always tested them: an input with one fault keeps its code
// and text, and where two coincide the same one wins.  The two families differ in where the table and img_idx stand.
inline BfErr bf_validate(const BfCall &c)
{
    const mi_mat *q = c.query, *ti = c.train_idx, *im = c.img_idx, *di = c.distance;
    const bool radius = c.kind == BF_CALL_RADIUS, two = c.kind == BF_CALL_KNN2, collection_ok = c.n_trains == 1 || im;
    const int k = c.kind == BF_CALL_KNN ? c.k : two ? 2 : 1, cols = radius && ti ? ti->cols : 0;
    if (c.kind == BF_CALL_MATCH || two) {
        const int ity = two ? MI_32SC2 : MI_32SC1, dty = two ? MI_32FC2 : MI_32FC1;
        BF_REQUIRE(q && c.trains, MI_ERR_BAD_ARG, "null argument");
        BF_REQUIRE(ti && di && ti->data && di->data, MI_ERR_BAD_ARG, "null argument");
        BF_REQUIRE(ti->type == ity && di->type == dty, MI_ERR_BAD_TYPE,
                   two ? "k = 2: train_idx CV_32SC2 / distance CV_32FC2" : "train_idx CV_32SC1 / distance CV_32FC1");
        BF_REQUIRE(bf_is_rows(ti, ity, 1, q->rows) && bf_is_rows(di, dty, 1, q->rows), MI_ERR_BAD_SIZE, "outputs must be 1 x query.rows");
    } else if (!radius) {
        BF_REQUIRE(q && c.trains && ti && di, MI_ERR_BAD_ARG, "null argument");
        BF_REQUIRE(k >= 1, MI_ERR_BAD_ARG, "k >= 1");
        BF_REQUIRE(bf_is_rows(ti, MI_32SC1, q->rows, k) && bf_is_rows(di, MI_32FC1, q->rows, k) && (!im || bf_is_rows(im, MI_32SC1, q->rows, k)),
                   MI_ERR_BAD_SIZE, "train_idx / img_idx CV_32SC1 and distance CV_32FC1 must be query.rows x k");
    } else {
        BF_REQUIRE(c.handle && q && c.trains && ti && di && c.n_matches, MI_ERR_BAD_ARG, "null argument");
        BF_REQUIRE(collection_ok, MI_ERR_BAD_ARG, "a collection needs img_idx");
        BF_REQUIRE(cols > 0 && bf_is_rows(ti, MI_32SC1, q->rows, cols) && bf_is_rows(di, MI_32FC1, q->rows, cols) &&
                       (!im || bf_is_rows(im, MI_32SC1, q->rows, cols)) && bf_is_rows(c.n_matches, MI_32SC1, 1, q->rows),
                   MI_ERR_BAD_SIZE, "train_idx / img_idx CV_32SC1, distance CV_32FC1: query.rows x cols; n_matches CV_32SC1 1 x query.rows");
    }
    BF_REQUIRE(c.handle, MI_ERR_BAD_ARG, "null handle");
    const bool flt = q->type == MI_32FC1;
    const bool table_ok = bf_type_norm_ok(q->type, c.norm);
    if (flt) {
        BF_REQUIRE(table_ok, MI_ERR_BAD_TYPE, "unsupported combination of query.depth() and norm");
        BF_REQUIRE(collection_ok, MI_ERR_BAD_ARG, "a collection needs img_idx");
    }
    BF_REQUIRE(q->data && c.n_trains > 0, MI_ERR_BAD_ARG, "null argument");
    BF_REQUIRE(table_ok, MI_ERR_BAD_TYPE, "unsupported combination of query.depth() and norm");
    BF_REQUIRE(q->rows > 0 && q->cols > 0, MI_ERR_BAD_SIZE, "empty query");
    BF_REQUIRE(q->cols <= (flt ? kBfRows[kBfRowCount - 1].D : bfint::MAX_D), MI_ERR_BAD_SIZE,
               flt ? "descriptor length <= 512; longer descriptors are not built" : "integer descriptors of up to 128 elements; longer ones are not built");
    long long total = 0;
    for (int m = 0; m < c.n_trains; ++m) {
        const mi_mat &t = c.trains[m];
        BF_REQUIRE(t.data && t.type == q->type, MI_ERR_BAD_TYPE, flt ? "descriptors must be CV_32FC1" : "train.type() == query.type()");
        BF_REQUIRE(t.rows > 0 && t.cols == q->cols, MI_ERR_BAD_SIZE, "query.cols == train.cols, non-empty");
        if (c.masks && c.masks[m].data)
            BF_REQUIRE(c.masks[m].type == MI_8UC1 && c.masks[m].rows == q->rows && c.masks[m].cols == t.rows, MI_ERR_BAD_SIZE,
                       "mask must be CV_8UC1, query.rows x train.rows");
        total += t.rows;   // float family: the lists hold indices into the concatenated collection
        BF_REQUIRE(!flt || total < INT_MAX, MI_ERR_BAD_SIZE, "train collection too large");
    }
    if (!flt) {
        BF_REQUIRE(radius || k <= bfint::MAX_K, MI_ERR_NOT_IMPL, "integer descriptors: 1 <= k <= 16");
        BF_REQUIRE(collection_ok, MI_ERR_BAD_ARG, "a collection needs img_idx");
    }
    // k_assign_image indexes the n_q x cols outputs with an int (the integer family and a call without img_idx index in 64 bits)
    BF_REQUIRE(!(flt && im) || (long long)q->rows * (radius ? cols : k) <= INT_MAX, MI_ERR_BAD_SIZE,
               "query.rows x output columns must fit 32 bits");
    return BfErr{MI_OK, nullptr};
}
#undef BF_REQUIRE

// w_knob: MIFLOW_BF_W (4: the table's W, 1: its W1)
inline BfPlan bf_make_plan(const BfCall &c, int w_knob)
{
    BfPlan p = {};
    if ((p.err = bf_validate(c)).code) return p;
    const bool radius = c.kind == BF_CALL_RADIUS, have_img = c.img_idx != nullptr;
    p.flt = c.query->type == MI_32FC1;
    p.norm = c.norm; p.nq = c.query->rows; p.d = c.query->cols; p.n_trains = c.n_trains;
    p.k = radius ? 0 : c.kind == BF_CALL_KNN ? c.k : c.kind == BF_CALL_KNN2 ? 2 : 1;
    p.cols = radius ? c.train_idx->cols : p.k;
    if (!p.flt) {   // one launch per train set, no scratch: the lists live in the output matrices
        for (int m = 0; m < p.n_trains; ++m)
            p.launches.push_back({radius ? BF_OP_INT_RADIUS : BF_OP_INT_KNN, m, bf_div_up(p.nq, bfint::T), 1, bfint::T, 0, p.cols});
        return p;
    }
    p.K = radius ? 0 : bf_list_len(p.k); p.row = bf_row_of(p.d);
    p.tt = kBfRows[p.row].TT; p.w = radius ? 1 : w_knob == 1 ? kBfRows[p.row].W1 : kBfRows[p.row].W;
    // the splits: enough workgroups for 256 CUs, multiples of the LDS tile
    const int qblocks = bf_div_up(p.nq, 64);
    p.segs.resize(p.n_trains);
    for (int m = 0, t_base = 0; m < p.n_trains; t_base += c.trains[m++].rows) {
        const int nt = c.trains[m].rows, nsplit = std::min(std::max(1, 2048 / qblocks), bf_div_up(nt, p.tt));
        const int rps = bf_div_up(bf_div_up(nt, nsplit), p.tt) * p.tt;
        p.segs[m] = BfSeg{bf_div_up(nt, rps), rps, p.nseg, t_base};
        p.nseg += p.segs[m].nsplit;
    }
    p.part_bytes = (radius ? sizeof(int) : 2 * sizeof(float) * p.K) * (size_t)p.nseg * p.nq;
    const auto per_set = [&](int op, int block, int col0, int ncol) {
        for (int m = 0; m < p.n_trains; ++m) p.launches.push_back({op, m, qblocks, p.segs[m].nsplit, block, col0, ncol});
    };
    if (radius) {
        per_set(BF_OP_RADIUS_COUNT, 64, 0, p.cols);
        p.launches.push_back({BF_OP_RADIUS_SCAN, -1, bf_div_up(p.nq, 256), 1, 256, 0, p.cols});
        per_set(BF_OP_RADIUS_WRITE, 64, 0, p.cols);
    } else for (int col0 = 0; col0 < p.k; col0 += p.K) {
        const int ncol = std::min(p.K, p.k - col0);
        per_set(BF_OP_KNN_PASS, 64 * p.w, col0, ncol);
        p.launches.push_back({BF_OP_MERGE, -1, bf_div_up(p.nq, 256), 1, 256, col0, ncol});
    }
    // an unresolved entry >= t_base of image m belongs to image m: descending
    for (int m = have_img ? p.n_trains - 1 : -1; m >= 0; --m)
        p.launches.push_back({BF_OP_ASSIGN_IMAGE, m, bf_div_up((long long)p.nq * p.cols, 256), 1, 256, 0, p.cols});
    return p;
}

}  // namespace bf
}  // namespace mi
