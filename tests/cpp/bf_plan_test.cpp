// The plan of the brute-force matcher (csrc/bf_plan.h) on the host, against the rules it replaced, restated here in the form they had:
// knn_shape / radius_shape, the split arithmetic, the two scratch formulas and the call sequences of run_knn / mi_bf_radius_match /
// bfint::knn / bfint::radius, and the validation of the four entry points with bf::plan and bfint::check in their order, codes and
// texts.  Plain C++, no device.
#include <climits>
#include <cstdio>
#include <cstring>
#include <vector>
#include "bf_plan.h"

using namespace mi::bf;

static int fails = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); ++fails; } } while (0)

static char g_byte;   // the plan reads `data == NULL` only
static mi_mat mat(int rows, int cols, int type) { return mi_mat{&g_byte, 0, rows, cols, type}; }

// ---------------------------------------------------------------------------------------------------- the old rules
struct OldShape { int D, tt, w; };
static OldShape old_knn_shape(int d, int w_small)
{
    if (d <= 64) return w_small == 4 ? OldShape{64, 32, 4} : OldShape{64, 32, 1};
    if (d <= 128) return w_small == 4 ? OldShape{128, 32, 4} : OldShape{128, 32, 1};
    if (d <= 256) return OldShape{256, 16, 4};
    return OldShape{512, 8, 2};
}
static OldShape old_radius_shape(int d)
{
    if (d <= 64) return OldShape{64, 32, 1};
    if (d <= 128) return OldShape{128, 32, 1};
    if (d <= 256) return OldShape{256, 16, 1};
    return OldShape{512, 8, 1};
}
static int div_up(int a, int b) { return (a + b - 1) / b; }
static int align_up(int a, int b) { return div_up(a, b) * b; }
static int imin(int a, int b) { return a < b ? a : b; }
static int imax(int a, int b) { return a > b ? a : b; }

#define OLD_REQUIRE(cond, code, text) do { if (!(cond)) return BfErr{(code), (text)}; } while (0)
static bool old_is_rows(const mi_mat *m, int type, int rows, int cols) { return m && m->data && m->type == type && m->rows == rows && m->cols == cols; }

// bf::plan: validation and splits in one loop
static BfErr old_plan(const mi_mat *query, const mi_mat *trains, const mi_mat *masks, int n_trains, int tt, std::vector<BfSeg> &segs, int *nseg)
{
    OLD_REQUIRE(query && trains && query->data && n_trains > 0, MI_ERR_BAD_ARG, "null argument");
    OLD_REQUIRE(query->type == MI_32FC1, MI_ERR_BAD_TYPE, "descriptors must be CV_32FC1");
    OLD_REQUIRE(query->rows > 0 && query->cols > 0, MI_ERR_BAD_SIZE, "empty query");
    OLD_REQUIRE(query->cols <= 512, MI_ERR_BAD_SIZE, "descriptor length <= 512; longer descriptors are not built");
    const int qblocks = div_up(query->rows, 64);
    long long total = 0;
    int s0 = 0;
    segs.resize(n_trains);
    for (int m = 0; m < n_trains; ++m) {
        const mi_mat &t = trains[m];
        OLD_REQUIRE(t.data && t.type == MI_32FC1, MI_ERR_BAD_TYPE, "descriptors must be CV_32FC1");
        OLD_REQUIRE(t.rows > 0 && t.cols == query->cols, MI_ERR_BAD_SIZE, "query.cols == train.cols, non-empty");
        if (masks && masks[m].data)
            OLD_REQUIRE(masks[m].type == MI_8UC1 && masks[m].rows == query->rows && masks[m].cols == t.rows, MI_ERR_BAD_SIZE,
                        "mask must be CV_8UC1, query.rows x train.rows");
        int nsplit = imin(imax(1, 2048 / qblocks), div_up(t.rows, tt));
        const int rps = align_up(div_up(t.rows, nsplit), tt);
        nsplit = div_up(t.rows, rps);
        segs[m] = BfSeg{nsplit, rps, s0, (int)total};
        s0 += nsplit;
        total += t.rows;
        OLD_REQUIRE(total < INT_MAX, MI_ERR_BAD_SIZE, "train collection too large");
    }
    *nseg = s0;
    return BfErr{MI_OK, nullptr};
}

// bfint::check
static BfErr old_int_check(int norm, const mi_mat *query, const mi_mat *trains, const mi_mat *masks, int n_trains)
{
    OLD_REQUIRE(query && trains && query->data && n_trains > 0, MI_ERR_BAD_ARG, "null argument");
    const int ty = query->type;
    const bool ok = (norm == 2 && (ty == MI_8UC1 || ty == MI_16UC1 || ty == MI_16SC1 || ty == MI_32SC1)) ||
                    (norm == 6 && (ty == MI_8UC1 || ty == MI_16UC1 || ty == MI_32SC1));
    OLD_REQUIRE(ok, MI_ERR_BAD_TYPE, "unsupported combination of query.depth() and norm");
    OLD_REQUIRE(query->rows > 0 && query->cols > 0, MI_ERR_BAD_SIZE, "empty query");
    OLD_REQUIRE(query->cols <= 128, MI_ERR_BAD_SIZE, "integer descriptors of up to 128 elements; longer ones are not built");
    for (int m = 0; m < n_trains; ++m) {
        OLD_REQUIRE(trains[m].data && trains[m].type == ty, MI_ERR_BAD_TYPE, "train.type() == query.type()");
        OLD_REQUIRE(trains[m].rows > 0 && trains[m].cols == query->cols, MI_ERR_BAD_SIZE, "query.cols == train.cols, non-empty");
        if (masks && masks[m].data)
            OLD_REQUIRE(masks[m].type == MI_8UC1 && masks[m].rows == query->rows && masks[m].cols == trains[m].rows, MI_ERR_BAD_SIZE,
                        "mask must be CV_8UC1, query.rows x train.rows");
    }
    return BfErr{MI_OK, nullptr};
}

// what a call did: its verdict and, where it ran, its shape, splits, scratch and launches
struct Old {
    BfErr err;
    OldShape sh;
    int K, nseg;
    size_t part_bytes;
    std::vector<BfSeg> segs;
    std::vector<BfLaunch> launches;
};

static void old_assign_images(Old &o, int nq, int ncols)
{
    const int blocks = div_up(nq * ncols, 256);
    for (int m = (int)o.segs.size() - 1; m >= 0; --m) o.launches.push_back({BF_OP_ASSIGN_IMAGE, m, blocks, 1, 256, 0, ncols});
}

// run_knn behind mi_bf_match / mi_bf_knn_match2 / mi_bf_knn_match
static BfErr old_run_knn(Old &o, bool handle, int norm, const mi_mat *query, const mi_mat *trains, const mi_mat *masks, int n_trains, int k, bool img,
                         int w_small)
{
    OLD_REQUIRE(handle, MI_ERR_BAD_ARG, "null handle");
    OLD_REQUIRE(k >= 1, MI_ERR_BAD_ARG, "k >= 1");
    if (query && query->type != MI_32FC1) {   // bfint::knn
        const BfErr e = old_int_check(norm, query, trains, masks, n_trains);
        if (e.code) return e;
        OLD_REQUIRE(k >= 1 && k <= 16, MI_ERR_NOT_IMPL, "integer descriptors: 1 <= k <= 16");
        OLD_REQUIRE(n_trains == 1 || img, MI_ERR_BAD_ARG, "a collection needs img_idx");
        for (int m = 0; m < n_trains; ++m) o.launches.push_back({BF_OP_INT_KNN, m, div_up(query->rows, 64), 1, 64, 0, k});
        return BfErr{MI_OK, nullptr};
    }
    OLD_REQUIRE(norm == MI_NORM_L1 || norm == MI_NORM_L2, MI_ERR_BAD_TYPE, "unsupported combination of query.depth() and norm");
    OLD_REQUIRE(n_trains == 1 || img, MI_ERR_BAD_ARG, "a collection needs img_idx");
    const int K = k <= 2 ? 2 : 8;
    o.K = K;
    o.sh = old_knn_shape(query ? query->cols : 0, w_small);
    const BfErr e = old_plan(query, trains, masks, n_trains, o.sh.tt, o.segs, &o.nseg);
    if (e.code) return e;
    const int nq = query->rows;
    o.part_bytes = 8 * (size_t)o.nseg * nq * K;
    const int qblocks = div_up(nq, 64), mblocks = div_up(nq, 256);
    for (int col0 = 0; col0 < k; col0 += K) {
        const int ncol = imin(K, k - col0);
        for (int m = 0; m < n_trains; ++m) o.launches.push_back({BF_OP_KNN_PASS, m, qblocks, o.segs[m].nsplit, 64 * o.sh.w, col0, ncol});
        o.launches.push_back({BF_OP_MERGE, -1, mblocks, 1, 256, col0, ncol});
    }
    if (img) old_assign_images(o, nq, k);
    return BfErr{MI_OK, nullptr};
}

static Old old_call(const BfCall &c, int w_small)
{
    Old o = {};
    const mi_mat *query = c.query, *train_idx = c.train_idx, *distance = c.distance, *img_idx = c.img_idx, *n_matches = c.n_matches;
    o.err = [&]() -> BfErr {
        switch (c.kind) {
        case BF_CALL_MATCH:
            OLD_REQUIRE(query && c.trains, MI_ERR_BAD_ARG, "null argument");
            OLD_REQUIRE(train_idx && distance && train_idx->data && distance->data, MI_ERR_BAD_ARG, "null argument");
            OLD_REQUIRE(train_idx->type == MI_32SC1 && distance->type == MI_32FC1, MI_ERR_BAD_TYPE, "train_idx CV_32SC1 / distance CV_32FC1");
            OLD_REQUIRE(old_is_rows(train_idx, MI_32SC1, 1, query->rows) && old_is_rows(distance, MI_32FC1, 1, query->rows), MI_ERR_BAD_SIZE,
                        "outputs must be 1 x query.rows");
            return old_run_knn(o, c.handle, c.norm, query, c.trains, c.masks, 1, 1, false, w_small);
        case BF_CALL_KNN2:
            OLD_REQUIRE(query && c.trains, MI_ERR_BAD_ARG, "null argument");
            OLD_REQUIRE(train_idx && distance && train_idx->data && distance->data, MI_ERR_BAD_ARG, "null argument");
            OLD_REQUIRE(train_idx->type == MI_32SC2 && distance->type == MI_32FC2, MI_ERR_BAD_TYPE, "k = 2: train_idx CV_32SC2 / distance CV_32FC2");
            OLD_REQUIRE(old_is_rows(train_idx, MI_32SC2, 1, query->rows) && old_is_rows(distance, MI_32FC2, 1, query->rows), MI_ERR_BAD_SIZE,
                        "outputs must be 1 x query.rows");
            return old_run_knn(o, c.handle, c.norm, query, c.trains, c.masks, 1, 2, false, w_small);
        case BF_CALL_KNN:
            OLD_REQUIRE(query && c.trains && train_idx && distance, MI_ERR_BAD_ARG, "null argument");
            OLD_REQUIRE(c.k >= 1, MI_ERR_BAD_ARG, "k >= 1");
            OLD_REQUIRE(old_is_rows(train_idx, MI_32SC1, query->rows, c.k) && old_is_rows(distance, MI_32FC1, query->rows, c.k) &&
                            (!img_idx || old_is_rows(img_idx, MI_32SC1, query->rows, c.k)),
                        MI_ERR_BAD_SIZE, "train_idx / img_idx CV_32SC1 and distance CV_32FC1 must be query.rows x k");
            return old_run_knn(o, c.handle, c.norm, query, c.trains, c.masks, c.n_trains, c.k, img_idx != nullptr, w_small);
        default: break;
        }
        OLD_REQUIRE(c.handle && query && c.trains && train_idx && distance && n_matches, MI_ERR_BAD_ARG, "null argument");
        OLD_REQUIRE(c.n_trains == 1 || img_idx, MI_ERR_BAD_ARG, "a collection needs img_idx");
        const int cols = train_idx->cols;
        OLD_REQUIRE(cols > 0 && old_is_rows(train_idx, MI_32SC1, query->rows, cols) && old_is_rows(distance, MI_32FC1, query->rows, cols) &&
                        (!img_idx || old_is_rows(img_idx, MI_32SC1, query->rows, cols)) && old_is_rows(n_matches, MI_32SC1, 1, query->rows),
                    MI_ERR_BAD_SIZE, "train_idx / img_idx CV_32SC1, distance CV_32FC1: query.rows x cols; n_matches CV_32SC1 1 x query.rows");
        if (query->type != MI_32FC1) {   // bfint::radius
            const BfErr e = old_int_check(c.norm, query, c.trains, c.masks, c.n_trains);
            if (e.code) return e;
            OLD_REQUIRE(c.n_trains == 1 || img_idx, MI_ERR_BAD_ARG, "a collection needs img_idx");
            for (int m = 0; m < c.n_trains; ++m) o.launches.push_back({BF_OP_INT_RADIUS, m, div_up(query->rows, 64), 1, 64, 0, cols});
            return BfErr{MI_OK, nullptr};
        }
        OLD_REQUIRE(c.norm == MI_NORM_L1 || c.norm == MI_NORM_L2, MI_ERR_BAD_TYPE, "unsupported combination of query.depth() and norm");
        o.sh = old_radius_shape(query->cols);
        const BfErr e = old_plan(query, c.trains, c.masks, c.n_trains, o.sh.tt, o.segs, &o.nseg);
        if (e.code) return e;
        const int nq = query->rows;
        o.part_bytes = 4 * (size_t)o.nseg * nq;
        const int qblocks = div_up(nq, 64);
        for (int pass = 0; pass < 2; ++pass) {
            for (int m = 0; m < c.n_trains; ++m)
                o.launches.push_back({pass ? BF_OP_RADIUS_WRITE : BF_OP_RADIUS_COUNT, m, qblocks, o.segs[m].nsplit, 64, 0, cols});
            if (pass == 0) o.launches.push_back({BF_OP_RADIUS_SCAN, -1, div_up(nq, 256), 1, 256, 0, cols});
        }
        if (img_idx) old_assign_images(o, nq, cols);
        return BfErr{MI_OK, nullptr};
    }();
    return o;
}

// ---------------------------------------------------------------------------------------------------- calls
struct Call {   // owns the matrices a BfCall points to
    mi_mat query, ti, im, di, nm;
    std::vector<mi_mat> trains, masks;
    BfCall c;
};

// a valid call: k > 0: k-nearest (kind KNN); k == 0: radius match with `cols` output columns
static void make_call(Call &C, int kind, int type, int norm, int nq, const std::vector<int> &nts, int d, int k, int cols, bool img, bool with_masks = false)
{
    C.query = mat(nq, d, type);
    C.trains.clear(); C.masks.clear();
    for (int nt : nts) {
        C.trains.push_back(mat(nt, d, type));
        if (with_masks) C.masks.push_back(mat(nq, nt, MI_8UC1));
    }
    const int oc = kind == BF_CALL_RADIUS ? cols : k;
    if (kind == BF_CALL_MATCH) { C.ti = mat(1, nq, MI_32SC1); C.di = mat(1, nq, MI_32FC1); }
    else if (kind == BF_CALL_KNN2) { C.ti = mat(1, nq, MI_32SC2); C.di = mat(1, nq, MI_32FC2); }
    else { C.ti = mat(nq, oc, MI_32SC1); C.di = mat(nq, oc, MI_32FC1); }
    C.im = mat(nq, oc, MI_32SC1);
    C.nm = mat(1, nq, MI_32SC1);
    C.c = BfCall{kind, true, norm, &C.query, C.trains.data(), with_masks ? C.masks.data() : nullptr, (int)nts.size(), kind == BF_CALL_KNN ? k : 0,
                 &C.ti, img ? &C.im : nullptr, &C.di, kind == BF_CALL_RADIUS ? &C.nm : nullptr};
}

static bool same(const BfLaunch &a, const BfLaunch &b)
{
    return a.op == b.op && a.m == b.m && a.gx == b.gx && a.gy == b.gy && a.block == b.block && a.col0 == b.col0 && a.ncol == b.ncol;
}
static bool same_err(const BfErr &a, const BfErr &b) { return a.code == b.code && (a.code == MI_OK || !strcmp(a.msg, b.msg)); }

// field by field against the old rules, then the invariants
static void check_plan(const Call &C, int knob)
{
    const BfCall &c = C.c;
    const BfPlan p = bf_make_plan(c, knob);
    const Old o = old_call(c, knob);
    CHECK(o.err.code == MI_OK && p.err.code == MI_OK);
    if (o.err.code || p.err.code) { printf("  old %d '%s', plan %d '%s'\n", o.err.code, o.err.code ? o.err.msg : "", p.err.code, p.err.code ? p.err.msg : ""); return; }
    const bool radius = c.kind == BF_CALL_RADIUS, flt = c.query->type == MI_32FC1;
    const int nq = c.query->rows, k = radius ? 0 : c.kind == BF_CALL_KNN ? c.k : c.kind == BF_CALL_KNN2 ? 2 : 1;
    CHECK(p.flt == flt && p.norm == c.norm && p.nq == nq && p.d == c.query->cols && p.n_trains == c.n_trains && p.k == k);
    CHECK(p.cols == (radius ? c.train_idx->cols : k));
    CHECK(p.launches.size() == o.launches.size());
    for (size_t i = 0; i < p.launches.size() && i < o.launches.size(); ++i) CHECK(same(p.launches[i], o.launches[i]));
    CHECK(p.part_bytes == o.part_bytes && p.nseg == o.nseg && p.segs.size() == o.segs.size());
    if (!flt) { CHECK(p.part_bytes == 0 && p.segs.empty() && (int)p.launches.size() == c.n_trains); return; }
    CHECK(p.K == o.K && p.row >= 0 && p.row < kBfRowCount && kBfRows[p.row].D == o.sh.D && p.tt == o.sh.tt && p.w == o.sh.w && kBfRows[p.row].TT == p.tt);
    CHECK(p.d <= kBfRows[p.row].D && (p.row == 0 || p.d > kBfRows[p.row - 1].D));
    int seg0 = 0;
    long long t_base = 0;
    for (int m = 0; m < c.n_trains && m < (int)p.segs.size(); ++m) {
        const BfSeg &s = p.segs[m], &r = o.segs[m];
        const int nt = c.trains[m].rows;
        CHECK(s.nsplit == r.nsplit && s.rows_per_split == r.rows_per_split && s.seg0 == r.seg0 && s.t_base == r.t_base);
        // every train row lies in exactly one split: splits [i * rps, min((i + 1) * rps, nt)) are disjoint by construction; they cover
        // [0, nt) and none is empty
        CHECK(s.nsplit >= 1 && s.rows_per_split % p.tt == 0 && (long long)s.nsplit * s.rows_per_split >= nt &&
              (long long)(s.nsplit - 1) * s.rows_per_split < nt);
        CHECK(s.seg0 == seg0 && s.t_base == t_base);
        seg0 += s.nsplit; t_base += nt;
    }
    CHECK(p.nseg == seg0);
    // the sequences
    const size_t n = p.launches.size();
    const int nt = c.n_trains, assigns = c.img_idx ? nt : 0;
    for (const BfLaunch &l : p.launches) {
        if (l.op == BF_OP_KNN_PASS || l.op == BF_OP_RADIUS_COUNT || l.op == BF_OP_RADIUS_WRITE)
            CHECK(l.gx == div_up(nq, 64) && l.m >= 0 && l.m < nt && l.gy == p.segs[l.m].nsplit && l.block == 64 * p.w);
    }
    size_t i = 0;
    if (radius) {
        CHECK(n == (size_t)(2 * nt + 1 + assigns));
        for (int m = 0; m < nt; ++m, ++i) CHECK(p.launches[i].op == BF_OP_RADIUS_COUNT && p.launches[i].m == m);
        CHECK(p.launches[i].op == BF_OP_RADIUS_SCAN); ++i;
        for (int m = 0; m < nt; ++m, ++i) CHECK(p.launches[i].op == BF_OP_RADIUS_WRITE && p.launches[i].m == m);
    } else {
        int covered = 0;   // the passes' columns tile [0, k) once, and each merge follows all passes of its block
        while (covered < k && i + nt < n) {
            const int ncol = imin(p.K, k - covered);
            for (int m = 0; m < nt; ++m, ++i) CHECK(p.launches[i].op == BF_OP_KNN_PASS && p.launches[i].m == m && p.launches[i].col0 == covered && p.launches[i].ncol == ncol);
            CHECK(p.launches[i].op == BF_OP_MERGE && p.launches[i].col0 == covered && p.launches[i].ncol == ncol); ++i;
            covered += ncol;
        }
        CHECK(covered == k);
    }
    CHECK(i + assigns == n);   // assign image: only with img_idx, once per train set, descending, last
    for (int m = nt - 1; m >= 0 && assigns && i < n; --m, ++i) CHECK(p.launches[i].op == BF_OP_ASSIGN_IMAGE && p.launches[i].m == m);
    for (size_t j = 0; j + assigns < n; ++j) CHECK(p.launches[j].op != BF_OP_ASSIGN_IMAGE);
}

static void expect_list(const Call &C, int knob, const std::vector<BfLaunch> &want)
{
    const BfPlan p = bf_make_plan(C.c, knob);
    CHECK(p.err.code == MI_OK && p.launches.size() == want.size());
    for (size_t i = 0; i < want.size() && i < p.launches.size(); ++i) CHECK(same(p.launches[i], want[i]));
}

static int n_rejected = 0;
// the new validator and the old sequence both give (code, text), and a rejecting plan sets nothing else
static void rejected(const BfCall &c, int code, const char *text)
{
    const BfPlan p = bf_make_plan(c, 4);
    const Old o = old_call(c, 4);
    const bool ok = p.err.code == code && p.err.msg && !strcmp(p.err.msg, text) && p.launches.empty() && p.segs.empty() && p.part_bytes == 0 && p.nq == 0;
    if (!ok) printf("  plan: %d '%s'; wanted %d '%s'\n", p.err.code, p.err.msg ? p.err.msg : "", code, text);
    CHECK(ok);
    CHECK(same_err(o.err, BfErr{code, text}));
    ++n_rejected;
}

int main()
{
    // ---- the table: k_knn's static_assert (D >= 2 W K scratch, whole 4-row groups per wave) for every instantiation; k_radius is one wave
    CHECK(kBfRowCount == 4);
    const BfRow want_rows[4] = {{64, 32, 4, 1}, {128, 32, 4, 1}, {256, 16, 4, 4}, {512, 8, 2, 2}};
    for (int r = 0; r < kBfRowCount; ++r) {
        const BfRow &R = kBfRows[r];
        CHECK(R.D == want_rows[r].D && R.TT == want_rows[r].TT && R.W == want_rows[r].W && R.W1 == want_rows[r].W1);
        for (int W : {R.W, R.W1})
            for (int K : {2, 8}) CHECK(R.TT % (4 * W) == 0 && R.D % 4 == 0 && R.D >= 2 * W * K);
        CHECK(bf_row_of(R.D) == r && bf_row_of(R.D + 1) == (r + 1 < kBfRowCount ? r + 1 : r));
    }
    CHECK(bf_list_len(1) == 2 && bf_list_len(2) == 2 && bf_list_len(3) == 8 && bf_list_len(1000) == 8);

    // ---- sweep
    long long n = 0;
    Call C;
    const int nqs[] = {1, 63, 64, 65, 150, 4096, 12564, 131073}, ds[] = {1, 17, 64, 65, 128, 129, 256, 257, 512}, ks[] = {1, 2, 3, 8, 9, 16, 17, 20};
    for (int nq : nqs)
        for (int d : ds) {
            const int tt = old_radius_shape(d).tt;
            for (int nt : {1, tt - 1, tt, tt + 1, 3 * tt + 1, 1000, 12564})
                for (int norm : {MI_NORM_L1, MI_NORM_L2})
                    for (int sets : {1, 4}) {
                        const std::vector<int> nts = sets == 1 ? std::vector<int>{nt} : std::vector<int>{nt, 33, 1, 260};
                        for (int knob : {4, 1}) {
                            for (int k : ks) {
                                make_call(C, BF_CALL_KNN, MI_32FC1, norm, nq, nts, d, k, 0, sets > 1 || k == 9);
                                check_plan(C, knob); ++n;
                            }
                            // (cols = max(n_t / 100, n_q) like the callers, capped: 131 073^2 entries are beyond the old code's int)
                            make_call(C, BF_CALL_RADIUS, MI_32FC1, norm, nq, nts, d, 0, imin(imax(nt / 100, nq), 5000), sets > 1 || nt == tt);
                            check_plan(C, knob); ++n;
                        }
                    }
        }
    CHECK(n == 8 * 9 * 7 * 2 * 2 * 2 * 9);
    // the fixed shapes are k = 1 and k = 2 of the same path
    for (int kind : {BF_CALL_MATCH, BF_CALL_KNN2})
        for (int nq : nqs)
            for (int d : ds) { make_call(C, kind, MI_32FC1, MI_NORM_L2, nq, {777}, d, 0, 0, false); check_plan(C, 4); ++n; }
    // the seven integer rows of the table
    const int int_rows[7][2] = {{MI_8UC1, MI_NORM_L1}, {MI_16UC1, MI_NORM_L1}, {MI_16SC1, MI_NORM_L1}, {MI_32SC1, MI_NORM_L1},
                                {MI_8UC1, MI_NORM_HAMMING}, {MI_16UC1, MI_NORM_HAMMING}, {MI_32SC1, MI_NORM_HAMMING}};
    long long ni = 0;
    for (const int (&tn)[2] : int_rows)
        for (int d : {1, 32, 61, 128})
            for (int nq : nqs)
                for (int nt : {1, 31, 32, 33, 97, 1000, 12564})
                    for (int sets : {1, 4}) {
                        const std::vector<int> nts = sets == 1 ? std::vector<int>{nt} : std::vector<int>{nt, 33, 1, 260};
                        for (int k : ks) {
                            make_call(C, BF_CALL_KNN, tn[0], tn[1], nq, nts, d, k, 0, sets > 1);
                            if (k > 16) rejected(C.c, MI_ERR_NOT_IMPL, "integer descriptors: 1 <= k <= 16");
                            else { check_plan(C, 4); ++ni; }
                        }
                        make_call(C, BF_CALL_RADIUS, tn[0], tn[1], nq, nts, d, 0, nq, sets > 1);
                        check_plan(C, 4); ++ni;
                    }
    CHECK(ni == 7 * 4 * 8 * 7 * 2 * 7 && n_rejected == 7 * 4 * 8 * 7 * 2 * 2);
    n += ni;
    const int swept_rejections = n_rejected;

    // ---- exact launch lists
    const std::vector<int> four = {700, 33, 1, 260};
    make_call(C, BF_CALL_KNN, MI_32FC1, MI_NORM_L2, 150, four, 64, 13, 0, true);
    {
        const BfPlan p = bf_make_plan(C.c, 4);
        const int nsplit[4] = {22, 2, 1, 9}, seg0[4] = {0, 22, 24, 25}, t_base[4] = {0, 700, 733, 734};
        CHECK(p.nseg == 34 && p.K == 8 && p.row == 0 && p.tt == 32 && p.w == 4 && p.part_bytes == 8u * 34 * 150 * 8);
        for (int m = 0; m < 4; ++m) CHECK(p.segs[m].nsplit == nsplit[m] && p.segs[m].rows_per_split == 32 && p.segs[m].seg0 == seg0[m] && p.segs[m].t_base == t_base[m]);
    }
    expect_list(C, 4, {{BF_OP_KNN_PASS, 0, 3, 22, 256, 0, 8}, {BF_OP_KNN_PASS, 1, 3, 2, 256, 0, 8}, {BF_OP_KNN_PASS, 2, 3, 1, 256, 0, 8},
                       {BF_OP_KNN_PASS, 3, 3, 9, 256, 0, 8}, {BF_OP_MERGE, -1, 1, 1, 256, 0, 8},
                       {BF_OP_KNN_PASS, 0, 3, 22, 256, 8, 5}, {BF_OP_KNN_PASS, 1, 3, 2, 256, 8, 5}, {BF_OP_KNN_PASS, 2, 3, 1, 256, 8, 5},
                       {BF_OP_KNN_PASS, 3, 3, 9, 256, 8, 5}, {BF_OP_MERGE, -1, 1, 1, 256, 8, 5},
                       {BF_OP_ASSIGN_IMAGE, 3, 8, 1, 256, 0, 13}, {BF_OP_ASSIGN_IMAGE, 2, 8, 1, 256, 0, 13}, {BF_OP_ASSIGN_IMAGE, 1, 8, 1, 256, 0, 13},
                       {BF_OP_ASSIGN_IMAGE, 0, 8, 1, 256, 0, 13}});
    make_call(C, BF_CALL_KNN, MI_32FC1, MI_NORM_L2, 12564, {12564}, 64, 2, 0, false);
    {
        const BfPlan p = bf_make_plan(C.c, 4);
        CHECK(p.nseg == 10 && p.K == 2 && p.segs[0].rows_per_split == 1280 && p.part_bytes == 8u * 10 * 12564 * 2);
    }
    expect_list(C, 4, {{BF_OP_KNN_PASS, 0, 197, 10, 256, 0, 2}, {BF_OP_MERGE, -1, 50, 1, 256, 0, 2}});
    expect_list(C, 1, {{BF_OP_KNN_PASS, 0, 197, 10, 64, 0, 2}, {BF_OP_MERGE, -1, 50, 1, 256, 0, 2}});
    make_call(C, BF_CALL_RADIUS, MI_32FC1, MI_NORM_L1, 150, four, 64, 0, 150, true);
    CHECK(bf_make_plan(C.c, 4).part_bytes == 4u * 34 * 150);
    expect_list(C, 4, {{BF_OP_RADIUS_COUNT, 0, 3, 22, 64, 0, 150}, {BF_OP_RADIUS_COUNT, 1, 3, 2, 64, 0, 150}, {BF_OP_RADIUS_COUNT, 2, 3, 1, 64, 0, 150},
                       {BF_OP_RADIUS_COUNT, 3, 3, 9, 64, 0, 150}, {BF_OP_RADIUS_SCAN, -1, 1, 1, 256, 0, 150},
                       {BF_OP_RADIUS_WRITE, 0, 3, 22, 64, 0, 150}, {BF_OP_RADIUS_WRITE, 1, 3, 2, 64, 0, 150}, {BF_OP_RADIUS_WRITE, 2, 3, 1, 64, 0, 150},
                       {BF_OP_RADIUS_WRITE, 3, 3, 9, 64, 0, 150},
                       {BF_OP_ASSIGN_IMAGE, 3, 88, 1, 256, 0, 150}, {BF_OP_ASSIGN_IMAGE, 2, 88, 1, 256, 0, 150}, {BF_OP_ASSIGN_IMAGE, 1, 88, 1, 256, 0, 150},
                       {BF_OP_ASSIGN_IMAGE, 0, 88, 1, 256, 0, 150}});
    make_call(C, BF_CALL_KNN, MI_8UC1, MI_NORM_HAMMING, 70, {130, 40}, 32, 16, 0, true);
    expect_list(C, 4, {{BF_OP_INT_KNN, 0, 2, 1, 64, 0, 16}, {BF_OP_INT_KNN, 1, 2, 1, 64, 0, 16}});

    // ---- the type table: every (depth, norm) pair against the reference's three caller arrays (brute_force_matcher.cpp:339-356;
    // depth 6 = CV_64F is refused by the assert of :331), as a predicate and through a whole call
    const int norms[3] = {MI_NORM_L1, MI_NORM_L2, MI_NORM_HAMMING};
    const bool callers[3][7] = {{true, false, true, true, true, true, false}, {false, false, false, false, false, true, false},
                                {true, false, true, false, true, false, false}};
    for (int ni3 = 0; ni3 < 3; ++ni3)
        for (int depth = 0; depth < 7; ++depth) {
            CHECK(bf_type_norm_ok(depth, norms[ni3]) == callers[ni3][depth]);
            make_call(C, BF_CALL_KNN, depth, norms[ni3], 10, {20}, 32, 2, 0, false);
            if (callers[ni3][depth]) CHECK(bf_make_plan(C.c, 4).err.code == MI_OK && old_call(C.c, 4).err.code == MI_OK);
            else rejected(C.c, MI_ERR_BAD_TYPE, "unsupported combination of query.depth() and norm");
            make_call(C, BF_CALL_RADIUS, depth, norms[ni3], 10, {20}, 32, 0, 10, false);
            if (callers[ni3][depth]) CHECK(bf_make_plan(C.c, 4).err.code == MI_OK && old_call(C.c, 4).err.code == MI_OK);
            else rejected(C.c, MI_ERR_BAD_TYPE, "unsupported combination of query.depth() and norm");
        }
    CHECK(n_rejected - swept_rejections == 2 * 12);   // the twelve empty slots of the three arrays (with depth 6), k-nearest and radius
    for (int norm = -1; norm < 10; ++norm) CHECK((bf_type_norm_ok(MI_32FC1, norm) || bf_type_norm_ok(MI_8UC1, norm)) == (norm == 2 || norm == 4 || norm == 6));   // mi_bf_create
    CHECK(!bf_type_norm_ok(MI_32FC1, 7) && !bf_type_norm_ok(MI_32FC2, MI_NORM_L2));

    // ---- rejections: one input per requirement, in the order of the calls
    const char *NULLARG = "null argument", *COLL = "a collection needs img_idx", *COMBO = "unsupported combination of query.depth() and norm";
    const char *OUT1 = "outputs must be 1 x query.rows", *KNN_OUT = "train_idx / img_idx CV_32SC1 and distance CV_32FC1 must be query.rows x k";
    const char *RAD_OUT = "train_idx / img_idx CV_32SC1, distance CV_32FC1: query.rows x cols; n_matches CV_32SC1 1 x query.rows";
    const char *TRAIN_SIZE = "query.cols == train.cols, non-empty", *MASK = "mask must be CV_8UC1, query.rows x train.rows";
    const auto base = [&](int kind, int type = MI_32FC1, int norm = MI_NORM_L2, bool img = true, bool masks = false) {
        make_call(C, kind, type, norm, 50, kind <= BF_CALL_KNN2 ? std::vector<int>{70} : std::vector<int>{70, 30}, 32, 3, 50, img, masks);
    };
    // mi_bf_match / mi_bf_knn_match2
    for (int kind : {BF_CALL_MATCH, BF_CALL_KNN2}) {
        base(kind); C.c.query = nullptr; rejected(C.c, MI_ERR_BAD_ARG, NULLARG);
        base(kind); C.c.trains = nullptr; rejected(C.c, MI_ERR_BAD_ARG, NULLARG);
        base(kind); C.c.train_idx = nullptr; rejected(C.c, MI_ERR_BAD_ARG, NULLARG);
        base(kind); C.c.distance = nullptr; rejected(C.c, MI_ERR_BAD_ARG, NULLARG);
        base(kind); C.ti.data = nullptr; rejected(C.c, MI_ERR_BAD_ARG, NULLARG);
        base(kind); C.di.data = nullptr; rejected(C.c, MI_ERR_BAD_ARG, NULLARG);
        const char *ty = kind == BF_CALL_MATCH ? "train_idx CV_32SC1 / distance CV_32FC1" : "k = 2: train_idx CV_32SC2 / distance CV_32FC2";
        base(kind); C.ti.type = MI_32FC1; rejected(C.c, MI_ERR_BAD_TYPE, ty);
        base(kind); C.di.type = MI_32SC1; rejected(C.c, MI_ERR_BAD_TYPE, ty);
        base(kind); C.ti.rows = 2; rejected(C.c, MI_ERR_BAD_SIZE, OUT1);
        base(kind); C.di.cols = 49; rejected(C.c, MI_ERR_BAD_SIZE, OUT1);
        base(kind); C.c.handle = false; rejected(C.c, MI_ERR_BAD_ARG, "null handle");
        base(kind); C.trains[0].cols = 31; rejected(C.c, MI_ERR_BAD_SIZE, TRAIN_SIZE);
        base(kind, MI_8UC1, MI_NORM_HAMMING); C.query.cols = C.trains[0].cols = 129;
        rejected(C.c, MI_ERR_BAD_SIZE, "integer descriptors of up to 128 elements; longer ones are not built");
    }
    // mi_bf_knn_match
    base(BF_CALL_KNN); C.c.query = nullptr; rejected(C.c, MI_ERR_BAD_ARG, NULLARG);
    base(BF_CALL_KNN); C.c.trains = nullptr; rejected(C.c, MI_ERR_BAD_ARG, NULLARG);
    base(BF_CALL_KNN); C.c.train_idx = nullptr; rejected(C.c, MI_ERR_BAD_ARG, NULLARG);
    base(BF_CALL_KNN); C.c.distance = nullptr; rejected(C.c, MI_ERR_BAD_ARG, NULLARG);
    base(BF_CALL_KNN); C.c.k = 0; rejected(C.c, MI_ERR_BAD_ARG, "k >= 1");
    base(BF_CALL_KNN); C.ti.data = nullptr; rejected(C.c, MI_ERR_BAD_SIZE, KNN_OUT);
    base(BF_CALL_KNN); C.ti.type = MI_32FC1; rejected(C.c, MI_ERR_BAD_SIZE, KNN_OUT);
    base(BF_CALL_KNN); C.di.rows = 49; rejected(C.c, MI_ERR_BAD_SIZE, KNN_OUT);
    base(BF_CALL_KNN); C.im.cols = 4; rejected(C.c, MI_ERR_BAD_SIZE, KNN_OUT);
    base(BF_CALL_KNN); C.c.handle = false; rejected(C.c, MI_ERR_BAD_ARG, "null handle");
    // mi_bf_radius_match
    base(BF_CALL_RADIUS); C.c.handle = false; rejected(C.c, MI_ERR_BAD_ARG, NULLARG);
    base(BF_CALL_RADIUS); C.c.query = nullptr; rejected(C.c, MI_ERR_BAD_ARG, NULLARG);
    base(BF_CALL_RADIUS); C.c.trains = nullptr; rejected(C.c, MI_ERR_BAD_ARG, NULLARG);
    base(BF_CALL_RADIUS); C.c.train_idx = nullptr; rejected(C.c, MI_ERR_BAD_ARG, NULLARG);
    base(BF_CALL_RADIUS); C.c.distance = nullptr; rejected(C.c, MI_ERR_BAD_ARG, NULLARG);
    base(BF_CALL_RADIUS); C.c.n_matches = nullptr; rejected(C.c, MI_ERR_BAD_ARG, NULLARG);
    base(BF_CALL_RADIUS, MI_32FC1, MI_NORM_L2, false); rejected(C.c, MI_ERR_BAD_ARG, COLL);
    base(BF_CALL_RADIUS, MI_8UC1, MI_NORM_L1, false); rejected(C.c, MI_ERR_BAD_ARG, COLL);
    base(BF_CALL_RADIUS); C.ti.cols = C.di.cols = C.im.cols = 0; rejected(C.c, MI_ERR_BAD_SIZE, RAD_OUT);
    base(BF_CALL_RADIUS); C.di.cols = 49; rejected(C.c, MI_ERR_BAD_SIZE, RAD_OUT);
    base(BF_CALL_RADIUS); C.im.type = MI_32FC1; rejected(C.c, MI_ERR_BAD_SIZE, RAD_OUT);
    base(BF_CALL_RADIUS); C.nm.rows = 50; C.nm.cols = 1; rejected(C.c, MI_ERR_BAD_SIZE, RAD_OUT);
    base(BF_CALL_RADIUS); C.nm.data = nullptr; rejected(C.c, MI_ERR_BAD_SIZE, RAD_OUT);
    // both descriptor families, k-nearest and radius
    for (int kind : {BF_CALL_KNN, BF_CALL_RADIUS})
        for (int flt = 0; flt < 2; ++flt) {
            const int type = flt ? MI_32FC1 : MI_16UC1, norm = MI_NORM_L1;
            base(kind, type, flt ? MI_NORM_HAMMING : MI_NORM_L2); rejected(C.c, MI_ERR_BAD_TYPE, COMBO);
            if (kind == BF_CALL_KNN) { base(kind, type, norm, false); rejected(C.c, MI_ERR_BAD_ARG, COLL); }
            base(kind, type, norm); C.query.data = nullptr; rejected(C.c, MI_ERR_BAD_ARG, NULLARG);
            base(kind, type, norm); C.c.n_trains = 0; rejected(C.c, MI_ERR_BAD_ARG, NULLARG);
            base(kind, type, norm); C.c.n_trains = -1; rejected(C.c, MI_ERR_BAD_ARG, NULLARG);
            base(kind, type, norm); C.query.rows = C.ti.rows = C.di.rows = C.im.rows = 0; C.nm.cols = 0; rejected(C.c, MI_ERR_BAD_SIZE, "empty query");
            base(kind, type, norm); C.query.cols = 0; rejected(C.c, MI_ERR_BAD_SIZE, "empty query");
            base(kind, type, norm); C.query.cols = C.trains[0].cols = C.trains[1].cols = flt ? 513 : 129;
            rejected(C.c, MI_ERR_BAD_SIZE, flt ? "descriptor length <= 512; longer descriptors are not built"
                                               : "integer descriptors of up to 128 elements; longer ones are not built");
            base(kind, type, norm); C.query.cols = C.trains[0].cols = C.trains[1].cols = flt ? 512 : 128; CHECK(bf_make_plan(C.c, 4).err.code == MI_OK);
            const char *tty = flt ? "descriptors must be CV_32FC1" : "train.type() == query.type()";
            base(kind, type, norm); C.trains[1].type = flt ? MI_16UC1 : MI_32FC1; rejected(C.c, MI_ERR_BAD_TYPE, tty);
            base(kind, type, norm); C.trains[0].data = nullptr; rejected(C.c, MI_ERR_BAD_TYPE, tty);
            base(kind, type, norm); C.trains[1].rows = 0; rejected(C.c, MI_ERR_BAD_SIZE, TRAIN_SIZE);
            base(kind, type, norm); C.trains[1].cols = 31; rejected(C.c, MI_ERR_BAD_SIZE, TRAIN_SIZE);
            base(kind, type, norm, true, true); C.masks[1].type = MI_32SC1; rejected(C.c, MI_ERR_BAD_SIZE, MASK);
            base(kind, type, norm, true, true); C.masks[0].rows = 49; rejected(C.c, MI_ERR_BAD_SIZE, MASK);
            base(kind, type, norm, true, true); C.masks[1].cols = 70; rejected(C.c, MI_ERR_BAD_SIZE, MASK);
            base(kind, type, norm, true, true); C.masks[0].data = nullptr; C.masks[0].cols = 1; CHECK(bf_make_plan(C.c, 4).err.code == MI_OK);   // data == NULL: no mask
            // INT_MAX train rows: the float family's lists index the concatenated collection
            base(kind, type, norm); C.trains[0].rows = 1 << 30; C.trains[1].rows = (1 << 30) - 1;   // INT_MAX rows; one fewer below (one set close to INT_MAX overflowed the old int div_up)
            if (flt) rejected(C.c, MI_ERR_BAD_SIZE, "train collection too large");
            else CHECK(bf_make_plan(C.c, 4).err.code == MI_OK && old_call(C.c, 4).err.code == MI_OK);
            base(kind, type, norm); C.trains[0].rows = 1 << 30; C.trains[1].rows = (1 << 30) - 2; CHECK(bf_make_plan(C.c, 4).err.code == MI_OK && old_call(C.c, 4).err.code == MI_OK);
        }
    base(BF_CALL_KNN, MI_32SC1, MI_NORM_HAMMING); C.c.k = 17; C.ti.cols = C.di.cols = C.im.cols = 17;
    rejected(C.c, MI_ERR_NOT_IMPL, "integer descriptors: 1 <= k <= 16");

    // ---- two faults at once: the winner is the one the calls tested first
    base(BF_CALL_KNN, MI_32FC1, MI_NORM_HAMMING); C.c.n_trains = 0; rejected(C.c, MI_ERR_BAD_TYPE, COMBO);         // float: the table before the matrices
    base(BF_CALL_KNN, MI_16UC1, MI_NORM_L2); C.c.n_trains = 0; rejected(C.c, MI_ERR_BAD_ARG, NULLARG);              // integer: after
    base(BF_CALL_KNN, MI_32FC1, MI_NORM_HAMMING, false); rejected(C.c, MI_ERR_BAD_TYPE, COMBO);                    // float: the table before img_idx
    base(BF_CALL_KNN, MI_32FC1, MI_NORM_L2, false); C.query.data = nullptr; rejected(C.c, MI_ERR_BAD_ARG, COLL);    // float: img_idx before the matrices
    base(BF_CALL_KNN, MI_8UC1, MI_NORM_L1, false); C.query.data = nullptr; rejected(C.c, MI_ERR_BAD_ARG, NULLARG);  // integer: img_idx last
    base(BF_CALL_KNN, MI_8UC1, MI_NORM_L1, false); C.trains[1].cols = 31; rejected(C.c, MI_ERR_BAD_SIZE, TRAIN_SIZE);
    base(BF_CALL_KNN, MI_8UC1, MI_NORM_L1, false); C.c.k = 17; C.ti.cols = C.di.cols = 17; rejected(C.c, MI_ERR_NOT_IMPL, "integer descriptors: 1 <= k <= 16");
    base(BF_CALL_KNN, MI_8UC1, MI_NORM_L1); C.c.k = 17; C.ti.cols = C.di.cols = C.im.cols = 17; C.query.cols = 129;
    rejected(C.c, MI_ERR_BAD_SIZE, "integer descriptors of up to 128 elements; longer ones are not built");
    base(BF_CALL_KNN); C.c.handle = false; C.c.k = 0; rejected(C.c, MI_ERR_BAD_ARG, "k >= 1");                      // the outputs before the handle
    base(BF_CALL_KNN); C.c.handle = false; C.di.rows = 49; rejected(C.c, MI_ERR_BAD_SIZE, KNN_OUT);
    base(BF_CALL_KNN, MI_32FC1, MI_NORM_HAMMING); C.c.handle = false; rejected(C.c, MI_ERR_BAD_ARG, "null handle");
    base(BF_CALL_MATCH); C.c.handle = false; C.ti.type = MI_32SC2; rejected(C.c, MI_ERR_BAD_TYPE, "train_idx CV_32SC1 / distance CV_32FC1");
    base(BF_CALL_RADIUS, MI_32FC1, MI_NORM_HAMMING, false); rejected(C.c, MI_ERR_BAD_ARG, COLL);                    // radius: img_idx before everything but NULLs
    base(BF_CALL_RADIUS, MI_32FC1, MI_NORM_HAMMING); C.di.cols = 49; rejected(C.c, MI_ERR_BAD_SIZE, RAD_OUT);
    base(BF_CALL_KNN); C.trains[0].cols = 31; C.trains[1].type = MI_8UC1; rejected(C.c, MI_ERR_BAD_SIZE, TRAIN_SIZE);   // set 0 before set 1
    base(BF_CALL_KNN, MI_32FC1, MI_NORM_L2, true, true); C.trains[0].rows = 0; C.masks[0].cols = 0; C.trains[1].data = nullptr;
    rejected(C.c, MI_ERR_BAD_SIZE, TRAIN_SIZE);
    base(BF_CALL_KNN); C.query.rows = C.ti.rows = C.di.rows = C.im.rows = 0; C.query.cols = 513; rejected(C.c, MI_ERR_BAD_SIZE, "empty query");

    // ---- the 32-bit bound of k_assign_image's index: the one call the old code ran (with a garbage grid) and the plan rejects
    const char *BITS = "query.rows x output columns must fit 32 bits";
    const auto rejected_new = [&](const BfCall &c) {
        const BfPlan p = bf_make_plan(c, 4);
        CHECK(p.err.code == MI_ERR_BAD_SIZE && !strcmp(p.err.msg, BITS) && p.launches.empty());
        BfCall c2 = c;   // the old validation passed the call; its int product is formed for img_idx only, so it is not restated with one
        c2.img_idx = nullptr;
        CHECK(old_call(c2, 4).err.code == MI_OK);
    };
    make_call(C, BF_CALL_RADIUS, MI_32FC1, MI_NORM_L2, 46341, {100}, 64, 0, 46341, true); rejected_new(C.c);      // 46 341^2 = 2^31 + 4 633
    make_call(C, BF_CALL_RADIUS, MI_32FC1, MI_NORM_L2, 46340, {100, 20}, 64, 0, 46340, true); check_plan(C, 4);
    CHECK(bf_make_plan(C.c, 4).launches.back().gx == (int)((46340ll * 46340 + 255) / 256));
    make_call(C, BF_CALL_RADIUS, MI_32FC1, MI_NORM_L2, 46341, {100}, 64, 0, 46341, false);                            // no img_idx: 64-bit indices throughout
    CHECK(bf_make_plan(C.c, 4).err.code == MI_OK);
    make_call(C, BF_CALL_KNN, MI_32FC1, MI_NORM_L2, 65536, {100}, 64, 32768, 0, true); rejected_new(C.c);         // n_q k = 2^31
    make_call(C, BF_CALL_KNN, MI_32FC1, MI_NORM_L2, 65536, {100, 20}, 64, 32767, 0, true); check_plan(C, 4);
    make_call(C, BF_CALL_RADIUS, MI_32SC1, MI_NORM_L1, 46341, {100, 20}, 64, 0, 46341, true); CHECK(bf_make_plan(C.c, 4).err.code == MI_OK);   // integer family: 64-bit

    if (fails) { printf("bf_plan_test: %d FAILED\n", fails); return 1; }
    printf("bf_plan_test: ok (%lld plans, %d rejections)\n", n, n_rejected);
    return 0;
}
