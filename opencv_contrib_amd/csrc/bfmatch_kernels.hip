// Brute-force matcher for float descriptors (SURF output), NORM_L1 / NORM_L2, gfx950.  Replaces cudafeatures2d/src/cuda/bf_match.cu,
// bf_knnmatch.cu and bf_radius_match.cu behind the C-ABI (match, knnMatch for any k, radiusMatch; single train set or a collection).
//
// Layout: a lane owns one QUERY; the 64 queries of a workgroup sit transposed in LDS (conflict-free lane-contiguous reads) and the
// train set streams through LDS in tiles read as broadcasts, four train descriptors at a time = four independent accumulation
// chains per lane.  W waves of a workgroup share the queries and the tile and take TT / W rows of every tile each.  The train
// range is cut into contiguous splits over blockIdx.y so that a few thousand queries still fill 256 CUs.  Every lane keeps its K
// best candidates as a list sorted by (distance, index) -- the order the reference's strict-< scan over ascending train indices
// produces -- so waves, splits and images can be merged in any order; a second kernel merges the per-split lists.  k > K runs
// further passes that only admit candidates after the last entry found so far (no distance matrix).  Distances follow the
// reference's summation order exactly (k ascending; L2: sum = fma(d, d, sum) then sqrtf; L1: sum += |d|), so the HIP result is
// bit-identical to oracle/bfmatch_ref.c.
#include "bf_dispatch.h"
#include <cfloat>
#include <climits>

namespace mi {
namespace bf {

// K best (distance, index) pairs of a lane, ascending; empty slots are (FLT_MAX, INT_MAX).  push() keeps the K smallest pairs in
// lexicographic order, which is what "if (d < best1) {...} else if (d < best2) {...}" (bf_knnmatch.cu:353-371) yields when the
// candidates arrive in ascending index order, and does not depend on the arrival order.
template <int K>
struct KBest {
    float d[K];
    int i[K];
    __device__ __forceinline__ void init()
    {
#pragma unroll
        for (int j = 0; j < K; ++j) { d[j] = FLT_MAX; i[j] = INT_MAX; }
    }
    __device__ __forceinline__ void push(float dv, int ti, bool ok)
    {
        ok = ok && dv < FLT_MAX && (dv < d[K - 1] || (dv == d[K - 1] && ti < i[K - 1]));
        if (!__any(ok)) return;          // wave-uniform: after the first tiles almost no candidate enters the list
        if (ok) { d[K - 1] = dv; i[K - 1] = ti; }
#pragma unroll
        for (int j = K - 1; j > 0; --j) {
            const bool sw = d[j] < d[j - 1] || (d[j] == d[j - 1] && i[j] < i[j - 1]);
            const float dl = sw ? d[j] : d[j - 1], dh = sw ? d[j - 1] : d[j];
            const int il = sw ? i[j] : i[j - 1], ih = sw ? i[j - 1] : i[j];
            d[j - 1] = dl; d[j] = dh; i[j - 1] = il; i[j] = ih;
        }
    }
};

// 64 queries of the workgroup, transposed (s_q[k][query]); zero padding like loadQueryToSmem, bf_match.cu:81-90
template <int D, int W>
__device__ __forceinline__ void stage_queries(const Args &A, float *s_q)
{
    for (int e = threadIdx.x; e < D * 64; e += 64 * W) {   // e = ql * D + k: global reads run along the rows
        const int ql = e / D, k = e % D;
        const int qrow = min((int)blockIdx.x * 64 + ql, A.nq - 1);
        s_q[k * 64 + ql] = k < A.d ? reinterpret_cast<const float *>(reinterpret_cast<const char *>(A.q) + (size_t)qrow * A.qstep)[k] : 0.f;
    }
}

template <int D, int TT, int W>
__device__ __forceinline__ void stage_tile(const Args &A, int tb, float *s_t)
{
    for (int e = threadIdx.x; e < TT * D; e += 64 * W) {
        const int r = e / D, k = e % D;
        const int tr = min(tb + r, A.nt - 1);
        s_t[e] = k < A.d ? reinterpret_cast<const float *>(reinterpret_cast<const char *>(A.t) + (size_t)tr * A.tstep)[k] : 0.f;
    }
}

template <int NORM>
__device__ __forceinline__ void acc(float &s, float q, float t)
{
    const float e = q - t;
    if (NORM == MI_NORM_L2) s = fmaf(e, e, s);      // L2Dist::reduceIter, one fma
    else s = s + fabsf(e);                          // L1Dist::reduceIter
}

// distances of this lane's query to the four train descriptors at p0: four independent k-ascending chains (bf_match.cu:100-121)
template <int D, int NORM>
__device__ __forceinline__ void dist4(const float *s_q, const float *p0, int lane, float (&dv)[4])
{
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
#pragma unroll 2
    for (int k = 0; k < D; k += 4) {
        const float q0 = s_q[k * 64 + lane], q1 = s_q[(k + 1) * 64 + lane], q2 = s_q[(k + 2) * 64 + lane], q3 = s_q[(k + 3) * 64 + lane];
        const float4 a = *reinterpret_cast<const float4 *>(p0 + k), b = *reinterpret_cast<const float4 *>(p0 + D + k);
        const float4 c = *reinterpret_cast<const float4 *>(p0 + 2 * D + k), d = *reinterpret_cast<const float4 *>(p0 + 3 * D + k);
        acc<NORM>(s0, q0, a.x); acc<NORM>(s0, q1, a.y); acc<NORM>(s0, q2, a.z); acc<NORM>(s0, q3, a.w);
        acc<NORM>(s1, q0, b.x); acc<NORM>(s1, q1, b.y); acc<NORM>(s1, q2, b.z); acc<NORM>(s1, q3, b.w);
        acc<NORM>(s2, q0, c.x); acc<NORM>(s2, q1, c.y); acc<NORM>(s2, q2, c.z); acc<NORM>(s2, q3, c.w);
        acc<NORM>(s3, q0, d.x); acc<NORM>(s3, q1, d.y); acc<NORM>(s3, q2, d.z); acc<NORM>(s3, q3, d.w);
    }
    if (NORM == MI_NORM_L2) { dv[0] = sqrtf(s0); dv[1] = sqrtf(s1); dv[2] = sqrtf(s2); dv[3] = sqrtf(s3); }
    else { dv[0] = s0; dv[1] = s1; dv[2] = s2; dv[3] = s3; }
}

// W waves per workgroup, 64 queries (lane = query), runtime loops with a 4 x 4 (train x k) body, so no large register arrays (a
// lane-resident query of 64-128 floats made the compiler hoist every LDS read of the unrolled chain and spill).
template <int D, int TT, int W, int NORM, int K>
__global__ __launch_bounds__(64 * W) void k_knn(Args A)
{
    static_assert(TT % (4 * W) == 0 && D % 4 == 0 && D >= 2 * W * K, "tile / scratch shape");
    __shared__ __attribute__((aligned(16))) float s_q[D * 64];
    __shared__ __attribute__((aligned(16))) float s_t[TT * D];
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    const int qi = blockIdx.x * 64 + lane;
    const int split = blockIdx.y;
    const int t0 = split * A.rows_per_split, t1 = min(t0 + A.rows_per_split, A.nt);
    stage_queries<D, W>(A, s_q);
    float lo_d = -1.f;
    int lo_i = -1;
    if (A.lo_idx && qi < A.nq) {
        lo_i = A.lo_idx[(size_t)qi * A.lo_istep];
        lo_d = lo_i < 0 ? FLT_MAX : A.lo_dist[(size_t)qi * A.lo_dstep];     // list already exhausted: admit nothing
    }
    KBest<K> best;
    best.init();
    constexpr int RW = TT / W;      // tile rows per wave
#pragma unroll 1
    for (int tb = t0; tb < t1; tb += TT) {
        __syncthreads();
        stage_tile<D, TT, W>(A, tb, s_t);
        __syncthreads();
        const int nrow = min(TT, t1 - tb);
        const int rend = min((wv + 1) * RW, nrow);
#pragma unroll 1
        for (int r = wv * RW; r < rend; r += 4) {
            float dv[4];
            dist4<D, NORM>(s_q, s_t + r * D, lane, dv);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int tl = tb + r + j;
                bool ok = (r + j < nrow) && qi < A.nq;
                if (ok && A.mask) ok = A.mask[(size_t)qi * A.mstep + tl] != 0;
                const int ti = A.t_base + tl;
                ok = ok && (dv[j] > lo_d || (dv[j] == lo_d && ti > lo_i));
                best.push(dv[j], ti, ok);
            }
        }
    }
    if (W > 1) {                     // fold the other waves' lists into wave 0's through the (now free) query area
        __syncthreads();
        float *sc = s_q;             // [W][K][2][64]
        if (wv > 0) {
#pragma unroll
            for (int j = 0; j < K; ++j) {
                sc[((wv * K + j) * 2 + 0) * 64 + lane] = best.d[j];
                sc[((wv * K + j) * 2 + 1) * 64 + lane] = __int_as_float(best.i[j]);
            }
        }
        __syncthreads();
        if (wv == 0) {
#pragma unroll 1
            for (int w = 1; w < W; ++w) {
#pragma unroll
                for (int j = 0; j < K; ++j)
                    best.push(sc[((w * K + j) * 2 + 0) * 64 + lane], __float_as_int(sc[((w * K + j) * 2 + 1) * 64 + lane]), true);
            }
        }
    }
    if (wv == 0 && qi < A.nq) {
        float2 *o = A.part + ((size_t)(A.seg0 + split) * A.nq + qi) * K;
#pragma unroll
        for (int j = 0; j < K; ++j) o[j] = make_float2(best.d[j], __int_as_float(best.i[j]));
    }
}

// merges the segment lists of every query; writes columns [col0, col0 + ncol) of the n_q x k outputs (element strides per query)
template <int K>
__global__ __launch_bounds__(256) void k_merge(const float2 *part, int nq, int nseg, int *idx, size_t istep, float *dist, size_t dstep,
                                               int *img, size_t mstep, int col0, int ncol)
{
    const int qi = blockIdx.x * 256 + threadIdx.x;
    if (qi >= nq) return;
    KBest<K> b;
    b.init();
    for (int s = 0; s < nseg; ++s) {
        const float2 *p = part + ((size_t)s * nq + qi) * K;
#pragma unroll
        for (int j = 0; j < K; ++j) b.push(p[j].x, __float_as_int(p[j].y), true);
    }
#pragma unroll
    for (int j = 0; j < K; ++j) {
        if (j >= ncol) break;
        const bool none = b.i[j] == INT_MAX;
        idx[(size_t)qi * istep + col0 + j] = none ? -1 : b.i[j];
        dist[(size_t)qi * dstep + col0 + j] = b.d[j];
        if (img) img[(size_t)qi * mstep + col0 + j] = none ? -1 : -2;      // -2: collection index not yet resolved
    }
}

// Collection index -> (image, train index).  Launched for m = n_trains - 1 ... 0: an unresolved entry >= off belongs to image m.
__global__ __launch_bounds__(256) void k_assign_image(int *idx, size_t istep, int *img, size_t mstep, int nq, int ncols,
                                                      const int *nvalid, int off, int m)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= nq * ncols) return;
    const int q = e / ncols, j = e % ncols;
    if (nvalid && j >= min(nvalid[q], ncols)) return;
    int *pi = idx + (size_t)q * istep + j, *pm = img + (size_t)q * mstep + j;
    if (*pm == -2 && *pi >= off) { *pm = m; *pi -= off; }
}

// radiusMatch, one wave per workgroup.  Pass 0 (write = 0) counts the hits of every (segment, query); k_radius_scan turns the counts
// into output slots; pass 1 recomputes the distances and stores the hits, so a row lists them in ascending collection order.
template <int D, int TT, int NORM>
__global__ __launch_bounds__(64) void k_radius(Args A)
{
    __shared__ __attribute__((aligned(16))) float s_q[D * 64];
    __shared__ __attribute__((aligned(16))) float s_t[TT * D];
    const int lane = threadIdx.x;
    const int qi = blockIdx.x * 64 + lane;
    const int split = blockIdx.y;
    const int t0 = split * A.rows_per_split, t1 = min(t0 + A.rows_per_split, A.nt);
    stage_queries<D, 1>(A, s_q);
    const size_t slot = (size_t)(A.seg0 + split) * A.nq + min(qi, A.nq - 1);
    const int base = A.write ? A.cnt[slot] : 0;
    int n = 0;
#pragma unroll 1
    for (int tb = t0; tb < t1; tb += TT) {
        __syncthreads();
        stage_tile<D, TT, 1>(A, tb, s_t);
        __syncthreads();
        const int nrow = min(TT, t1 - tb);
#pragma unroll 1
        for (int r = 0; r < nrow; r += 4) {
            float dv[4];
            dist4<D, NORM>(s_q, s_t + r * D, lane, dv);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int tl = tb + r + j;
                bool ok = (r + j < nrow) && qi < A.nq;
                if (ok && A.mask) ok = A.mask[(size_t)qi * A.mstep + tl] != 0;
                ok = ok && dv[j] < A.max_dist;                       // bf_radius_match.cu:106
                if (ok) {
                    const int pos = base + n;
                    if (A.write && pos < A.cols) {
                        A.r_idx[(size_t)qi * A.r_istep + pos] = A.t_base + tl;
                        A.r_dist[(size_t)qi * A.r_dstep + pos] = dv[j];
                        if (A.r_img) A.r_img[(size_t)qi * A.r_mstep + pos] = -2;
                    }
                    ++n;
                }
            }
        }
    }
    if (!A.write && qi < A.nq) A.cnt[slot] = n;
}

__global__ __launch_bounds__(256) void k_radius_scan(int *cnt, int nq, int nseg, int *n_matches)
{
    const int qi = blockIdx.x * 256 + threadIdx.x;
    if (qi >= nq) return;
    int run = 0;
    for (int s = 0; s < nseg; ++s) {
        const int c = cnt[(size_t)s * nq + qi];
        cnt[(size_t)s * nq + qi] = run;
        run += c;
    }
    n_matches[qi] = run;             // every hit is counted, like the reference's atomicInc (may exceed cols)
}

// ------------------------------------------------------------------------------------------------ launcher
// The kernel of a plan's passes, instantiated from kBfRows (bf_plan.h) and nowhere else: per row k_knn<D, TT, W | W1, L2 | L1, 2 | 8>
// and k_radius<D, TT, L2 | L1>; rows whose W1 equals W name one kernel twice: 24 k_knn, 8 k_radius.
typedef void (*kernel_t)(Args);

template <int R = 0>
static kernel_t kernel_of(const BfPlan &p)
{
    constexpr BfRow r = kBfRows[R];
    constexpr int L2 = MI_NORM_L2, L1 = MI_NORM_L1;
    if constexpr (R + 1 < kBfRowCount) if (p.row != R) return kernel_of<R + 1>(p);
    static const kernel_t tab[3][2][2] = {   // [radius, K = 2, K = 8][W, W1][L2, L1]
        {{k_radius<r.D, r.TT, L2>, k_radius<r.D, r.TT, L1>}, {k_radius<r.D, r.TT, L2>, k_radius<r.D, r.TT, L1>}},
        {{k_knn<r.D, r.TT, r.W, L2, 2>, k_knn<r.D, r.TT, r.W, L1, 2>}, {k_knn<r.D, r.TT, r.W1, L2, 2>, k_knn<r.D, r.TT, r.W1, L1, 2>}},
        {{k_knn<r.D, r.TT, r.W, L2, 8>, k_knn<r.D, r.TT, r.W, L1, 8>}, {k_knn<r.D, r.TT, r.W1, L2, 8>, k_knn<r.D, r.TT, r.W1, L1, 8>}}};
    return tab[p.K == 0 ? 0 : p.K == 2 ? 1 : 2][p.w != r.W][p.norm == L1];
}

void launch(const BfPlan &p, const BfLaunch &l, const Args &A, const bfint::Lists &o, int *n_matches, hipStream_t st)
{
    const dim3 grid(l.gx, l.gy), block(l.block);
    if (l.op == BF_OP_MERGE)
        hipLaunchKernelGGL((p.K == 2 ? k_merge<2> : k_merge<8>), grid, block, 0, st, A.part, A.nq, p.nseg, o.idx, (size_t)o.istep, o.dist,
                           (size_t)o.dstep, o.img, (size_t)o.mstep, l.col0, l.ncol);
    else if (l.op == BF_OP_ASSIGN_IMAGE)   // radius match: only the entries a row holds (n_matches) are resolved
        hipLaunchKernelGGL(k_assign_image, grid, block, 0, st, o.idx, (size_t)o.istep, o.img, (size_t)o.mstep, A.nq, p.cols,
                           p.k ? nullptr : n_matches, p.segs[l.m].t_base, l.m);
    else if (l.op == BF_OP_RADIUS_SCAN) hipLaunchKernelGGL(k_radius_scan, grid, block, 0, st, A.cnt, A.nq, p.nseg, n_matches);
    else hipLaunchKernelGGL(kernel_of(p), grid, block, 0, st, A);   // BF_OP_KNN_PASS, BF_OP_RADIUS_COUNT, BF_OP_RADIUS_WRITE
}

}  // namespace bf
}  // namespace mi
