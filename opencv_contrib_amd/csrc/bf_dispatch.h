// Internal: what bf_api.cpp (the executor of bf_plan.h) hands to the two kernel files -- the float kernels' argument struct and one
// launcher per family.  The outputs of both families are bfint::Lists (bf_shared.h).
#pragma once
#include "mi_common.h"
#include "bf_plan.h"
#include "bfint_dev.h"   // Desc, Mask

namespace mi {
namespace bf {

struct Args {
    const float *q; size_t qstep;      // bytes
    const float *t; size_t tstep;
    const unsigned char *mask; size_t mstep;
    int nq, nt, d;
    int rows_per_split;
    int t_base;                        // index of this train set's row 0 in the concatenated collection
    int seg0;                          // first segment (split) of this train set in `part` / `cnt`
    float2 *part;                      // knn: [(seg0 + split) * nq + query][K] = {distance, as_float(collection index)}
    // knn continuation pass (k > K): only candidates after (lo_dist, lo_idx) in (distance, index) order; per-query element strides
    const float *lo_dist; const int *lo_idx; size_t lo_dstep, lo_istep;
    // radius
    int *cnt;                          // [(seg0 + split) * nq + query]: hits of the segment (count pass) / first output slot (write pass)
    float max_dist;
    int write, cols;
    int *r_idx, *r_img; float *r_dist; size_t r_istep, r_mstep, r_dstep;   // element strides per query
};

// launches entry l of a float-family plan: the kernel form is the plan's (row, w, norm, K), grid and block are the entry's
void launch(const BfPlan &p, const BfLaunch &l, const Args &A, const bfint::Lists &o, int *n_matches, hipStream_t st);

}  // namespace bf

namespace bfint {

// launches entry l (BF_OP_INT_KNN / BF_OP_INT_RADIUS) of an integer-family plan on train set l.m
void launch(const bf::BfLaunch &l, const Desc &Q, const Desc &Tr, const Mask &M, int norm, int k, float max_dist, int cols, const Lists &L,
            int *n_matches, hipStream_t st);

}  // namespace bfint
}  // namespace mi
