// Integer-descriptor brute-force matcher: the two kernels and their launcher (see bfint_dev.h for the design and the reference pointers;
// validation and the launch list are bf_plan.h's).
#include "bf_dispatch.h"
#include "bfint_dev.h"

namespace mi {
namespace bfint {

__global__ __launch_bounds__(T) void k_knn(Desc Q, Desc Tr, Mask M, int norm, int k, int image, int first, Lists L)
{
    __shared__ Shared sm;
    knn_block(Q, Tr, M, blockIdx.x * T, norm, k, image, first, L, sm);
}

__global__ __launch_bounds__(T) void k_radius(Desc Q, Desc Tr, Mask M, int norm, float max_dist, int cols, int image, int first, Lists L, int *n_matches)
{
    __shared__ Shared sm;
    radius_block(Q, Tr, M, blockIdx.x * T, norm, max_dist, cols, image, first, L, n_matches, sm);
}

void launch(const bf::BfLaunch &l, const Desc &Q, const Desc &Tr, const Mask &M, int norm, int k, float max_dist, int cols, const Lists &L,
            int *n_matches, hipStream_t st)
{
    const dim3 grid(l.gx, l.gy), block(l.block);
    if (l.op == bf::BF_OP_INT_KNN) hipLaunchKernelGGL(k_knn, grid, block, 0, st, Q, Tr, M, norm, k, l.m, l.m == 0, L);
    else hipLaunchKernelGGL(k_radius, grid, block, 0, st, Q, Tr, M, norm, max_dist, cols, l.m, l.m == 0, L, n_matches);
}

}  // namespace bfint
}  // namespace mi
