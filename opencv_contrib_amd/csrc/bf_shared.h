// What the plan (bf_plan.h) and the kernels of both matcher families share: the integer family's limits and the view of the output
// matrices.  No HIP types.
#pragma once

namespace mi {
namespace bfint {

constexpr int T = 64;          // queries per workgroup
constexpr int MAX_D = 128;     // descriptor elements (ORB 32, BRISK / FREAK 64, AKAZE 61)
constexpr int MAX_K = 16;
struct Lists { int *idx; long long istep; int *img; long long mstep; float *dist; long long dstep; };   // n_q x k, element strides; img may be null

}  // namespace bfint
}  // namespace mi
