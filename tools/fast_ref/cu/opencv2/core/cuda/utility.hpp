/* tools/fast_ref/cu: in front of oracle/refshim/cudashim on the include path while the reference's cudafeatures2d/src/cuda/fast.cu is
 * compiled for the host.  TEST INFRASTRUCTURE.  Adds what fast.cu asks of the main-repo opencv2/core/cuda/utility.hpp and of the CUDA
 * runtime and the shim lacks: the two mask functors, short2, __popc, and the stream-ordered memset / copy / wait of the launch wrappers
 * (everything runs on the calling thread here, so they are plain memset / memcpy / nothing).  No arithmetic of the detector. */
#ifndef FAST_REF_UTILITY_HPP
#define FAST_REF_UTILITY_HPP
#include_next "opencv2/core/cuda/utility.hpp"
#include "opencv2/core/cuda/common.hpp"

struct short2 { short x, y; };
static inline short2 make_short2(short x, short y) { short2 r = {x, y}; return r; }
static inline int __popc(unsigned v) { return __builtin_popcount(v); }
static inline cudaError_t cudaMemsetAsync(void *p, int v, size_t n, cudaStream_t) { memset(p, v, n); return cudaSuccess; }
static inline cudaError_t cudaMemcpyAsync(void *d, const void *s, size_t n, cudaMemcpyKind, cudaStream_t) { memcpy(d, s, n); return cudaSuccess; }
static inline cudaError_t cudaStreamSynchronize(cudaStream_t) { return cudaSuccess; }

namespace cv { namespace cuda { namespace device {
struct SingleMask {   /* main repo: the pixel is taken where the mask is non-zero */
    explicit SingleMask(PtrStepb mask_) : mask(mask_) {}
    bool operator()(int y, int x) const { return mask.ptr(y)[x] != 0; }
    PtrStepb mask;
};
struct WithOutMask {
    bool operator()(int, int) const { return true; }
};
}}}
#endif
