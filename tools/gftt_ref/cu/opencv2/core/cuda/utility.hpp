/* tools/gftt_ref/cu: in front of oracle/refshim/cudashim on the include path while the reference's cudaimgproc/src/cuda/gftt.cu is
 * compiled for the host.  TEST INFRASTRUCTURE.  Adds what gftt.cu asks of the main-repo opencv2/core/cuda/utility.hpp and of the CUDA
 * runtime and the shim lacks: the two mask functors, atomicAdd on an int, the allocator thrust's policy is given (nothing is allocated through it here), and
 * the stream-ordered memset / copy / wait of the launch wrappers (everything runs on the calling thread here, so they are plain memset /
 * memcpy / nothing).  No arithmetic of the detector. */
#ifndef GFTT_REF_UTILITY_HPP
#define GFTT_REF_UTILITY_HPP
#include_next "opencv2/core/cuda/utility.hpp"
#include <algorithm>
#include "opencv2/core/cuda/common.hpp"

static inline cudaError_t cudaMemsetAsync(void *p, int v, size_t n, cudaStream_t) { memset(p, v, n); return cudaSuccess; }
static inline cudaError_t cudaMemcpyAsync(void *d, const void *s, size_t n, cudaMemcpyKind, cudaStream_t) { memcpy(d, s, n); return cudaSuccess; }
#ifndef GFTT_REF_HAVE_STREAM_SYNC
#define GFTT_REF_HAVE_STREAM_SYNC
static inline cudaError_t cudaStreamSynchronize(cudaStream_t) { return cudaSuccess; }
#endif
static inline int atomicAdd(int *p, int v) { return __atomic_fetch_add(p, v, __ATOMIC_SEQ_CST); }

namespace cv { namespace cuda { namespace device {
struct SingleMask {   /* main repo: the pixel is taken where the mask is non-zero */
    explicit SingleMask(PtrStepb mask_) : mask(mask_) {}
    bool operator()(int y, int x) const { return mask.ptr(y)[x] != 0; }
    PtrStepb mask;
};
struct WithOutMask {
    bool operator()(int, int) const { return true; }
};
struct ThrustAllocator {   /* main repo: where thrust takes its temporary storage from */
    static ThrustAllocator &getAllocator() { static ThrustAllocator a; return a; }
};
}}}
#endif
