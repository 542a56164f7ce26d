/* tools/fast_ref: core/private.cuda.hpp in front of the stub's.  TEST INFRASTRUCTURE.  The stub's BufferPool has getBuffer(Size, type)
 * only; FAST_Impl also asks for getBuffer(rows, cols, type) (fast.cpp:116,134). */
#ifndef FAST_REF_PRIVATE_CUDA_HPP
#define FAST_REF_PRIVATE_CUDA_HPP
#include "opencv2/core/cuda.hpp"
#define BufferPool BufferPoolStub
#include_next "opencv2/core/private.cuda.hpp"
#undef BufferPool
namespace cv { namespace cuda {
class BufferPool {
public:
    explicit BufferPool(Stream &) {}
    GpuMat getBuffer(int rows, int cols, int type) { return GpuMat(rows, cols, type); }
    GpuMat getBuffer(Size s, int type) { return GpuMat(s, type); }
};
}}
#endif
