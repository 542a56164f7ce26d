/* tools/brox_ref/cu -- TEST INFRASTRUCTURE.  What NCVBroxOpticalFlow.cu and the kernels of NPP_staging.cu need from NCV.hpp,
 * NPP_staging.hpp and the CUDA runtime, for the host: scalar type names, size and rectangle, status codes, the assertion macros (a
 * failed one returns its code), an allocator that answers "initialised, not counting", a vector that owns host memory filled with NaN
 * (device memory is not initialised either: a result that depended on it would not repeat), a matrix view, and the few runtime calls
 * as memcpy / memset.  Written for this recorder: names and signatures are the interface the reference's text compiles against, the
 * bodies are not the reference's. */
#ifndef BROX_REF_NCV_STANDIN_HPP
#define BROX_REF_NCV_STANDIN_HPP
#include <cmath>
#include <cstring>
#include <limits>
#include <memory>
#include <vector>
#include "cudashim.h"

#define CV_EXPORTS
typedef float Ncv32f;
typedef unsigned int Ncv32u;
typedef int Ncv32s;
typedef unsigned char Ncv8u;
typedef int NCVStatus;
enum { NCV_SUCCESS = 0, NCV_INCONSISTENT_INPUT = 1, NCV_CUDA_ERROR = 2, NCV_ALLOCATOR_NOT_INITIALIZED = 3, NCV_ALLOCATOR_BAD_ALLOC = 4, NCV_NULL_PTR = 5,
       NPPST_SUCCESS = 0, NPPST_ERROR = 10, NPPST_CUDA_KERNEL_EXECUTION_ERROR = 11, NPPST_NULL_POINTER_ERROR = 12, NPPST_INVALID_ROI = 13,
       NPPST_INVALID_STEP = 14, NPPST_INVALID_SCALE = 15 };
struct NcvSize32u { Ncv32u width, height; NcvSize32u() : width(0), height(0) {} NcvSize32u(Ncv32u w, Ncv32u h) : width(w), height(h) {} };
struct NcvRect32u { Ncv32u x, y, width, height; NcvRect32u() : x(0), y(0), width(0), height(0) {} NcvRect32u(Ncv32u x_, Ncv32u y_, Ncv32u w, Ncv32u h) : x(x_), y(y_), width(w), height(h) {} };
static inline Ncv32u alignUp(Ncv32u what, Ncv32u alignment) { return (what + alignment - 1) / alignment * alignment; }

#define ncvAssertPrintReturn(pred, msg, err) do { if (!(pred)) return (err); } while (0)
#define ncvAssertReturn(pred, err) do { if (!(pred)) return (err); } while (0)
#define ncvAssertReturnNcvStat(op) do { const NCVStatus s_ = (op); if (s_ != NCV_SUCCESS) return s_; } while (0)
#define ncvAssertCUDAReturn(call, err) do { if ((call) != cudaSuccess) return (err); } while (0)
#define ncvAssertCUDALastErrorReturn(err) do { } while (0)

struct INCVMemAllocator {
    Ncv32u align;
    explicit INCVMemAllocator(Ncv32u a) : align(a) {}
    bool isInitialized() const { return true; }
    bool isCounting() const { return false; }
    Ncv32u alignment() const { return align; }
};
template <class T> class NCVVectorAlloc {
public:
    NCVVectorAlloc(INCVMemAllocator &, Ncv32u n) : v(n, std::numeric_limits<T>::quiet_NaN()) {}
    bool isMemAllocated() const { return true; }
    T *ptr() { return v.data(); }
private:
    std::vector<T> v;
};
template <class T> class NCVMatrix {
public:
    NCVMatrix(T *p, Ncv32u w, Ncv32u h, Ncv32u pitch_bytes) : p_(p), w_(w), h_(h), pitch_(pitch_bytes) {}
    Ncv32u width() const { return w_; }
    Ncv32u height() const { return h_; }
    Ncv32u pitch() const { return pitch_; }
    T *ptr() const { return p_; }
private:
    T *p_; Ncv32u w_, h_, pitch_;
};

struct cudaDeviceProp { size_t textureAlignment; };
static inline cudaError_t cudaGetDevice(int *d) { *d = 0; return cudaSuccess; }
static inline cudaError_t cudaGetDeviceProperties(cudaDeviceProp *p, int) { p->textureAlignment = 512; return cudaSuccess; }
static inline cudaError_t cudaStreamSynchronize(cudaStream_t) { return cudaSuccess; }
static inline cudaError_t cudaMemsetAsync(void *p, int v, size_t n, cudaStream_t) { memset(p, v, n); return cudaSuccess; }
static inline cudaError_t cudaMemcpy2DAsync(void *dst, size_t dpitch, const void *src, size_t spitch, size_t width, size_t height, cudaMemcpyKind,
                                            cudaStream_t)
{
    for (size_t y = 0; y < height; ++y) memcpy((char *)dst + y * dpitch, (const char *)src + y * spitch, width);
    return cudaSuccess;
}
static inline cudaStream_t nppStGetActiveCUDAstream() { return 0; }

enum NppStBorderType { nppStBorderNone = 0, nppStBorderClamp = 1, nppStBorderWrap = 2, nppStBorderMirror = 3 };
enum NppStInterpMode { nppStSupersample, nppStBicubic };
NCVStatus nppiStResize_32f_C1R(Ncv32f *pSrc, NcvSize32u srcSize, Ncv32u nSrcStep, NcvRect32u srcROI, Ncv32f *pDst, NcvSize32u dstSize, Ncv32u nDstStep,
                               NcvRect32u dstROI, Ncv32f xFactor, Ncv32f yFactor, NppStInterpMode interpolation);
NCVStatus nppiStFilterRowBorder_32f_C1R(Ncv32f *pSrc, NcvSize32u srcSize, Ncv32u nSrcStep, Ncv32f *pDst, NcvSize32u dstSize, Ncv32u nDstStep,
                                        NcvRect32u oROI, NppStBorderType borderType, Ncv32f *pKernel, Ncv32s nKernelSize, Ncv32s nAnchor,
                                        Ncv32f multiplier);
NCVStatus nppiStFilterColumnBorder_32f_C1R(Ncv32f *pSrc, NcvSize32u srcSize, Ncv32u nSrcStep, Ncv32f *pDst, NcvSize32u dstSize, Ncv32u nDstStep,
                                           NcvRect32u oROI, NppStBorderType borderType, Ncv32f *pKernel, Ncv32s nKernelSize, Ncv32s nAnchor,
                                           Ncv32f multiplier);

struct NCVBroxOpticalFlowDescriptor {
    Ncv32f alpha, gamma, scale_factor;
    Ncv32u number_of_inner_iterations, number_of_outer_iterations, number_of_solver_iterations;
};
NCVStatus NCVBroxOpticalFlow(const NCVBroxOpticalFlowDescriptor desc, INCVMemAllocator &gpu_mem_allocator, const NCVMatrix<Ncv32f> &frame0,
                             const NCVMatrix<Ncv32f> &frame1, NCVMatrix<Ncv32f> &u, NCVMatrix<Ncv32f> &v, cudaStream_t stream);

// rsqrtf(x) is DEFINED as 1.0f / sqrtf(x), both correctly rounded (the device intrinsic it stands for is within 2 ulp of that)
static inline float rsqrtf(float x) { return 1.0f / sqrtf(x); }
#endif
