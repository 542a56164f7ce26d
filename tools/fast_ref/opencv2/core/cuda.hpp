/* tools/fast_ref: in front of oracle/refshim/cudahost on the include path while modules/cudafeatures2d/src/fast.cpp and
 * feature2d_async.cpp are compiled.  TEST INFRASTRUCTURE.  The stub core lacks what FAST_Impl asks of it: cv::KeyPoint's constructor,
 * GpuMat over a caller's memory, colRange, the untyped ptr(), setTo / copyTo / download that do not come from cudahost.cpp (which is not
 * linked), Algorithm::clear / empty, Mat::elemSize, an OutputArray proxy with clear() and a GpuMat& of this class, ensureSizeIsEnough
 * on such a proxy, short2, cudaMalloc / cudaFree and Error::StsNotImplemented.  The stub's header is read with its classes under other names; the classes of those names are defined
 * here on top of them, every member the class calls inline.  Nothing of the detector's arithmetic. */
#ifndef FAST_REF_CORE_CUDA_HPP
#define FAST_REF_CORE_CUDA_HPP
#define GpuMat GpuMatStub
#define Algorithm AlgorithmStub
#define Mat MatStub
#define KeyPoint KeyPointStub
#define _OutputArray _OutputArrayStub
#define OutputArray OutputArrayStub
#define InputOutputArray InputOutputArrayStub
#define OutputArrayOfArrays OutputArrayOfArraysStub
#define noArray noArrayStub
#define ensureSizeIsEnough ensureSizeIsEnoughStub
#include_next "opencv2/core/cuda.hpp"
#undef GpuMat
#undef Algorithm
#undef Mat
#undef KeyPoint
#undef _OutputArray
#undef OutputArray
#undef InputOutputArray
#undef OutputArrayOfArrays
#undef noArray
#undef ensureSizeIsEnough
#include <cstdlib>
#include <cstring>
#include <vector>

#ifndef FAST_REF_SHORT2
#define FAST_REF_SHORT2
struct short2 { short x, y; };
#endif
#ifndef CV_16SC2
#define CV_16SC2 CV_MAKETYPE(CV_16S, 2)
#endif
static inline cudaError_t cudaMalloc(unsigned int **p, size_t n) { *p = (unsigned int *)malloc(n); return cudaSuccess; }
static inline cudaError_t cudaFree(void *p) { free(p); return cudaSuccess; }

namespace cv {
namespace Error { enum { StsNotImplemented = -213 }; }   /* core/base.hpp */
class Algorithm : public AlgorithmStub {   /* core.hpp: the two virtuals cuda::DescriptorMatcher overrides */
public:
    virtual void clear() {}
    virtual bool empty() const { return false; }
};
class Mat : public MatStub {
public:
    Mat() {}
    Mat(const MatStub &m) : MatStub(m) {}
    size_t elemSize() const { return elem_size_of(type()); }
};
class KeyPoint {   /* core/types.hpp */
public:
    KeyPoint() {}
    KeyPoint(float x, float y, float size_, float angle_ = -1, float response_ = 0, int octave_ = 0, int class_id_ = -1)
        : size(size_), angle(angle_), response(response_), octave(octave_), class_id(class_id_) { pt.x = x; pt.y = y; }
    Point2f pt;
    float size = 0, angle = -1, response = 0;
    int octave = 0, class_id = -1;
};
class _OutputArray;
namespace cuda {
class GpuMat : public GpuMatStub {
public:
    GpuMat() {}
    GpuMat(int r, int c, int type) : GpuMatStub(r, c, type) {}
    GpuMat(Size s, int type) : GpuMatStub(s, type) {}
    GpuMat(const GpuMatStub &m) : GpuMatStub(m) {}
    GpuMat(int r, int c, int type, void *user)   /* over the caller's memory, dense */
    {
        GpuMatStub::create(1, 1, type);   /* sets the type; the one-element buffer goes with the reassignment below */
        rows = r; cols = c; step = (size_t)c * elem_size_of(type); data = datastart = (unsigned char *)user;
    }
    size_t elemSize() const { return elem_size_of(type()); }
    using GpuMatStub::ptr;
    unsigned char *ptr(int y = 0) { return data + (size_t)y * step; }
    const unsigned char *ptr(int y = 0) const { return data + (size_t)y * step; }
    GpuMat row(int y) const { return GpuMat(GpuMatStub::row(y)); }
    GpuMat colRange(int a, int b) const
    {
        CV_Assert(0 <= a && a <= b && b <= cols);
        return GpuMat((*this)(Rect(a, 0, b - a, rows)));
    }
    GpuMat &setTo(Scalar s, Stream &)
    {
        CV_Assert(s[0] == 0);
        for (int y = 0; y < rows; ++y) memset(ptr(y), 0, (size_t)cols * elemSize());
        return *this;
    }
    void copyTo(GpuMat &dst, Stream &) const   /* dst has the size and type already (fast.cpp:169-170) */
    {
        CV_Assert(dst.rows == rows && dst.cols == cols && dst.type() == type());
        for (int y = 0; y < rows; ++y) memcpy(dst.ptr(y), ptr(y), (size_t)cols * elemSize());
    }
    void release() { *this = GpuMat(); }
};
}  // namespace cuda
class _OutputArray : public _OutputArrayStub {
public:
    _OutputArray() {}
    _OutputArray(cuda::GpuMat &m) : _OutputArrayStub(m) {}
    cuda::GpuMat &getGpuMatRef() const { CV_Assert(m_); return *static_cast<cuda::GpuMat *>(m_); }
    void clear() const { release(); }
};
typedef const _OutputArray &OutputArray;
typedef const _OutputArray &InputOutputArray;
typedef OutputArray OutputArrayOfArrays;
inline const _OutputArray &noArray() { static _OutputArray a; return a; }
namespace cuda {
/* core/cuda.inl.hpp / core/src/cuda_gpu_mat.cpp: a buffer that is large enough and of the type is kept and its top-left view taken */
inline void ensureSizeIsEnough(int rows, int cols, int type, const _OutputArray &arr)
{
    GpuMat &m = arr.getGpuMatRef();
    if (!m.empty() && m.type() == type && m.rows >= rows && m.cols >= cols) { m.rows = rows; m.cols = cols; }
    else m.create(rows, cols, type);
}
}  // namespace cuda
}  // namespace cv
#endif
