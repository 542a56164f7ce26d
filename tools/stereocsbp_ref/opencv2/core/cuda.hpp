/* tools/stereocsbp_ref: in front of oracle/refshim/cudahost on the include path while modules/cudastereo/src/stereocsbp.cpp is compiled.
 * TEST INFRASTRUCTURE.  The stub core lacks what StereoCSBPImpl::compute asks of it: cv::AutoBuffer, GpuMat::rowRange / elemSize, setTo
 * and convertTo on 16-bit matrices, an OutputArray proxy with fixedType / type / create(rows, cols, type), and the type code CV_16SC1.
 * The stub's header is read with its GpuMat and its output proxy under other names; the classes of those names are defined here on top
 * of them, with every member the class calls defined inline (oracle/refshim/cudahost/cudahost.cpp is not linked). */
#ifndef CSBP_REF_CORE_CUDA_HPP
#define CSBP_REF_CORE_CUDA_HPP
#define GpuMat GpuMatStub
#define _OutputArray _OutputArrayStub
#define OutputArray OutputArrayStub
#define InputOutputArray InputOutputArrayStub
#define OutputArrayOfArrays OutputArrayOfArraysStub
#define noArray noArrayStub
#include_next "opencv2/core/cuda.hpp"
#undef GpuMat
#undef _OutputArray
#undef OutputArray
#undef InputOutputArray
#undef OutputArrayOfArrays
#undef noArray
#include <cstring>
#include <vector>
#ifndef CV_16SC1
#define CV_16SC1 CV_MAKETYPE(CV_16S, 1)
#endif
namespace cv {
template <typename T> class AutoBuffer {   // core/utility.hpp: here always on the heap
public:
    explicit AutoBuffer(size_t n) : v_(n) {}
    T *data() { return v_.data(); }
private:
    std::vector<T> v_;
};
class _OutputArray;
namespace cuda {
class GpuMat : public GpuMatStub {
public:
    GpuMat() {}
    GpuMat(int r, int c, int type) : GpuMatStub(r, c, type) {}
    GpuMat(Size s, int type) : GpuMatStub(s, type) {}
    GpuMat(const GpuMatStub &m) : GpuMatStub(m) {}
    // StereoCSBPImpl sizes temp_ by comparing data_cost's cols x rows with step x rows of the coarsest cost volume (stereocsbp.cpp:216-220);
    // where the pitch is much wider than the image (small images) temp_ gets fewer rows than init_message writes (nr_plane2 * h rows of
    // the common step).  Each pixel reads back only what it wrote there, so the result does not depend on it, but the write must land in
    // memory: every allocation here has eight times its rows (the pitch is at most 64 elements wider than the row).
    void create(int r, int c, int type)
    {
        if (data && rows == r && cols == c && this->type() == type) return;
        GpuMatStub::create(r * 8 + 64, c, type);
        rows = r;
    }
    void create(Size s, int type) { create(s.height, s.width, type); }
    size_t elemSize() const { return elem_size_of(type()); }
    GpuMat rowRange(int a, int b) const
    {
        CV_Assert(0 <= a && a <= b && b <= rows);
        GpuMat m = *this;
        m.data = data + (size_t)a * step;
        m.rows = b - a;
        return m;
    }
    GpuMat &setTo(Scalar s, Stream &)
    {
        CV_Assert(s[0] == 0);
        for (int y = 0; y < rows; ++y) memset(ptr<unsigned char>(y), 0, (size_t)cols * elemSize());
        return *this;
    }
    // convertTo of a CV_16SC1 map: saturate_cast<D>(short)
    inline void convertTo(const _OutputArray &dst, int rtype, Stream &) const;
};
}  // namespace cuda
class _OutputArray : public _OutputArrayStub {
public:
    _OutputArray() {}
    _OutputArray(cuda::GpuMat &m, bool fixed_type = false) : _OutputArrayStub(m), fixed_(fixed_type) {}
    bool fixedType() const { return fixed_; }
    int type() const { return m_ ? m_->type() : 0; }
    using _OutputArrayStub::create;
    void create(int rows, int cols, int type) const { CV_Assert(m_); m_->create(rows, cols, type); }
private:
    bool fixed_ = false;
};
typedef const _OutputArray &OutputArray;
typedef const _OutputArray &InputOutputArray;
typedef OutputArray OutputArrayOfArrays;
inline const _OutputArray &noArray() { static _OutputArray a; return a; }
inline void cuda::GpuMat::convertTo(const _OutputArray &dst, int rtype, Stream &) const
{
    CV_Assert(type() == CV_16SC1);
    const int dd = rtype & 7;
    CV_Assert(dd == CV_8U || dd == CV_32S || dd == CV_32F);
    dst.create(rows, cols, CV_MAKETYPE(dd, 1));
    GpuMat out = dst.getGpuMat();
    for (int y = 0; y < rows; ++y) {
        const short *s = ptr<short>(y);
        for (int x = 0; x < cols; ++x) {
            if (dd == CV_8U) out.ptr<unsigned char>(y)[x] = (unsigned char)(s[x] < 0 ? 0 : s[x] > 255 ? 255 : s[x]);
            else if (dd == CV_32S) out.ptr<int>(y)[x] = s[x];
            else out.ptr<float>(y)[x] = (float)s[x];
        }
    }
}
}  // namespace cv
#endif
