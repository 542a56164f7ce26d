/*
 * oracle/refshim/cudahost -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.
 *
 * The smallest stand-in for the main-repo headers (opencv/opencv: core.hpp, core/cuda.hpp, core/private.cuda.hpp; absent from
 * /root/reference) that lets the reference's OWN host class of cv::cuda::OpticalFlowDual_TVL1 --
 * modules/cudaoptflow/src/tvl1flow.cpp, compiled VERBATIM from where it lies, against the reference's OWN public header
 * modules/cudaoptflow/include/opencv2/cudaoptflow.hpp -- build and run on the CPU, driving the reference's OWN kernels
 * (modules/cudaoptflow/src/cuda/tvl1flow.cu and the resize_linear template of modules/cudawarping/src/cuda/resize.cu, both already
 * in oracle/_ref/libref_cu.so).  calc / calcImpl / procOneScale -- the pyramid loop, the level sizes and the 16-px rule, the
 * per-warp loop with cv::cuda's sparse convergence schedule, the flow upsampling and its 1 / scaleStep multiplies -- are then
 * REFERENCE code end to end (VERDICT r02 missing #4).  What this stub supplies: GpuMat as host memory, Stream / BufferPool as
 * no-ops, InputArray proxies, and the five cv::cuda functions the file calls (cudahost.cpp: convertTo, setTo, multiply, merge,
 * calcSum, resize -- host glue of cudaarithm / cudawarping / core restated from the cited lines; their kernels are elementwise).
 *
 * The same for cv::cuda::FarnebackOpticalFlow -- modules/cudaoptflow/src/farneback.cpp, verbatim, over the reference's farneback.cu,
 * resize.cu and pyr_down.cu kernels: calc / calcImpl (level cropping, the per-level blur + resize or the pyrDown pyramid, the flow
 * upsampling, prepareGaussian, the iteration loop) are reference code.  Added for it: Event, Stream's bool / waitEvent, Mat_<double>
 * with the Cholesky inverse of a 6 x 6 matrix (main repo core/src/matrix_decomp.cpp CholImpl, restated), getGaussianKernel (main
 * repo imgproc/src/smooth.dispatch.cpp, restated in oracle/imgproc_ref.c), cuda::split / pyrDown.
 *
 * The same for superres' BTVL1_CUDA -- modules/superres/src/btv_l1_cuda.cpp, super_resolution.cpp and frame_source.cpp, verbatim, over
 * cudawarping/src/resize.cpp and remap.cpp (verbatim), the separable-filter slice of cudafilters/src/filtering.cpp and the reference's
 * kernels (btv_l1_gpu.cu, row_filter.hpp / column_filter.hpp, resize.cu, remap.cu, the functors of cudaarithm) on the fiber shim.  Added
 * for it: Point, Scalar_<float>, UMat (a name), DeviceInfo (cc 7.0), streams that are not the null stream, GpuMat::locateROI / reshape /
 * convertTo between CV_8U and CV_32F, InputArray over a Mat, cuda::Filter, cuda::add / addWeighted (element loops over the reference's
 * functors), and the superres glue of oracle/refshim/cudahost/btvl1_host.cpp.
 */
#ifndef ORACLE_CUDAHOST_CORE_CUDA_HPP
#define ORACLE_CUDAHOST_CORE_CUDA_HPP
#include "../../../cudashim/opencv2/core/cuda/common.hpp"   // PtrStepSz / cudaStream_t exactly as the kernels of libref_cu.so were built with
#include <cfloat>
#include <cmath>
#include <limits>
#include <memory>
#include <string>
#include <vector>

#define HAVE_CUDA 1
#define CV_EXPORTS
#define CV_EXPORTS_W
#define CV_WRAP
#define CV_OUT
#define CV_IN_OUT
#define CV_WRAP_AS(x)
#define CV_PROP
#define CV_PROP_RW
#define CV_OVERRIDE override
#define CV_FINAL final
#define CV_Assert(expr) do { if (!(expr)) throw std::runtime_error("CV_Assert failed: " #expr); } while (0)
#define CV_DbgAssert(expr) CV_Assert(expr)
#define CV_8U 0
#define CV_16U 2
#define CV_16S 3
#define CV_32S 4
#define CV_32F 5
#define CV_64F 6
#define CV_MAKETYPE(depth, cn) ((depth) + (((cn) - 1) << 3))
#define CV_8UC1 CV_MAKETYPE(CV_8U, 1)
#define CV_8UC3 CV_MAKETYPE(CV_8U, 3)
#define CV_16UC1 CV_MAKETYPE(CV_16U, 1)
#ifndef CV_16SC1
#define CV_16SC1 CV_MAKETYPE(CV_16S, 1)
#endif
#define CV_32SC1 CV_MAKETYPE(CV_32S, 1)
#define CV_32SC4 CV_MAKETYPE(CV_32S, 4)
#define CV_32FC1 CV_MAKETYPE(CV_32F, 1)
#define CV_32FC2 CV_MAKETYPE(CV_32F, 2)
#define CV_64FC1 CV_MAKETYPE(CV_64F, 1)
#define CV_MAKE_TYPE CV_MAKETYPE
#define CV_MAT_DEPTH(type) ((type) & 7)
#define CV_MAT_CN(type) (((type) >> 3) + 1)
#define CV_8UC4 CV_MAKETYPE(CV_8U, 4)
#define CV_32FC3 CV_MAKETYPE(CV_32F, 3)
#define CV_32FC4 CV_MAKETYPE(CV_32F, 4)
#define CV_INSTRUMENT_REGION()
#define CV_UNUSED(name) (void)name

namespace cv {
typedef std::string String;
enum { INTER_NEAREST = 0, INTER_LINEAR = 1, INTER_CUBIC = 2, INTER_AREA = 3, INTER_LANCZOS4 = 4, WARP_RELATIVE_MAP = 32 };
enum { BORDER_CONSTANT = 0, BORDER_REPLICATE = 1, BORDER_REFLECT = 2, BORDER_WRAP = 3, BORDER_REFLECT101 = 4, BORDER_REFLECT_101 = 4, BORDER_DEFAULT = 4 };
enum { NORM_INF = 1, NORM_L1 = 2, NORM_L2 = 4 };
enum { DECOMP_LU = 0, DECOMP_SVD = 1, DECOMP_EIG = 2, DECOMP_CHOLESKY = 3 };
inline int cvRound(double v) { return (int)lrint(v); }   // round half to even, like the SSE2 path of core/fast_math.hpp
struct Size {
    int width = 0, height = 0;
    Size() {}
    Size(int w, int h) : width(w), height(h) {}
    int area() const { return width * height; }
    bool operator==(const Size &o) const { return width == o.width && height == o.height; }
    bool operator!=(const Size &o) const { return !(*this == o); }
};
struct Point { int x = 0, y = 0; Point() {} Point(int x_, int y_) : x(x_), y(y_) {} };
template <typename T> static inline T saturate_cast(double v);
template <> inline int saturate_cast<int>(double v) { return cvRound(v); }   // core/saturate.hpp
struct Point2f { float x = 0, y = 0; };
struct KeyPoint { Point2f pt; float size = 0, angle = -1, response = 0; int octave = 0, class_id = -1; };   // core/types.hpp
class Mutex { public: void lock() {} void unlock() {} };
class AutoLock { public: explicit AutoLock(Mutex &) {} };
struct Rect { int x = 0, y = 0, width = 0, height = 0; Rect() {} Rect(int x_, int y_, int w, int h) : x(x_), y(y_), width(w), height(h) {} };
struct Scalar {
    double val[4] = {0, 0, 0, 0};
    Scalar() {}
    Scalar(double v0) { val[0] = v0; }
    static Scalar all(double v) { Scalar s; s.val[0] = s.val[1] = s.val[2] = s.val[3] = v; return s; }
    double operator[](int i) const { return val[i]; }
};
template <typename T> struct Scalar_ {   // the float copy of a border value (cudawarping/src/remap.cpp)
    T val[4] = {0, 0, 0, 0};
    Scalar_ &operator=(const Scalar &s) { for (int i = 0; i < 4; ++i) val[i] = (T)s.val[i]; return *this; }
};
template <typename T> using Ptr = std::shared_ptr<T>;
template <typename T, typename... A> Ptr<T> makePtr(A &&...a) { return std::make_shared<T>(std::forward<A>(a)...); }
class Algorithm {
public:
    virtual ~Algorithm() {}
    virtual String getDefaultName() const { return "my_object"; }
};
inline size_t elem_size_of(int type) { const int d = type & 7, cn = (type >> 3) + 1; return (size_t)cn * (d == CV_8U ? 1 : d == CV_16S || d == CV_16U ? 2 : d == CV_64F ? 8 : 4); }

// What a build may set to stand nearer to a device allocator: the pitch of GpuMat rows (cudaMallocPitch on current devices gives
// multiples of 512 bytes; the reference's StereoSGM picks its median kernel by the pitch), and the byte every new GpuMat buffer is
// filled with (device memory is not cleared: running a class with 0x00 and then with 0xFF shows which output it never writes).
#ifndef CUDAHOST_PITCH_ALIGN
#define CUDAHOST_PITCH_ALIGN 256
#endif
inline unsigned char &cudahost_alloc_fill() { static unsigned char v = 0; return v; }

namespace cuda { class GpuMat; }
class Mat {   // a dense host matrix: what diff_sum_host (1 x 1 CV_64F), getGaussianKernel (n x 1 CV_32F) and SURF_CUDA's keypoint /
public:       // descriptor transfers (7 x n CV_32F, n x 64|128 CV_32F over a caller's buffer) need
    int rows = 0, cols = 0;
    size_t step = 0;
    unsigned char *data = nullptr;
    Mat() {}
    Mat(int r, int c, int type) { create(r, c, type); }
    Mat(Size s, int type, void *user) : rows(s.height), cols(s.width), step((size_t)s.width * elem_size_of(type)), data((unsigned char *)user), type_(type) {}
    explicit Mat(const cuda::GpuMat &m);   // downloads (core/src/cuda_gpu_mat... Mat::Mat(const GpuMat&))
    void create(int r, int c, int type)
    {
        rows = r; cols = c; type_ = type; step = (size_t)c * elem_size_of(type);
        buf_ = std::make_shared<std::vector<unsigned char> >((size_t)r * step + 16);
        data = buf_->data();
    }
    int type() const { return type_; }
    int channels() const { return (type_ >> 3) + 1; }
    Size size() const { return Size(cols, rows); }
    bool empty() const { return data == nullptr; }
    // what SeparableLinearFilter's constructor does to a kernel (cudafilters/src/filtering.cpp:427-439): convertTo(CV_32F) of a CV_32F
    // matrix shares it; reshape(1, 1) of a dense n x 1 matrix is the same buffer read as 1 x n
    void convertTo(Mat &dst, int rtype) const { CV_Assert(rtype == (type_ & 7) && rtype == CV_32F); dst = *this; }
    Mat reshape(int cn, int nrows) const
    {
        CV_Assert(cn == channels() && step == (size_t)cols * elem_size_of(type_) && (rows * cols) % nrows == 0);
        Mat m = *this;
        m.rows = nrows; m.cols = rows * cols / nrows; m.step = (size_t)m.cols * elem_size_of(type_);
        return m;
    }
    template <typename T> T &at(int y, int x) { return reinterpret_cast<T *>(data + (size_t)y * step)[x]; }
    template <typename T> T *ptr(int y = 0) { return reinterpret_cast<T *>(data + (size_t)y * step); }
    template <typename T> const T *ptr(int y = 0) const { return reinterpret_cast<const T *>(data + (size_t)y * step); }
private:
    int type_ = CV_8UC1;
    std::shared_ptr<std::vector<unsigned char> > buf_;
};
// Mat_<double>: the 6 x 6 normal matrix of FarnebackOpticalFlowImpl::prepareGaussian and its inverse
template <typename T> class Mat_ {
public:
    int rows = 0, cols = 0;
    std::vector<T> v;
    Mat_() {}
    Mat_(int r, int c) : rows(r), cols(c), v((size_t)r * c) {}
    void setTo(T s) { for (auto &e : v) e = s; }
    T &operator()(int y, int x) { return v[(size_t)y * cols + x]; }
    const T &operator()(int y, int x) const { return v[(size_t)y * cols + x]; }
    // Mat::inv(DECOMP_CHOLESKY) of an n x n matrix, n > 3 (core/src/lapack.cpp cv::invert: dst = I, then hal::Cholesky(src, dst) solves
    // L L^T X = I in place; core/src/matrix_decomp.cpp CholImpl: L stored with RECIPROCAL diagonal, sums accumulated in double)
    Mat_ inv(int method) const
    {
        CV_Assert(method == DECOMP_CHOLESKY && rows == cols);
        const int m = rows;
        Mat_ A = *this, B(m, m);
        B.setTo(0);
        for (int i = 0; i < m; ++i) B(i, i) = 1;
        for (int i = 0; i < m; ++i) {
            for (int j = 0; j < i; ++j) {
                double s = A(i, j);
                for (int k = 0; k < j; ++k) s -= A(i, k) * A(j, k);
                A(i, j) = s * A(j, j);
            }
            double s = A(i, i);
            for (int k = 0; k < i; ++k) { const double t = A(i, k); s -= t * t; }
            if (s < std::numeric_limits<T>::epsilon()) { B.setTo(0); return B; }   // cv::invert returns 0 and zeroes dst
            A(i, i) = 1. / std::sqrt(s);
        }
        for (int i = 0; i < m; ++i)          // L y = b
            for (int j = 0; j < m; ++j) {
                double s = B(i, j);
                for (int k = 0; k < i; ++k) s -= A(i, k) * B(k, j);
                B(i, j) = s * A(i, i);
            }
        for (int i = m - 1; i >= 0; --i)     // L^T x = y
            for (int j = 0; j < m; ++j) {
                double s = B(i, j);
                for (int k = m - 1; k > i; --k) s -= A(k, i) * B(k, j);
                B(i, j) = s * A(i, i);
            }
        return B;
    }
};
// cv::getGaussianKernel(n, sigma, CV_32F) (imgproc.hpp; main repo imgproc/src/smooth.dispatch.cpp): the one restatement of
// oracle/imgproc_ref.c (orc_get_gaussian_kernel)
extern "C" void orc_get_gaussian_kernel(int n, double sigma, float *k);
inline Mat getGaussianKernel(int n, double sigma, int ktype)
{
    CV_Assert(ktype == CV_32F && n > 0);
    Mat k(n, 1, CV_32FC1);
    orc_get_gaussian_kernel(n, sigma, k.ptr<float>(0));
    return k;
}

class UMat {};   // named by superres/src/input_array_utility.hpp; never instantiated with data
namespace cuda {
enum FeatureSet { FEATURE_SET_COMPUTE_10 = 10, FEATURE_SET_COMPUTE_11 = 11, FEATURE_SET_COMPUTE_12 = 12, FEATURE_SET_COMPUTE_13 = 13,
                  FEATURE_SET_COMPUTE_20 = 20 };
inline bool deviceSupports(FeatureSet) { return true; }
// the device the kernels are compiled "for" (oracle/Makefile.ref: -D__CUDA_ARCH__=700): cc >= 20 selects the 32 x 8 / 16 x 16 launch geometry
// of the separable filter (cudafilters/src/cuda/row_filter.hpp:150-161, column_filter.hpp:150-161)
class DeviceInfo {
public:
    int majorVersion() const { return 7; }
    int minorVersion() const { return 0; }
};
class Event;
class Stream {   // every call of this stub runs synchronously on the host: the streams only order work that is already ordered
public:
    Stream() : null_(false) {}   // a stream of one's own is not the null stream: StreamAccessor::getStream is non-zero for it, and the
                                 // reference's launchers take their stream branch (cudawarping/src/cuda/remap.cu:240-243) as in the class
    void waitForCompletion() {}
    void waitEvent(const Event &) {}
    explicit operator bool() const { return !null_; }   // "the default stream": FarnebackOpticalFlowImpl::calcImpl then skips its event plumbing
    static Stream &Null() { static Stream s(true); return s; }
private:
    explicit Stream(bool null) : null_(null) {}
    bool null_;
};
class Event {
public:
    void record(Stream & = Stream::Null()) {}
};
class GpuMat {   // host memory; views share the buffer (like the reference's refcounted device buffers)
public:
    int rows = 0, cols = 0;
    size_t step = 0;
    unsigned char *data = nullptr;
    unsigned char *datastart = nullptr;
    GpuMat() {}
    GpuMat(Size s, int type) { create(s, type); }
    GpuMat(int r, int c, int type) { create(r, c, type); }
    int type() const { return type_; }
    int depth() const { return type_ & 7; }
    int channels() const { return (type_ >> 3) + 1; }
    Size size() const { return Size(cols, rows); }
    bool empty() const { return data == nullptr; }
    void create(int r, int c, int type)   // GpuMat::create: keeps the buffer when size and type match (core/src/cuda/gpu_mat.cu)
    {
        if (data && rows == r && cols == c && type_ == type) return;
        type_ = type; rows = r; cols = c;
        step = ((size_t)c * elem_size_of(type) + CUDAHOST_PITCH_ALIGN - 1) / CUDAHOST_PITCH_ALIGN * CUDAHOST_PITCH_ALIGN;   // a pitched allocation, like cudaMallocPitch
        buf_ = std::make_shared<std::vector<unsigned char> >((size_t)r * step + 64, cudahost_alloc_fill());
        data = datastart = buf_->data();
        whole_ = Size(c, r);
    }
    void create(Size s, int type) { create(s.height, s.width, type); }
    void locateROI(Size &wholeSize, Point &ofs) const   // where this view lies in its allocation
    {
        const size_t d = (size_t)(data - datastart);
        ofs.y = step ? (int)(d / step) : 0;
        ofs.x = (int)((d - (size_t)ofs.y * step) / elem_size_of(type_));
        wholeSize = whole_;
    }
    GpuMat reshape(int cn) const   // the same rows read with another channel count (cols * channels() stays)
    {
        CV_Assert((cols * channels()) % cn == 0);
        GpuMat m = *this;
        m.cols = cols * channels() / cn;
        m.type_ = CV_MAKETYPE(depth(), cn);
        return m;
    }
    GpuMat operator()(const Rect &r) const
    {
        CV_Assert(r.x >= 0 && r.y >= 0 && r.x + r.width <= cols && r.y + r.height <= rows);
        GpuMat m = *this;
        m.data = data + (size_t)r.y * step + (size_t)r.x * elem_size_of(type_);
        m.rows = r.height; m.cols = r.width;
        return m;
    }
    template <typename T> T *ptr(int y = 0) { return reinterpret_cast<T *>(data + (size_t)y * step); }
    template <typename T> const T *ptr(int y = 0) const { return reinterpret_cast<const T *>(data + (size_t)y * step); }
    GpuMat row(int y) const { return (*this)(Rect(0, y, cols, 1)); }
    GpuMat colRange(int a, int b) const { return (*this)(Rect(a, 0, b - a, rows)); }
    void release() { *this = GpuMat(); }
    template <typename T> operator PtrStep<T>() const { return PtrStep<T>((T *)data, step); }
    template <typename T> operator PtrStepSz<T>() const { return PtrStepSz<T>(rows, cols, (T *)data, step); }
    // cudahost.cpp
    void convertTo(GpuMat &dst, int rtype, double alpha, Stream &stream) const;
    void convertTo(GpuMat &dst, int rtype, Stream &stream) const;
    GpuMat &setTo(Scalar s, Stream &stream);
    GpuMat &setTo(Scalar s);                      // any 4-byte-element type (CV_32F / CV_32S, any channel count): s[0] everywhere is all SURF_CUDA asks
    void download(Mat &dst, Stream &stream) const;
    void download(Mat &dst) const;
    void upload(const Mat &src);
    void copyTo(GpuMat &dst, Stream &stream) const;
    void copyTo(GpuMat &dst) const { copyTo(dst, Stream::Null()); }
    void convertTo(GpuMat &dst, int rtype) const;   // CV_8U <-> CV_32F, any channel count (BTVL1_CUDA's frames in, results out)
private:
    int type_ = CV_8UC1;
    Size whole_;
    std::shared_ptr<std::vector<unsigned char> > buf_;
};
inline void swap(GpuMat &a, GpuMat &b) { GpuMat t = a; a = b; b = t; }
// cuda::ensureSizeIsEnough (core/src/cuda/gpu_mat.cu... core/cuda.inl.hpp): keep a buffer that is large enough and take its top-left view
inline void ensureSizeIsEnough(Size s, int type, GpuMat &m)
{
    if (!m.empty() && m.type() == type && m.rows >= s.height && m.cols >= s.width) m = m(Rect(0, 0, s.width, s.height));
    else m.create(s, type);
}
inline void ensureSizeIsEnough(int rows, int cols, int type, GpuMat &m) { ensureSizeIsEnough(Size(cols, rows), type, m); }
}  // namespace cuda
inline Mat::Mat(const cuda::GpuMat &m) { m.download(*this); }

// InputArray / OutputArray proxies over GpuMat (the only kind this translation unit passes)
class _InputArray {
public:
    enum KindFlag { NONE = 0, MAT = 1 << 16, CUDA_GPU_MAT = 9 << 16, UMAT = 10 << 16 };
    _InputArray() : m_(nullptr) {}
    _InputArray(const cuda::GpuMat &m) : m_(const_cast<cuda::GpuMat *>(&m)) {}
    _InputArray(const Mat &m) : m_(nullptr), mat_(&m) {}   // the kernels of a separable filter (cudafilters/src/filtering.cpp:416-419)
    _InputArray(const double &v) : m_(nullptr), scalar_(v), is_scalar_(true) {}   // cuda::min(mask, 1.0, dst) of surf.cuda.cpp:164
    bool isScalar() const { return is_scalar_; }
    double scalar() const { return scalar_; }
    cuda::GpuMat getGpuMat() const { return m_ ? *m_ : cuda::GpuMat(); }
    bool empty() const { return mat_ ? mat_->empty() : (!m_ || m_->empty()); }
    cuda::GpuMat *gpuMatPtr() const { return m_; }
    int kind() const { return m_ ? CUDA_GPU_MAT : mat_ ? MAT : NONE; }
    bool isMat() const { return mat_ != nullptr; }
    bool isUMat() const { return false; }
    Mat getMat() const { return mat_ ? *mat_ : Mat(); }
protected:
    cuda::GpuMat *m_;
    const Mat *mat_ = nullptr;
    double scalar_ = 0;
    bool is_scalar_ = false;
};
class _OutputArray : public _InputArray {
public:
    _OutputArray() {}
    _OutputArray(cuda::GpuMat &m) : _InputArray(m) {}
    void create(Size s, int type) const { CV_Assert(m_); m_->create(s, type); }
    cuda::GpuMat &getGpuMatRef() const { CV_Assert(m_); return *m_; }
    void release() const { if (m_) m_->release(); }
};
typedef const _InputArray &InputArray;
typedef const _OutputArray &OutputArray;
typedef const _OutputArray &InputOutputArray;
typedef InputArray InputArrayOfArrays;
typedef OutputArray OutputArrayOfArrays;
inline const _OutputArray &noArray() { static _OutputArray a; return a; }
}  // namespace cv
#endif
