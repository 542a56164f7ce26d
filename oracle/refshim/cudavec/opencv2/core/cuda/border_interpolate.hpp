/* oracle/refshim/cudavec: stand-in for the main-repo opencv2/core/cuda/border_interpolate.hpp (absent from /root/reference), the part
 * the BTV-L1 path touches: the one-dimensional BrdRow* / BrdCol* readers of the separable filter (row_filter.hpp / column_filter.hpp
 * name all five modes in their tables; only Reflect101 runs here -- createGaussianFilter's BORDER_DEFAULT), the two-dimensional
 * BrdReplicate with its reader, and BorderReader.  The index maps are those of oracle/refshim/cudashim's version of this header.
 * TEST INFRASTRUCTURE. */
#ifndef ORACLE_CUDASHIM_BORDER_HPP
#define ORACLE_CUDASHIM_BORDER_HPP
#include "opencv2/core/cuda/common.hpp"
#include "opencv2/core/cuda/saturate_cast.hpp"
#include "opencv2/core/cuda/vec_traits.hpp"
namespace cv { namespace cuda { namespace device {
// ---- one index map per mode; n = the length of the axis
struct IdxReplicate { static int low(int i, int) { return ::max(i, 0); } static int high(int i, int n) { return ::min(i, n - 1); } };
struct IdxReflect101 {
    static int low(int i, int n) { return ::abs(i) % n; }
    static int high(int i, int n) { return ::abs((n - 1) - ::abs((n - 1) - i)) % n; }
};
struct IdxReflect {
    static int low(int i, int n) { return (::abs(i) - (i < 0)) % n; }
    static int high(int i, int n) { return ::abs((n - 1) - ::abs((n - 1) - i) + (i > n - 1)) % n; }
};
struct IdxWrap {
    static int low(int i, int n) { return (i >= 0) * i + (i < 0) * (i - ((i - n + 1) / n) * n); }
    static int high(int i, int n) { return (i < n) * i + (i >= n) * (i % n); }
};
template <typename D, typename M> struct BrdRowBase {
    typedef D result_type;
    explicit BrdRowBase(int width_) : width(width_) {}
    template <typename U> BrdRowBase(int width_, U) : width(width_) {}
    int idx_col_low(int x) const { return M::low(x, width); }
    int idx_col_high(int x) const { return M::high(x, width); }
    int idx_col(int x) const { return idx_col_low(idx_col_high(x)); }
    template <typename T> D at_low(int x, const T *data) const { return saturate_cast<D>(data[idx_col_low(x)]); }
    template <typename T> D at_high(int x, const T *data) const { return saturate_cast<D>(data[idx_col_high(x)]); }
    template <typename T> D at(int x, const T *data) const { return saturate_cast<D>(data[idx_col(x)]); }
    int width;
};
template <typename D, typename M> struct BrdColBase {
    typedef D result_type;
    explicit BrdColBase(int height_) : height(height_) {}
    template <typename U> BrdColBase(int height_, U) : height(height_) {}
    int idx_row_low(int y) const { return M::low(y, height); }
    int idx_row_high(int y) const { return M::high(y, height); }
    int idx_row(int y) const { return idx_row_low(idx_row_high(y)); }
    template <typename T> D at_low(int y, const T *data, size_t step) const { return saturate_cast<D>(*(const T *)((const char *)data + idx_row_low(y) * step)); }
    template <typename T> D at_high(int y, const T *data, size_t step) const { return saturate_cast<D>(*(const T *)((const char *)data + idx_row_high(y) * step)); }
    template <typename T> D at(int y, const T *data, size_t step) const { return saturate_cast<D>(*(const T *)((const char *)data + idx_row(y) * step)); }
    int height;
};
template <typename D> struct BrdRowReplicate : BrdRowBase<D, IdxReplicate> { explicit BrdRowReplicate(int w) : BrdRowBase<D, IdxReplicate>(w) {} };
template <typename D> struct BrdRowReflect101 : BrdRowBase<D, IdxReflect101> { explicit BrdRowReflect101(int w) : BrdRowBase<D, IdxReflect101>(w) {} };
template <typename D> struct BrdRowReflect : BrdRowBase<D, IdxReflect> { explicit BrdRowReflect(int w) : BrdRowBase<D, IdxReflect>(w) {} };
template <typename D> struct BrdRowWrap : BrdRowBase<D, IdxWrap> { explicit BrdRowWrap(int w) : BrdRowBase<D, IdxWrap>(w) {} };
template <typename D> struct BrdColReplicate : BrdColBase<D, IdxReplicate> { explicit BrdColReplicate(int h) : BrdColBase<D, IdxReplicate>(h) {} };
template <typename D> struct BrdColReflect101 : BrdColBase<D, IdxReflect101> { explicit BrdColReflect101(int h) : BrdColBase<D, IdxReflect101>(h) {} };
template <typename D> struct BrdColReflect : BrdColBase<D, IdxReflect> { explicit BrdColReflect(int h) : BrdColBase<D, IdxReflect>(h) {} };
template <typename D> struct BrdColWrap : BrdColBase<D, IdxWrap> { explicit BrdColWrap(int h) : BrdColBase<D, IdxWrap>(h) {} };
template <typename D> struct BrdRowConstant {
    typedef D result_type;
    explicit BrdRowConstant(int width_, const D &val_ = VecTraits<D>::all(0)) : width(width_), val(val_) {}
    template <typename T> D at_low(int x, const T *data) const { return x >= 0 ? saturate_cast<D>(data[x]) : val; }
    template <typename T> D at_high(int x, const T *data) const { return x < width ? saturate_cast<D>(data[x]) : val; }
    template <typename T> D at(int x, const T *data) const { return (x >= 0 && x < width) ? saturate_cast<D>(data[x]) : val; }
    int width;
    D val;
};
template <typename D> struct BrdColConstant {
    typedef D result_type;
    explicit BrdColConstant(int height_, const D &val_ = VecTraits<D>::all(0)) : height(height_), val(val_) {}
    template <typename T> D at_low(int y, const T *data, size_t step) const { return y >= 0 ? saturate_cast<D>(*(const T *)((const char *)data + y * step)) : val; }
    template <typename T> D at_high(int y, const T *data, size_t step) const { return y < height ? saturate_cast<D>(*(const T *)((const char *)data + y * step)) : val; }
    template <typename T> D at(int y, const T *data, size_t step) const { return (y >= 0 && y < height) ? saturate_cast<D>(*(const T *)((const char *)data + y * step)) : val; }
    int height;
    D val;
};
// ---- two-dimensional
template <typename D> struct BrdReplicate {
    typedef D result_type;
    BrdReplicate(int height, int width) : last_row(height - 1), last_col(width - 1) {}
    template <typename U> BrdReplicate(int height, int width, U) : last_row(height - 1), last_col(width - 1) {}
    int idx_row_low(int y) const { return ::max(y, 0); }
    int idx_row_high(int y) const { return ::min(y, last_row); }
    int idx_row(int y) const { return idx_row_low(idx_row_high(y)); }
    int idx_col_low(int x) const { return ::max(x, 0); }
    int idx_col_high(int x) const { return ::min(x, last_col); }
    int idx_col(int x) const { return idx_col_low(idx_col_high(x)); }
    template <typename Ptr2D> D at(int y, int x, const Ptr2D &src) const { return saturate_cast<D>(src(idx_row(y), idx_col(x))); }
    int last_row, last_col;
};
template <typename D> struct BrdReflect101 {
    typedef D result_type;
    BrdReflect101(int height, int width) : last_row(height - 1), last_col(width - 1) {}
    int idx_row_low(int y) const { return ::abs(y) % (last_row + 1); }
    int idx_row_high(int y) const { return ::abs(last_row - ::abs(last_row - y)) % (last_row + 1); }
    int idx_row(int y) const { return idx_row_low(idx_row_high(y)); }
    int idx_col_low(int x) const { return ::abs(x) % (last_col + 1); }
    int idx_col_high(int x) const { return ::abs(last_col - ::abs(last_col - x)) % (last_col + 1); }
    int idx_col(int x) const { return idx_col_low(idx_col_high(x)); }
    int last_row, last_col;
};
template <typename Ptr2D, typename B> struct BorderReader {
    typedef typename B::result_type elem_type;
    typedef typename Ptr2D::index_type index_type;
    BorderReader(const Ptr2D &ptr_, const B &b_) : ptr(ptr_), b(b_) {}
    elem_type operator()(index_type y, index_type x) const { return b.at(y, x, ptr); }
    Ptr2D ptr;
    B b;
};
}}}
#endif
