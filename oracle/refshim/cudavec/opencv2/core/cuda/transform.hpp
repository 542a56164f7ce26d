/* oracle/refshim/cudavec: stand-in for the main-repo opencv2/core/cuda/transform.hpp -- device::transform(src1, src2, dst, op, mask,
 * stream) as a plain elementwise loop (the real one picks a block shape from TransformFunctorTraits; the result does not depend on
 * it), and the traits templates btv_l1_gpu.cu:176-183 specialises.  TEST INFRASTRUCTURE. */
#ifndef ORACLE_CUDAVEC_TRANSFORM_HPP
#define ORACLE_CUDAVEC_TRANSFORM_HPP
#include "opencv2/core/cuda/common.hpp"
#include "opencv2/core/cuda/functional.hpp"
namespace cv { namespace cuda { namespace device {
struct WithOutMask {};
template <typename F> struct DefaultTransformFunctorTraits {
    enum { simple_block_dim_x = 16, simple_block_dim_y = 16, smart_block_dim_x = 16, smart_block_dim_y = 16, smart_shift = 4 };
};
template <typename F> struct TransformFunctorTraits : DefaultTransformFunctorTraits<F> {};
template <typename T1, typename T2, typename D, typename Op>
static inline void transform(PtrStepSz<T1> src1, PtrStepSz<T2> src2, PtrStepSz<D> dst, const Op &op, WithOutMask, cudaStream_t)
{
    for (int y = 0; y < dst.rows; ++y)
        for (int x = 0; x < dst.cols; ++x) dst(y, x) = op(src1(y, x), src2(y, x));
}
}}}
#endif
