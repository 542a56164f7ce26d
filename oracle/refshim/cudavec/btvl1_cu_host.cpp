/*
 * oracle/refshim/cudavec/btvl1_cu_host.cpp -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.
 * The device side of what BTVL1_CUDA (modules/superres/src/btv_l1_cuda.cpp) calls outside its own btv_l1_gpu.cu, run on the CPU
 * through cudashim.h.  Everything #included from oracle/_ref/ below is the reference's text, cut out at build time by cu2host.py
 * (launch sites rewritten, arithmetic untouched):
 *   btvl1_resize.gen.inc  cudawarping/src/cuda/resize.cu: the kernels resize_nearest, resize_linear and the generic resize<Ptr2D, T>,
 *                         with their launch wrappers call_resize_{nearest,linear,cubic}_glob (32 x 8 threads; the cubic one builds
 *                         CubicFilter<BorderReader<PtrStep<T>, BrdReplicate<T>>>);
 *   btvl1_remap.gen.inc   cudawarping/src/cuda/remap.cu: the kernels remap / remap_relative and RemapDispatcherStream;
 *   btvl1_arith.gen.inc   cudaarithm/src/cuda/{add_weighted,mul_scalar,add_mat}.cu: the functors AddWeightedOp, MulScalarOp, AddOp1.
 * Written here, because the reference's versions go through textures (cudev::Texture) or cudev's grid machinery:
 *   device::resize<T>     the table of resize.cu:723-743 reduced to nearest / linear / cubic, each through its _glob wrapper.  The
 *                         reference takes the texture wrapper instead for float / float4 on the null stream (resize.cu:519-616): the
 *                         same filter over a clamping point-sampled texture, i.e. the same arithmetic on the same texels;
 *   imgproc::remap_gpu<T> callers[interpolation][borderMode] of remap.cu:247-280 reduced to PointFilter + BrdReplicate, through
 *                         RemapDispatcherStream (what a non-null stream selects, remap.cu:240-243; BTVL1_CUDA passes its own streams);
 *   the element loops     gridTransformBinary_ / gridTransformUnary_ as `for each element: dst = op(src...)`, the functors
 *                         instantiated with the types the reference's tables select for CV_32F: AddWeightedOp<float, float, float,
 *                         float> (add_weighted.cu:86-93: scalar_type = the largest of T1, T2, D and float), MulScalarOp<float,
 *                         float, float> (mul_scalar.cu:151), AddOp1<float, float> (add_mat.cu funcs[CV_32F][CV_32F]).
 * Stand-ins for main-repo device headers (vec_traits, vec_math, saturate_cast, border_interpolate, filters): oracle/refshim/cudavec; this
 * file lies beside them so that its quoted includes find them before the scalar versions of oracle/refshim/cudashim.
 */
#include "opencv2/core/cuda/common.hpp"
#include "opencv2/core/cuda/vec_traits.hpp"
#include "opencv2/core/cuda/vec_math.hpp"
#include "opencv2/core/cuda/saturate_cast.hpp"
#include "opencv2/core/cuda/border_interpolate.hpp"
#include "opencv2/core/cuda/filters.hpp"
#include "opencv2/core/cuda/functional.hpp"

#include <type_traits>

namespace cv { namespace cuda { namespace device {
// the pixel types libref_cu.so builds; the tables of resize.cpp / remap.cpp name nine more (8- and 16-bit), which throw here
template <typename T> struct is_built : std::integral_constant<bool, std::is_same<T, float>::value || std::is_same<T, float3>::value || std::is_same<T, float4>::value> {};
#define ORACLE_ALL_PIXEL_TYPES(X) X(uchar) X(uchar3) X(uchar4) X(ushort) X(ushort3) X(ushort4) X(short) X(short3) X(short4) X(float) X(float3) X(float4)

#include "btvl1_resize.gen.inc"

template <typename T>
void resize(const PtrStepSzb &src, const PtrStepSzb &, int, int, const PtrStepSzb &dst, float fy, float fx, int interpolation, cudaStream_t stream)
{
    if constexpr (is_built<T>::value) {
        const PtrStepSz<T> s = static_cast<PtrStepSz<T> >(src), d = static_cast<PtrStepSz<T> >(dst);
        if (interpolation == 0) call_resize_nearest_glob(s, d, fy, fx, stream);
        else if (interpolation == 1) call_resize_linear_glob(s, d, fy, fx, stream);
        else if (interpolation == 2) call_resize_cubic_glob(s, d, fy, fx, stream);
        else throw std::runtime_error("device::resize: interpolation not built into libref_cu.so");
    } else
        throw std::runtime_error("device::resize: pixel type not built into libref_cu.so");
}
#define X(T) template void resize<T>(const PtrStepSzb &, const PtrStepSzb &, int, int, const PtrStepSzb &, float, float, int, cudaStream_t);
ORACLE_ALL_PIXEL_TYPES(X)
#undef X

namespace imgproc {

#include "btvl1_remap.gen.inc"

template <typename T>
void remap_gpu(PtrStepSzb src, PtrStepSzb, int, int, PtrStepSzf xmap, PtrStepSzf ymap, PtrStepSzb dst, int interpolation, int borderMode,
               const float *borderValue, cudaStream_t stream, bool cc20, bool isRelative)
{
    if (interpolation != 0 || borderMode != 1 || !is_built<T>::value)
        throw std::runtime_error("remap_gpu: only INTER_NEAREST + BORDER_REPLICATE on CV_32F is built into libref_cu.so");
    if constexpr (is_built<T>::value)
        RemapDispatcherStream<PointFilter, BrdReplicate, T>::call(static_cast<PtrStepSz<T> >(src), xmap, ymap, static_cast<PtrStepSz<T> >(dst), borderValue,
                                                                 stream, cc20, isRelative);
}
#define X(T) template void remap_gpu<T>(PtrStepSzb, PtrStepSzb, int, int, PtrStepSzf, PtrStepSzf, PtrStepSzb, int, int, const float *, cudaStream_t, bool, bool);
ORACLE_ALL_PIXEL_TYPES(X)
#undef X

}  // namespace imgproc
}}}  // namespace cv::cuda::device

namespace arith_host {
using namespace cv::cuda::device;   // unary_function / binary_function / saturate_cast, as `using namespace cv::cudev` gives the reference's files
namespace cudev { using cv::cuda::device::saturate_cast; }

#include "btvl1_arith.gen.inc"
}  // namespace arith_host

extern "C" {
void ref_cu_add_f32(const float *a, const float *b, float *dst, size_t n)
{
    const arith_host::AddOp1<float, float> op;
    for (size_t i = 0; i < n; ++i) dst[i] = op(a[i], b[i]);
}
void ref_cu_add_weighted_f32(const float *a, double alpha, const float *b, double beta, double gamma, float *dst, size_t n)
{
    typedef float scalar_type;   // add_weighted.cu:86-88 for T1 = T2 = D = float
    arith_host::AddWeightedOp<float, float, float, scalar_type> op;
    op.alpha = static_cast<scalar_type>(alpha);
    op.beta = static_cast<scalar_type>(beta);
    op.gamma = static_cast<scalar_type>(gamma);
    for (size_t i = 0; i < n; ++i) dst[i] = op(a[i], b[i]);
}
void ref_cu_mul_scalar_f32(const float *a, double val, float *dst, size_t n)
{
    arith_host::MulScalarOp<float, float, float> op;
    op.val = (float)val;   // mul_scalar.cu:86-89: cv::Scalar_<float> value_ = value
    for (size_t i = 0; i < n; ++i) dst[i] = op(a[i]);
}
}
