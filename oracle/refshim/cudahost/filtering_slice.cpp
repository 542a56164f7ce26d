/*
 * oracle/refshim/cudahost/filtering_slice.cpp -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.
 * cuda::createGaussianFilter and cuda::createSeparableLinearFilter with the class SeparableLinearFilter, as modules/cudafilters/src/
 * filtering.cpp writes them: oracle/Makefile.ref cuts three line ranges out of that file (cu2host.py --slice: normalizeAnchor; "Separable
 * Linear Filter" up to "Deriv Filter"; "Gaussian Filter" up to "Morphology Filter") into oracle/_ref/, and they are #included below,
 * verbatim.  The rest of filtering.cpp (box, Laplacian, morphology, rank and median filters) calls NPP and is left out.
 * Written here: the fallback body of filter::linearRow / linearColumn for the pixel types the class's tables name but libref_cu.so
 * does not build (it throws); CV_32FC1 / C3 / C4 are the reference's row_filter.32fc{1,3,4}.cu and column_filter.32fc{1,3,4}.cu.
 */
#include <cfloat>
#include <limits>
#include "opencv2/cudafilters.hpp"
#include "opencv2/cudaarithm.hpp"
#include "opencv2/imgproc.hpp"
#include "opencv2/core/private.cuda.hpp"

using namespace cv;
using namespace cv::cuda;

namespace filter {
template <typename T, typename D>
void linearRow(PtrStepSzb, PtrStepSzb, const float *, int, int, int, int, cudaStream_t) { throw std::runtime_error("linearRow: pixel type not built into libref_cu.so"); }
template <typename T, typename D>
void linearColumn(PtrStepSzb, PtrStepSzb, const float *, int, int, int, int, cudaStream_t) { throw std::runtime_error("linearColumn: pixel type not built into libref_cu.so"); }
#define ORACLE_FILTER_BUILT(T) \
    extern template void linearRow<T, T>(PtrStepSzb, PtrStepSzb, const float *, int, int, int, int, cudaStream_t); \
    extern template void linearColumn<T, T>(PtrStepSzb, PtrStepSzb, const float *, int, int, int, int, cudaStream_t);
ORACLE_FILTER_BUILT(float)
ORACLE_FILTER_BUILT(float3)
ORACLE_FILTER_BUILT(float4)
}

namespace {
#include "filtering_anchor.gen.inc"
}
#include "filtering_sep.gen.inc"
