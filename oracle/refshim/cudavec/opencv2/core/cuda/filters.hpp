/* oracle/refshim/cudavec: stand-in for the main-repo opencv2/core/cuda/filters.hpp -- PointFilter (the coordinate truncated toward zero,
 * __float2int_rz) and CubicFilter (Keys a = -0.5; taps cx = ceil(x - 2) .. floor(x + 2), stepped in float; w = c(x - cx) c(y - cy);
 * sum += w src(floor cy, floor cx); result sum / wsum, 0 where wsum == 0 -- the gather the reference spells out in-tree at
 * cudaoptflow/src/cuda/tvl1flow.cu:89-148).  TEST INFRASTRUCTURE. */
#ifndef ORACLE_CUDASHIM_FILTERS_HPP
#define ORACLE_CUDASHIM_FILTERS_HPP
#include "opencv2/core/cuda/saturate_cast.hpp"
#include "opencv2/core/cuda/vec_math.hpp"
namespace cv { namespace cuda { namespace device {
template <typename Ptr2D> struct PointFilter {
    typedef typename Ptr2D::elem_type elem_type;
    typedef float index_type;
    explicit PointFilter(const Ptr2D &src_, float = 0.f, float = 0.f) : src(src_) {}
    elem_type operator()(float y, float x) const { return src(__float2int_rz(y), __float2int_rz(x)); }
    Ptr2D src;
};
template <typename Ptr2D> struct CubicFilter {
    typedef typename Ptr2D::elem_type elem_type;
    typedef float index_type;
    typedef typename TypeVec<float, VecTraits<elem_type>::cn>::vec_type work_type;
    explicit CubicFilter(const Ptr2D &src_, float = 0.f, float = 0.f) : src(src_) {}
    static float bicubicCoeff(float x_)
    {
        const float x = fabsf(x_);
        if (x <= 1.0f) return x * x * (1.5f * x - 2.5f) + 1.0f;
        else if (x < 2.0f) return x * (x * (-0.5f * x + 2.5f) - 4.0f) + 2.0f;
        else return 0.0f;
    }
    elem_type operator()(float y, float x) const
    {
        const float xmin = ::ceilf(x - 2.0f), xmax = ::floorf(x + 2.0f);
        const float ymin = ::ceilf(y - 2.0f), ymax = ::floorf(y + 2.0f);
        work_type sum = VecTraits<work_type>::all(0);
        float wsum = 0.0f;
        for (float cy = ymin; cy <= ymax; cy += 1.0f)
            for (float cx = xmin; cx <= xmax; cx += 1.0f) {
                const float w = bicubicCoeff(x - cx) * bicubicCoeff(y - cy);
                sum = sum + w * src(__float2int_rd(cy), __float2int_rd(cx));
                wsum += w;
            }
        const work_type res = (!wsum) ? VecTraits<work_type>::all(0) : sum / wsum;
        return saturate_cast<elem_type>(res);
    }
    Ptr2D src;
};
}}}
#endif
