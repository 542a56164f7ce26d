/* oracle/refshim/cudavec: stand-in for the main-repo opencv2/core/cuda/vec_traits.hpp (absent from /root/reference) -- VecTraits / TypeVec
 * for the three pixel types BTV-L1 runs (float, float3, float4).  This directory comes BEFORE oracle/refshim/cudashim on the include
 * path of the BTV-L1 translation units only: the vector-capable versions of the device headers; the scalar ones the other kernels
 * were pinned with stay as they are.  TEST INFRASTRUCTURE. */
#ifndef ORACLE_CUDAVEC_VEC_TRAITS_HPP
#define ORACLE_CUDAVEC_VEC_TRAITS_HPP
#include "opencv2/core/cuda/common.hpp"
namespace cv { namespace cuda { namespace device {
template <typename T> struct VecTraits;
template <> struct VecTraits<float> {
    typedef float elem_type; enum { cn = 1 };
    static float all(float v) { return v; }
    static float make(float x) { return x; }
    static float make(const float *v) { return *v; }
};
template <> struct VecTraits<float3> {
    typedef float elem_type; enum { cn = 3 };
    static float3 all(float v) { return make_float3(v, v, v); }
    static float3 make(float x, float y, float z) { return make_float3(x, y, z); }
    static float3 make(const float *v) { return make_float3(v[0], v[1], v[2]); }
};
template <> struct VecTraits<float4> {
    typedef float elem_type; enum { cn = 4 };
    static float4 all(float v) { return make_float4(v, v, v, v); }
    static float4 make(float x, float y, float z, float w) { return make_float4(x, y, z, w); }
    static float4 make(const float *v) { return make_float4(v[0], v[1], v[2], v[3]); }
};
template <typename T, int CN> struct TypeVec;
template <> struct TypeVec<float, 1> { typedef float vec_type; };
template <> struct TypeVec<float, 3> { typedef float3 vec_type; };
template <> struct TypeVec<float, 4> { typedef float4 vec_type; };
template <> struct TypeVec<float3, 3> { typedef float3 vec_type; };
template <> struct TypeVec<float4, 4> { typedef float4 vec_type; };
}}}
#endif
