/* oracle/refshim/cudavec: stand-in for the main-repo opencv2/core/cuda/vec_math.hpp -- the component-wise operators the BTV-L1 path
 * uses on float3 / float4: vec + vec, vec - vec, vec * scalar, scalar * vec, vec / scalar; each component one separately rounded
 * float operation (the library is built with -ffp-contract=off).  TEST INFRASTRUCTURE. */
#ifndef ORACLE_CUDAVEC_VEC_MATH_HPP
#define ORACLE_CUDAVEC_VEC_MATH_HPP
#include "opencv2/core/cuda/vec_traits.hpp"
namespace cv { namespace cuda { namespace device {
static inline float3 operator+(const float3 &a, const float3 &b) { return make_float3(a.x + b.x, a.y + b.y, a.z + b.z); }
static inline float3 operator-(const float3 &a, const float3 &b) { return make_float3(a.x - b.x, a.y - b.y, a.z - b.z); }
static inline float3 operator*(const float3 &a, float s) { return make_float3(a.x * s, a.y * s, a.z * s); }
static inline float3 operator*(float s, const float3 &b) { return make_float3(s * b.x, s * b.y, s * b.z); }
static inline float3 operator/(const float3 &a, float s) { return make_float3(a.x / s, a.y / s, a.z / s); }
static inline float4 operator+(const float4 &a, const float4 &b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
static inline float4 operator-(const float4 &a, const float4 &b) { return make_float4(a.x - b.x, a.y - b.y, a.z - b.z, a.w - b.w); }
static inline float4 operator*(const float4 &a, float s) { return make_float4(a.x * s, a.y * s, a.z * s, a.w * s); }
static inline float4 operator*(float s, const float4 &b) { return make_float4(s * b.x, s * b.y, s * b.z, s * b.w); }
static inline float4 operator/(const float4 &a, float s) { return make_float4(a.x / s, a.y / s, a.z / s, a.w / s); }
}}}
#endif
