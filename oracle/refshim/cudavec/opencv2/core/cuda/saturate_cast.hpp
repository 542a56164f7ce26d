/* oracle/refshim/cudavec: stand-in for the main-repo opencv2/core/cuda/saturate_cast.hpp + the vector overloads of vec_math.hpp -- between
 * equal float types (all the BTV-L1 path asks for) the identity.  TEST INFRASTRUCTURE. */
#ifndef ORACLE_CUDASHIM_SATURATE_CAST_HPP
#define ORACLE_CUDASHIM_SATURATE_CAST_HPP
#include "opencv2/core/cuda/vec_traits.hpp"
namespace cv { namespace cuda { namespace device {
template <typename T> static inline T saturate_cast(float v);
template <typename T> static inline T saturate_cast(const float3 &v);
template <typename T> static inline T saturate_cast(const float4 &v);
template <> inline float saturate_cast<float>(float v) { return v; }
template <> inline float3 saturate_cast<float3>(const float3 &v) { return v; }
template <> inline float4 saturate_cast<float4>(const float4 &v) { return v; }
}}}
#endif
