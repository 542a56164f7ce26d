/* tools/stereocsbp_ref/cu: in front of oracle/refshim/cudashim on the include path while stereocsbp.cu is compiled for the host.
 * TEST INFRASTRUCTURE.  Adds the one conversion of the main-repo opencv2/core/cuda/saturate_cast.hpp that stereocsbp.cu uses and the
 * shim's stand-in lacks: float -> short is PTX cvt.rni.sat.s16.f32 (round to nearest even, saturate; NaN -> 0). */
#ifndef CSBP_REF_SATURATE_CAST_HPP
#define CSBP_REF_SATURATE_CAST_HPP
#include_next "opencv2/core/cuda/saturate_cast.hpp"
namespace cv { namespace cuda { namespace device {
template <> inline short saturate_cast<short>(float v)
{
    const float r = nearbyintf(v);
    return (short)(r < -32768.f ? -32768 : r > 32767.f ? 32767 : r != r ? 0 : (int)r);
}
}}}
#endif
