/* tools/gftt_ref/cu: in front of oracle/refshim/cudavec on the include path while the reference's 8-bit row filter is compiled for the
 * host.  TEST INFRASTRUCTURE.  Adds saturate_cast<uchar>(float) of the main-repo saturate_cast.hpp (cvt.rni.sat.u8.f32: round to nearest
 * even, saturate), spelled as oracle/refshim/cudashim/warping_cu_host.cpp spells it.  The border readers of a uchar row name it; the
 * values they pass are bytes, which it returns unchanged. */
#ifndef GFTT_REF_SATURATE_CAST_HPP
#define GFTT_REF_SATURATE_CAST_HPP
#include_next "opencv2/core/cuda/saturate_cast.hpp"
#include <cmath>
namespace cv { namespace cuda { namespace device {
template <> inline unsigned char saturate_cast<unsigned char>(float v)
{
    const float r = nearbyintf(v);
    return (unsigned char)(r < 0.f ? 0 : r > 255.f ? 255 : (int)r);
}
}}}
#endif
