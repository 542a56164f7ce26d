/* tools/brox_ref/cu -- TEST INFRASTRUCTURE.  Shadows oracle/refshim/cudashim/opencv2/core/cuda/utility.hpp for the Brox recorder: the
 * one name NCVBroxOpticalFlow.cu takes from the main repository's header.  Written for this recorder. */
#ifndef BROX_REF_UTILITY_HPP
#define BROX_REF_UTILITY_HPP
namespace cv { namespace cuda { namespace device {
template <typename T> static inline void swap(T &a, T &b) { const T t = a; a = b; b = t; }
}}}
#endif
