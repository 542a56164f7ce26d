/* tools/sgm_ref/cu: of the main repo's opencv2/cudev/common.hpp what modules/cudastereo/src/cuda/stereosgm.cu uses: the warp size, divUp,
 * the error check of a launch, the stream accessor and the error code of its depth switches.  TEST INFRASTRUCTURE. */
#ifndef SGM_REF_CUDEV_COMMON_HPP
#define SGM_REF_CUDEV_COMMON_HPP
#include <array>
#include "opencv2/core/cuda.hpp"
#include "opencv2/core/private.cuda.hpp"
#define CV_CUDEV_SAFE_CALL(expr) ((void)(expr))
namespace cv {
namespace Error { enum { BadDepth = -17 }; }
namespace cudev {
enum { LOG_WARP_SIZE = 5, WARP_SIZE = 1 << LOG_WARP_SIZE };
static inline int divUp(int total, int grain) { return (total + grain - 1) / grain; }
}}
#endif
