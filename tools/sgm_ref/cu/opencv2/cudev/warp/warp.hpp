/* tools/sgm_ref/cu: cv::cudev::Warp of the main repo's opencv2/cudev/warp/warp.hpp: a thread's warp within its block and its lane within
 * the warp, by the thread's linear index (the fibers of oracle/refshim/cudashim run in that order).  TEST INFRASTRUCTURE. */
#ifndef SGM_REF_CUDEV_WARP_HPP
#define SGM_REF_CUDEV_WARP_HPP
#include "opencv2/cudev/common.hpp"
namespace cv { namespace cudev {
struct Warp {
    static inline unsigned warpId() { return cudashim::linear_tid() >> LOG_WARP_SIZE; }
    static inline unsigned laneId() { return cudashim::linear_tid() & (WARP_SIZE - 1); }
};
}}
#endif
