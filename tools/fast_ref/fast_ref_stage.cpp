/* tools/fast_ref/fast_ref_stage.cpp -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.
 * C entry points over the two kernel wrappers of the reference's modules/cudafeatures2d/src/cuda/fast.cu (rewritten only at its launch
 * sites by oracle/refshim/cu2host.py and run on the CPU through oracle/refshim/cudashim), each on its own, called the way the host class
 * calls them (modules/cudafeatures2d/src/fast.cpp:134-157).  Matrices arrive dense. */
#include <cstring>
#include "opencv2/core/cuda/common.hpp"
#include "opencv2/core/cuda/utility.hpp"

namespace cv { namespace cuda { namespace device { namespace fast {
int calcKeypoints_gpu(PtrStepSzb img, PtrStepSzb mask, short2 *kpLoc, int maxKeypoints, PtrStepSzi score, int threshold, unsigned int *d_counter,
                      cudaStream_t stream);
int nonmaxSuppression_gpu(const short2 *kpLoc, int count, PtrStepSzi score, short2 *loc, float *response, unsigned int *d_counter,
                          cudaStream_t stream);
}}}}

using namespace cv::cuda;
namespace fd = cv::cuda::device::fast;

extern "C" {
/* img, mask (or null): rows x cols bytes; score (or null, as without suppression): rows x cols ints, CLEARED here as fast.cpp:140 does;
 * kp_loc: max_keypoints x {x, y} shorts.  -> the counter: every candidate, also those beyond max_keypoints */
int fast_ref_calc_keypoints(const unsigned char *img, const unsigned char *mask, int rows, int cols, int threshold, int max_keypoints, int *score,
                            short *kp_loc)
{
    unsigned counter = 0xdeadbeefu;
    if (score) memset(score, 0, (size_t)rows * cols * sizeof(int));
    return fd::calcKeypoints_gpu(PtrStepSzb(rows, cols, (unsigned char *)img, (size_t)cols),
                                 mask ? PtrStepSzb(rows, cols, (unsigned char *)mask, (size_t)cols) : PtrStepSzb(),
                                 (short2 *)kp_loc, max_keypoints, score ? PtrStepSzi(rows, cols, score, (size_t)cols * sizeof(int)) : PtrStepSzi(),
                                 threshold, &counter, 0);
}
/* kp_loc: count locations; loc, response: room for count.  -> the survivors */
int fast_ref_nonmax_suppression(const short *kp_loc, int count, const int *score, int rows, int cols, short *loc, float *response)
{
    unsigned counter = 0xdeadbeefu;
    return fd::nonmaxSuppression_gpu((const short2 *)kp_loc, count, PtrStepSzi(rows, cols, (int *)score, (size_t)cols * sizeof(int)), (short2 *)loc,
                                     response, &counter, 0);
}
}
