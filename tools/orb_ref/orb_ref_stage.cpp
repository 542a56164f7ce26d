/* tools/orb_ref/orb_ref_stage.cpp -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.
 * C entry points over the kernel wrappers of the reference's modules/cudafeatures2d/src/cuda/orb.cu (rewritten only at its launch sites by
 * oracle/refshim/cu2host.py and run on the CPU through oracle/refshim/cudashim), each on its own, called the way the host class calls
 * them (modules/cudafeatures2d/src/orb.cpp:735,773,780,818,856).  Matrices arrive dense.  The shim's reduce wants every thread of a block
 * in it, and the kernels guard it with ptidx < npoints: callers pass npoints as a multiple of 8 (blockDim.y). */
#include "opencv2/core/cuda/common.hpp"
#include "opencv2/core/cuda/reduce.hpp"

namespace cv { namespace cuda { namespace device { namespace orb {
int cull_gpu(int *loc, float *response, int size, int n_points, cudaStream_t stream);
void HarrisResponses_gpu(PtrStepSzb img, const short2 *loc, float *response, const int npoints, int blockSize, float harris_k, cudaStream_t stream);
void loadUMax(const int *u_max, int count);
void IC_Angle_gpu(PtrStepSzb image, const short2 *loc, float *angle, int npoints, int half_k, cudaStream_t stream);
void computeOrbDescriptor_gpu(PtrStepb img, const short2 *loc, const float *angle, const int npoints, const int *pattern_x, const int *pattern_y,
                              PtrStepb desc, int dsize, int WTA_K, cudaStream_t stream);
void mergeLocation_gpu(const short2 *loc, float *x, float *y, int npoints, float scale, cudaStream_t stream);
}}}}

using namespace cv::cuda;
namespace od = cv::cuda::device::orb;

extern "C" {
int orb_ref_cull(int *loc, float *response, int size, int n_points) { return od::cull_gpu(loc, response, size, n_points, 0); }
void orb_ref_harris(const unsigned char *img, int rows, int cols, const short *loc, float *response, int npoints)
{
    od::HarrisResponses_gpu(PtrStepSzb(rows, cols, (unsigned char *)img, (size_t)cols), (const short2 *)loc, response, npoints, 7, 0.04f, 0);
}
void orb_ref_angle(const unsigned char *img, int rows, int cols, const short *loc, float *angle, int npoints, const int *u_max, int n_u_max, int half_k)
{
    od::loadUMax(u_max, n_u_max);
    od::IC_Angle_gpu(PtrStepSzb(rows, cols, (unsigned char *)img, (size_t)cols), (const short2 *)loc, angle, npoints, half_k, 0);
}
void orb_ref_descriptors(const unsigned char *img, int rows, int cols, const short *loc, const float *angle, int npoints, const int *pattern, int pattern_cols,
                         int wta_k, unsigned char *desc)
{
    od::computeOrbDescriptor_gpu(PtrStepb((unsigned char *)img, (size_t)cols), (const short2 *)loc, angle, npoints, pattern, pattern + pattern_cols,
                                 PtrStepb(desc, 32), 32, wta_k, 0);
}
void orb_ref_merge(const short *loc, float *x, float *y, int npoints, float scale) { od::mergeLocation_gpu((const short2 *)loc, x, y, npoints, scale, 0); }
}
