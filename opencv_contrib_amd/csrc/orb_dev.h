// Internal launch API of the ORB HIP kernels (orb_kernels.hip).  Not part of the C-ABI.
// Geometry (level sizes, capacities, grids) is the plan's (orb_plan.h); these functions launch exactly one kernel each.  The kernels that
// walk keypoints take a device table of levels and read the keypoint counts on the device: grid.y is the level.
#pragma once
#include "mi_common.h"
#include "orb_plan.h"

namespace mi {
namespace orb {

inline int orb_fail(const OrbErr &e) { MI_REQUIRE(e.code == MI_OK, e.code, "%s", e.msg); return MI_OK; }

// one level as the kernels see it.  Keypoint area k (0: FAST's, 1: after the first cull, 2: final) holds counts[1 + k] keypoints:
// loc[k][i] = short2 {x, y} in an int, resp[k][i]
struct OrbLevelDev {
    const unsigned char *img;    // the level's image
    const unsigned char *dimg;   // what the descriptors sample: the blurred image, or img
    int *loc[3];
    float *resp[3];
    unsigned *keys;              // the first cull's / the second cull's order-preserving keys
    float *angle;
    int *counts;                 // {FAST candidates, count of area 0, of area 1, of area 2}
    int pitch, rows, cols, quota;
    float loc_scale, size;
};

struct OrbTaps { float k[7]; };   // getGaussianKernel(7, 2) as f32
struct OrbPlaneSrc { const unsigned char *data; long long step; int rows, cols; };

// resize_linear<uchar> (cudawarping/src/cuda/resize.cu:234-269) of the image and, fused, the level's mask: mask_mode 0 copy / 1 resize /
// 2 resize and THRESH_TOZERO at 254 (orb.cpp:689-708; msrc.data == null: all 255), AND the edge frame (orb.cpp:712-717).
// dmask == null: the image only
int level(const OrbLaunch &k, const OrbPlaneSrc &src, const OrbPlaneSrc &msrc, int mask_mode, float fx, float fy, int edge, unsigned char *dimg,
          long long ipitch, unsigned char *dmask, long long mpitch, int rows, int cols, hipStream_t st);
// one digit's histogram of the keys that are still in the race (cull_gpu's sort, orb.cu:62-89, replaced by a select)
int hist(const OrbLaunch &k, const OrbLevelDev *tab, int *hist, unsigned *state, int ncull, hipStream_t st);
// every keypoint's rank in (response descending, index ascending); the first n are written in that order.  count <= n: copied unchanged
int rank(const OrbLaunch &k, const OrbLevelDev *tab, const int *hist, unsigned *state, int ncull, hipStream_t st);
// HarrisResponses, orb.cu:94-146, on area `area`
int harris(const OrbLaunch &k, const OrbLevelDev *tab, int area, hipStream_t st);
// IC_Angle, orb.cu:173-228, on area 2; m01 / m10 (null: not wanted) receive the moments of level 0's keypoints
int angle(const OrbLaunch &k, const OrbLevelDev *tab, const int *u_max, int half_k, int *m01, int *m10, hipStream_t st);
// the 7 x 7 sigma 2 Gaussian, BORDER_REFLECT_101: row pass 8u -> f32, column pass f32 -> 8u (cudafilters row_filter.hpp, column_filter.hpp)
int blur(const OrbLaunch &k, const unsigned char *src, long long spitch, unsigned char *dst, long long dpitch, int rows, int cols, const OrbTaps &taps,
         hipStream_t st);
// computeOrbDescriptor, orb.cu:250-381, rows offset(level) + i of desc
int descriptors(const OrbLaunch &k, const OrbLevelDev *tab, const int *pattern, int pattern_cols, int wta_k, unsigned char *desc, long long dstep,
                int dcap, hipStream_t st);
// mergeLocation and the row copies and fills of mergeKeyPoints, orb.cu:416-427, orb.cpp:843-865
int merge(const OrbLaunch &k, const OrbLevelDev *tab, unsigned char *kp, long long kstep, int kcap, hipStream_t st);

}  // namespace orb
}  // namespace mi
