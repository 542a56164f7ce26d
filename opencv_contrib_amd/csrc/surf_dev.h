// Internal launch API of the SURF HIP kernels (surf_kernels.hip).  Not part of the C-ABI.
#pragma once
#include "mi_common.h"
#include "surf_plan.h"

namespace mi {
namespace surf {

// The device buffers of a handle, sized by its SurfPlan (surf_plan.h names the element counts).  A view for the kernels: the handle
// owns each region (surf_api.cpp) and fills this from the owners.  counters is the handle's for life; everything else is scratch of the plan.
struct DetectBufs {
    unsigned *sum, *msum;              // integral image of the frame / of the mask (a detect call without a mask is handed msum = nullptr)
    unsigned *V, *BT;                  // scratch of the integral image
    unsigned *poly;                    // polyphase planes (plan.poly)
    float *det, *trace;
    unsigned long long *bits, *sbits;  // sbits: plan.fuse0
    unsigned *rowcnt, *segcnt;
    int4 *cand;
    void *itmp;                        // per-candidate interpolation results
    void *geo;                         // HaarGeo table (plan.fused)
    unsigned *counters;                // 64: [0] = features, [1 + octave] = candidates of the octave (surf.cuda.cpp:158-159), [32 + octave] = accepted candidates
};

// integral image of a CV_8UC1 image into sum ((rows+1) x sld u32); V: rows x vld scratch, BT: integral_bands(rows) x vld scratch
int integral(const unsigned char *img, long long istep, int rows, int cols, bool clamp1, unsigned *V, unsigned *BT, int vld,
             unsigned *sum, int sld, hipStream_t s);
int integral_bands(int rows);
int det_trace(const unsigned *sum, int sld, int rows, int cols, int octave, int nOctaveLayers, float *det, float *trace, int dld,
              hipStream_t s);
// bits: nOctaveLayers*layer_rows*ceil(layer_cols/64) u64; rowcnt: nOctaveLayers*layer_rows + 1 u32; segcnt: layers x rows x row segments
int find_maxima(const float *det, const float *trace, int dld, const unsigned *mask_sum, int sld, int rows, int cols, int octave,
                int nOctaveLayers, float thr, unsigned long long *bits, unsigned *rowcnt, unsigned *segcnt, int4 *cand, int max_candidates,
                unsigned *ncand, hipStream_t s);
// surf.cuda.cpp:182-204 with every stage launched once for all octaves (k_*_all): executes a plan with plan.fused on the buffers the
// handle allocated for it; B.counters zeroed by the caller
int detect_all(const SurfPlan &plan, const DetectBufs &B, float thr, float *kp, int kld, int max_features, hipStream_t s);
// tmp: interp_tmp_bytes(max_candidates) bytes of scratch
int interpolate(const float *det, int dld, int rows, int cols, int octave, const int4 *cand, const unsigned *ncand, int max_candidates,
                void *tmp, float *kp, int kld, int max_features, unsigned *nfeat, hipStream_t s);
size_t interp_tmp_bytes(size_t candidates);
// nfeat_dev != nullptr: count read on the device (grid sized for n_or_max); else n_or_max features
int orientation(const unsigned *sum, int sld, int rows, int cols, float *kp, int kld, const unsigned *nfeat_dev, int n_or_max,
                bool upright, const float *apt /* [3][113] x, y, w */, hipStream_t s);
// nfeat_dev != nullptr: the count is read on the device and nfeat is its upper bound (desc must have that many rows)
int descriptors(const unsigned char *img, long long istep, int rows, int cols, const float *kp, int kld, int nfeat, bool extended,
                float *desc, long long dstep_floats, const float *dw /* [400] */, hipStream_t s, const unsigned *nfeat_dev = nullptr);
int dbg_scan(const unsigned *in_dev, unsigned *out_dev, hipStream_t s);
int dbg_libm(const float *a_dev, const float *b_dev, int n, float *atan2_dev, float *sin_dev, float *cos_dev, hipStream_t s);

}  // namespace surf
}  // namespace mi
