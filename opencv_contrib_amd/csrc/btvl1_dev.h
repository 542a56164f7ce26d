// BTV-L1 super-resolution (cv::superres::BTVL1_CUDA, superres/src/btv_l1_cuda.cpp + cuda/btv_l1_gpu.cu): kernel arguments and the
// launch wrappers shared by btvl1_kernels.hip (device side) and btvl1_api.cpp (handle, C-ABI).
//
// One process() is three set-up launches (relative motions, maps, initial estimate) and then TWO launches per iteration whatever
// the number of frames K is: the data kernel (grid over low-res pixels x K) writes sign(src_k - D H M_k X) and the update kernel
// (grid over high-res pixels) forms the BTV term and the K back-projected terms and writes the next estimate.  The estimate is
// double-buffered: every term of iteration i reads X of iteration i - 1, as the reference's do.
#pragma once
#include "mi_common.h"

namespace mi {
namespace btvl1 {

enum { MAX_TAPS = 32, MAX_WEIGHTS = 96 };   // blur kernel length <= 31 (filtering.cpp:441), BTV pairs <= 92 for btvKernelSize 16

// Host-computed tables, passed BY VALUE in the kernel arguments (no __constant__ state: handles stay independent).
struct Tables {
    float g[MAX_TAPS];      // Gaussian taps, getGaussianKernel(blurKernelSize, blurSigma, CV_32F)
    float w[MAX_WEIGHTS];   // BTV weights in the reference's enumeration order (btv_l1_cuda.cpp:180-184)
};

struct Geo {
    int lw, lh;             // low-res size
    int hw, hh;             // high-res size = low-res x scale
    int scale, K, cn;
    unsigned inv_scale;     // ceil(2^32 / scale): v / scale == __umulhi(v, inv_scale) for v < 65536
};

// Scratch planes of the handle's arena.  Positions of the two maps are stored after PointFilter's truncation and BrdReplicate's
// clamp (remap.cu:57-69,256-260) as (row << 16 | column): 4 bytes per map and pixel instead of two floats.
struct Planes {
    const float *src;       // K dense frames, lh x (lw cn)
    const float *mot[4];    // caller's motions, K planes each: forward x, forward y, backward x, backward y
    float *rel[4];          // relative motions to the base frame, K planes each: forward x, y, backward x, y
    unsigned *fidx, *bidx;  // K planes each, hh x hw: forwardMap / backwardMap positions
    float *X[2];            // the estimate, hh x (hw cn), double-buffered
    signed char *sgn;       // K planes, lh x (lw cn): sign(src_k - c_k)
};

struct IterArgs {
    Geo g;
    Planes p;
    Tables t;
    int kb, ks;             // blur kernel length, BTV radius (btvKernelSize - 1) / 2
    int cur;                // index of the estimate this iteration reads
    int use_btv;            // lambda > 0
    int data_lds;           // the data kernel stages the map positions of its taps in LDS (data_lds_bytes() fits DATA_LDS_MAX)
    float beta, tau;        // float(-tau lambda), float(tau)  (add_weighted.cu:91-93)
    unsigned char *dst;     // cropped output, written by the last iteration only (null otherwise)
    size_t dstep;
    int crop;               // btvKernelSize
};

// LDS of the data kernel's staged form: 4 waves x kb rows x (64 scale + kb - 1) packed positions; used where it stays small enough for
// several workgroups per CU (class defaults: 20.8 KB), else the taps read the map from global memory
enum { DATA_LDS_MAX = 40 * 1024 };
static inline size_t data_lds_bytes(int kb, int scale) { return (size_t)4 * kb * (64 * (size_t)scale + kb - 1) * sizeof(unsigned); }

void launch_rel_motions(const Geo &g, const Planes &p, int base_idx, hipStream_t st);
// maps_f (nullable, stage hook only): K x 4 dense hh x hw float planes forwardMap x, y, backwardMap x, y
void launch_maps(const Geo &g, const Planes &p, float *maps_f, hipStream_t st);
void launch_init(const Geo &g, const Planes &p, int base_idx, hipStream_t st);
void launch_data(const IterArgs &A, hipStream_t st);
void launch_update(const IterArgs &A, hipStream_t st);
// depths 0 (CV_8U) / 5 (CV_32F); n = scalars per row
void launch_convert(int sdepth, int ddepth, const void *src, size_t sstep, void *dst, size_t dstep, int rows, int n, hipStream_t st);

}  // namespace btvl1
}  // namespace mi
