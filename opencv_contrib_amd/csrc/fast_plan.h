// The PLAN of FastFeatureDetector (fast_kernels.hip): the validator (the asserts of cudafeatures2d/src/fast.cpp:129-130,213 and this
// library's documented deviations), tile and segment geometry, the degenerate-size rule, the scratch layout and the ordered launch list
// of one frame and of a batch.  fast_api.cpp only EXECUTES the list.  Pure arithmetic, no HIP types.
//
// Per frame the list is fixed: 4 launches with non-maximum suppression, 3 without, whatever the image holds:
//   SCORE  one workgroup per 64 x 16 tile: byte plane (0 = no candidate, else score + 1) and one 64-bit candidate mask per SEGMENT
//          (64 pixels of one row); every segment's mask is written, nothing is accumulated and nothing is cleared first
//   NMS    (only with suppression) one wave per segment: the candidates that beat their eight neighbours' SCORES -> survivor mask
//   SCAN   ONE workgroup: candidate ranks in row-major order, the cut at max_npoints, positions of what is emitted, the two counts
//   EMIT   one wave per segment: short2 locations and float responses into the caller's matrix, row-major
// Order comes from the launch boundaries and the single-workgroup scan; no workgroup waits for another.
#pragma once
#include <cstddef>
#include <vector>
#include "miflow/c_api.h"

namespace mi {
namespace fast {

constexpr int FAST_HALO = 3;            // radius of the Bresenham ring: the border nothing is tested in (fast.cu:217-220)
constexpr int FAST_MIN_SIDE = 2 * FAST_HALO + 1;   // below this no pixel has a whole ring
constexpr int FAST_TILE_W = 64;         // = FAST_SEG: a wave's ballot is one segment's candidate mask
constexpr int FAST_TILE_H = 16;         // 4 waves x 4 rows
constexpr int FAST_SEG = 64;
constexpr int FAST_BLOCK = 256;
constexpr int FAST_SEGS_PER_BLOCK = FAST_BLOCK / 64;   // NMS and EMIT: one wave per segment
constexpr int FAST_SCAN_THREADS = 1024;
constexpr int FAST_MAX_SIDE = 32767;    // locations are short2
constexpr int FAST_FEATURE_SIZE = 7, FAST_ROWS_COUNT = 2, FAST_LOCATION_ROW = 0, FAST_RESPONSE_ROW = 1;   // cudafeatures2d.hpp:419-424
constexpr int FAST_TYPE_9_16 = 2;       // cv::FastFeatureDetector::TYPE_9_16 (main repository, features2d.hpp)
constexpr size_t FAST_ALIGN = 256;

enum FastKernel { FAST_K_SCORE = 0, FAST_K_NMS, FAST_K_SCAN, FAST_K_EMIT };

struct FastErr { int code; const char *msg; };
struct FastMatDesc { int rows, cols, type; size_t step; bool has_data; };
struct FastLaunch { int kernel, frame; unsigned grid_x, grid_y, block; };

struct FastFrame {
    int rows, cols;
    bool degenerate;          // rows < 7 || cols < 7: zero keypoints, no launch
    int tiles_x, tiles_y;     // SCORE grid
    int segs_x;               // segments per row
    int nseg;                 // rows * segs_x, row-major
    int pitch;                // bytes per row of the byte plane
    // byte offsets into the frame area of the scratch
    size_t off_plane, off_cand, off_surv, off_emit, off_pos, area_bytes;
};

struct FastPlan {
    FastErr err;
    int nframes, threshold, nms, max_npoints;
    std::vector<FastFrame> frames;
    size_t counts_bytes;      // 2 ints per frame at the start of the scratch: {candidates, emitted}
    size_t scratch_bytes;     // counts + the largest frame area (frames of a batch run one behind the other on one stream)
    std::vector<FastLaunch> launches;
    int launches_per_frame;   // of a frame that is not degenerate
};

inline size_t fast_align(size_t n) { return (n + FAST_ALIGN - 1) / FAST_ALIGN * FAST_ALIGN; }

// create / set_params.  Deviations from the reference: a negative threshold and max_npoints < 1 are rejected.
inline FastErr fast_check_params(int threshold, int max_npoints)
{
    if (threshold < 0) return {MI_ERR_BAD_ARG, "threshold >= 0 (a negative threshold makes flat regions corners in the reference)"};
    if (max_npoints < 1) return {MI_ERR_BAD_ARG, "max_npoints >= 1"};
    return {MI_OK, nullptr};
}

inline FastErr fast_check_type(int type)
{
    if (type != FAST_TYPE_9_16) return {MI_ERR_BAD_ARG, "type == cv::FastFeatureDetector::TYPE_9_16"};   // fast.cpp:85,213
    return {MI_OK, nullptr};
}

// fast.cpp:129-130 and the deviations.  mask may be null (no mask); a mask without data counts as no mask
inline FastErr fast_check_image(const FastMatDesc &img, const FastMatDesc *mask)
{
    if (img.type != MI_8UC1) return {MI_ERR_BAD_TYPE, "img.type() == CV_8UC1"};
    if (img.rows < 0 || img.cols < 0) return {MI_ERR_BAD_SIZE, "negative image size"};
    if (img.rows > FAST_MAX_SIDE || img.cols > FAST_MAX_SIDE) return {MI_ERR_BAD_SIZE, "rows and cols must fit short2 locations (<= 32767)"};
    const bool degenerate = img.rows < FAST_MIN_SIDE || img.cols < FAST_MIN_SIDE;
    if (!degenerate && !img.has_data) return {MI_ERR_BAD_ARG, "img: null data"};
    if (!degenerate && img.step < (size_t)img.cols) return {MI_ERR_BAD_ARG, "img: step < cols"};
    if (mask && mask->has_data) {
        if (mask->type != MI_8UC1) return {MI_ERR_BAD_TYPE, "mask.type() == CV_8UC1"};
        if (mask->rows != img.rows || mask->cols != img.cols) return {MI_ERR_BAD_SIZE, "mask.size() == img.size()"};
        if (mask->step < (size_t)mask->cols) return {MI_ERR_BAD_ARG, "mask: step < cols"};
    }
    return {MI_OK, nullptr};
}

// the caller's 2 x (>= max_npoints) CV_32FC1 matrix
inline FastErr fast_check_keypoints(const FastMatDesc &kp, int max_npoints)
{
    if (!kp.has_data) return {MI_ERR_BAD_ARG, "keypoints: null data"};
    if (kp.type != MI_32FC1) return {MI_ERR_BAD_TYPE, "keypoints.type() == CV_32FC1"};
    if (kp.rows != FAST_ROWS_COUNT || kp.cols < max_npoints) return {MI_ERR_BAD_SIZE, "keypoints must be 2 x (at least max_npoints)"};
    if (kp.step % 4 != 0 || kp.step < (size_t)kp.cols * 4) return {MI_ERR_BAD_ARG, "keypoints: bad step"};
    return {MI_OK, nullptr};
}

inline FastFrame fast_frame(int rows, int cols, bool nms)
{
    FastFrame f = {};
    f.rows = rows; f.cols = cols;
    f.degenerate = rows < FAST_MIN_SIDE || cols < FAST_MIN_SIDE;
    if (f.degenerate) return f;
    f.tiles_x = (cols + FAST_TILE_W - 1) / FAST_TILE_W;
    f.tiles_y = (rows + FAST_TILE_H - 1) / FAST_TILE_H;
    f.segs_x = (cols + FAST_SEG - 1) / FAST_SEG;
    f.nseg = rows * f.segs_x;
    f.pitch = f.segs_x * FAST_SEG;
    size_t o = 0;
    f.off_plane = o; o += fast_align((size_t)rows * f.pitch);
    f.off_cand = o;  o += fast_align((size_t)f.nseg * 8);
    f.off_surv = o;  if (nms) o += fast_align((size_t)f.nseg * 8);   // without suppression the survivors ARE the candidates
    f.off_emit = o;  o += fast_align((size_t)f.nseg * 8);
    f.off_pos = o;   o += fast_align((size_t)f.nseg * 4);
    f.area_bytes = o;
    return f;
}

// sizes[2 i], sizes[2 i + 1]: rows and cols of frame i (validated by the caller with fast_check_image)
inline FastPlan fast_make_plan(int nframes, const int *sizes, int threshold, int nms, int max_npoints)
{
    FastPlan p = {};
    if ((p.err = fast_check_params(threshold, max_npoints)).code) return p;
    if (nframes < 1 || !sizes) { p.err = {MI_ERR_BAD_ARG, "n >= 1"}; return p; }
    p.nframes = nframes; p.threshold = threshold; p.nms = nms ? 1 : 0; p.max_npoints = max_npoints;
    p.launches_per_frame = p.nms ? 4 : 3;
    p.counts_bytes = fast_align((size_t)nframes * 2 * sizeof(int));
    size_t area = 0;
    for (int i = 0; i < nframes; ++i) {
        const FastFrame f = fast_frame(sizes[2 * i], sizes[2 * i + 1], p.nms != 0);
        p.frames.push_back(f);
        if (f.degenerate) continue;
        if (f.area_bytes > area) area = f.area_bytes;
        const unsigned per_seg = (unsigned)((f.nseg + FAST_SEGS_PER_BLOCK - 1) / FAST_SEGS_PER_BLOCK);
        p.launches.push_back({FAST_K_SCORE, i, (unsigned)f.tiles_x, (unsigned)f.tiles_y, FAST_BLOCK});
        if (p.nms) p.launches.push_back({FAST_K_NMS, i, per_seg, 1, FAST_BLOCK});
        p.launches.push_back({FAST_K_SCAN, i, 1, 1, FAST_SCAN_THREADS});
        p.launches.push_back({FAST_K_EMIT, i, per_seg, 1, FAST_BLOCK});
    }
    p.scratch_bytes = p.counts_bytes + area;
    return p;
}

}  // namespace fast
}  // namespace mi
