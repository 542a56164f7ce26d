// The PLAN of CornernessCriteria and CornersDetector (gftt_kernels.hip): the validators (the asserts of cudaimgproc/src/corners.cpp:86-91
// and gftt.cpp:94,114 and this library's documented limits), the launch form of the response, tiles, grids, the scratch layout, the
// capacity of gftt.cpp:122, the ordered launch list and the host loop of gftt.cpp:140-207.  gftt_api.cpp only EXECUTES it.  Pure
// arithmetic, no HIP types.
//
// The list of one detect, whatever the image holds:
//   RESPONSE  FUSED: one workgroup per 64 x 16 tile: source tile -> LDS, Dx / Dy of tile + blockSize halo -> LDS, window sums, response,
//             one maximum per workgroup.  PLANES (blockSize too large for the LDS): DERIV writes Dx / Dy planes, WINDOW reads them.
//   THRESHOLD ONE workgroup: the maximum of the per-workgroup maxima, threshold = (float)((double)max * qualityLevel) on the device
//   FIND      one wave per 64-pixel row SEGMENT: ballot of findCorners' test; one count per workgroup of 64 segments
//   SCAN      ONE workgroup over the per-workgroup counts (1 / 64 of the segments): bases, total, the cut at capacity, the sort's size
//   EMIT      64-bit keys {~ordered(response), linear index} at their row-major rank, the first `capacity` of them
//   SORT      bitonic: SORT_LOCAL sorts 4096-key tiles in LDS; per doubling, SORT_GLOBAL steps down to the tile, SORT_MERGE in LDS.
//             Launched for the capacity, cut on the device by the count: a workgroup beyond the padded count returns at once.
//   POINTS    the head of the sorted keys as float2 {x, y}, and the number written
// No atomics, nothing accumulated, no workgroup waits for another; order comes from launch boundaries.
#pragma once
#include <cmath>
#include <cstddef>
#include <vector>
#include "miflow/c_api.h"

namespace mi {
namespace gftt {

constexpr int GFTT_TILE_W = 64;          // = GFTT_SEG: a wave owns a row of the tile
constexpr int GFTT_TILE_H = 16;          // 4 waves x 4 rows
constexpr int GFTT_BLOCK = 256;
constexpr int GFTT_SEG = 64;
constexpr int GFTT_FIND_SEGS = 64;       // segments per FIND / EMIT workgroup: 4 waves x 16
constexpr int GFTT_SCAN_THREADS = 1024;
constexpr int GFTT_SORT_TILE = 4096;     // keys of one LDS tile (32 KB)
constexpr int GFTT_SORT_THREADS = 512;
constexpr int GFTT_MAX_SIDE = 32767;     // area < 2^30: linear indices, capacities and the padded sort size stay inside int
constexpr int GFTT_MAX_BLOCK_SIZE = 255; // the window sum is blockSize^2 serial adds per pixel
constexpr size_t GFTT_LDS_LIMIT = 65536; // of one workgroup
constexpr size_t GFTT_ALIGN = 256;
constexpr int GFTT_MIN_CAPACITY = 1000;  // gftt.cpp:122
constexpr int GFTT_BORDER_REPLICATE = 1, GFTT_BORDER_REFLECT = 2, GFTT_BORDER_REFLECT101 = 4;   // cv::BorderTypes (main repository)

enum GfttForm { GFTT_FORM_AUTO = 0, GFTT_FORM_FUSED = 1, GFTT_FORM_PLANES = 2 };
enum GfttKernel { GFTT_K_RESPONSE = 0, GFTT_K_DERIV, GFTT_K_WINDOW, GFTT_K_THRESHOLD, GFTT_K_FIND, GFTT_K_SCAN, GFTT_K_EMIT, GFTT_K_SORT_LOCAL,
                  GFTT_K_SORT_GLOBAL, GFTT_K_SORT_MERGE, GFTT_K_POINTS };

struct GfttErr { int code; const char *msg; };
struct GfttMatDesc { int rows, cols, type; size_t step; bool has_data; };
// k: SORT_GLOBAL / SORT_MERGE: the length of the bitonic sequences being merged; j: SORT_GLOBAL: the compare distance
struct GfttLaunch { int kernel; unsigned grid_x, grid_y, block; size_t lds; int k, j; };

struct GfttResponsePlan {
    GfttErr err;
    int rows, cols, block_size, form;
    int lo, hi;                // the window is [p - lo, p + hi], lo = blockSize / 2 (corners.cu:73-76)
    int tiles_x, tiles_y, ntiles;
    int dw, dh, sw, sh;        // FUSED: LDS extents of the Dx / Dy tile and of the source tile
    size_t lds_bytes;
    std::vector<GfttLaunch> launches;
};

struct GfttPlan {
    GfttErr err;
    GfttResponsePlan resp;
    int rows, cols, capacity, sort_cap;
    int segs_x, nseg, nfind;   // segments per row, in all (row-major), FIND workgroups
    // byte offsets into the scratch
    size_t off_resp, off_dx, off_dy, off_wgmax, off_ctl, off_masks, off_bcount, off_bbase, off_keys, off_pts, scratch_bytes;
    std::vector<GfttLaunch> launches;
};

// ints of the control block at off_ctl
enum { GFTT_CTL_THRESHOLD = 0 /* float bits */, GFTT_CTL_FOUND, GFTT_CTL_COUNT, GFTT_CTL_NPAD, GFTT_CTL_NOUT, GFTT_CTL_INTS = 8 };

inline size_t gftt_align(size_t n) { return (n + GFTT_ALIGN - 1) / GFTT_ALIGN * GFTT_ALIGN; }

// corners.cpp:86-91 and the limits.  ksize: only 3, see c_api.h
inline GfttErr gftt_check_corner(int type, int block_size, int ksize, int border)
{
    if (type != MI_8UC1 && type != MI_32FC1) return {MI_ERR_BAD_TYPE, "srcType == CV_8UC1 || srcType == CV_32FC1"};
    if (border != GFTT_BORDER_REFLECT101 && border != GFTT_BORDER_REPLICATE && border != GFTT_BORDER_REFLECT)
        return {MI_ERR_BAD_ARG, "borderType == BORDER_REFLECT101 || borderType == BORDER_REPLICATE || borderType == BORDER_REFLECT"};
    if (block_size < 1 || block_size > GFTT_MAX_BLOCK_SIZE) return {MI_ERR_BAD_ARG, "1 <= blockSize <= 255"};
    if (ksize != 3) return {MI_ERR_NOT_IMPL, "ksize == 3 (the taps of other sizes depend on main-repository code the reference tree lacks)"};
    return {MI_OK, nullptr};
}

// gftt.cpp:94
inline GfttErr gftt_check_params(int max_corners, double quality_level, double min_distance)
{
    if (!(quality_level > 0)) return {MI_ERR_BAD_ARG, "qualityLevel > 0"};
    if (!(min_distance >= 0) || !(min_distance < 1073741824.0)) return {MI_ERR_BAD_ARG, "0 <= minDistance < 2^30"};
    if (max_corners < 0) return {MI_ERR_BAD_ARG, "maxCorners >= 0"};
    return {MI_OK, nullptr};
}

inline GfttErr gftt_check_image(const GfttMatDesc &img, int type, const GfttMatDesc *mask)
{
    if (img.type != type) return {MI_ERR_BAD_TYPE, "src.type() == srcType"};
    if (img.rows < 1 || img.cols < 1) return {MI_ERR_BAD_SIZE, "empty image"};
    if (img.rows > GFTT_MAX_SIDE || img.cols > GFTT_MAX_SIDE) return {MI_ERR_BAD_SIZE, "rows and cols <= 32767 (index and capacity arithmetic)"};
    if (!img.has_data) return {MI_ERR_BAD_ARG, "img: null data"};
    const size_t es = type == MI_8UC1 ? 1 : 4;
    if (img.step < (size_t)img.cols * es || img.step % es != 0) return {MI_ERR_BAD_ARG, "img: bad step"};
    if (mask && mask->has_data) {   // gftt.cpp:114
        if (mask->type != MI_8UC1) return {MI_ERR_BAD_TYPE, "mask.type() == CV_8UC1"};
        if (mask->rows != img.rows || mask->cols != img.cols) return {MI_ERR_BAD_SIZE, "mask.size() == image.size()"};
        if (mask->step < (size_t)mask->cols) return {MI_ERR_BAD_ARG, "mask: step < cols"};
    }
    return {MI_OK, nullptr};
}

inline GfttErr gftt_check_f32(const GfttMatDesc &m, int rows, int cols, const char *what)
{
    if (!m.has_data) return {MI_ERR_BAD_ARG, what};
    if (m.type != MI_32FC1) return {MI_ERR_BAD_TYPE, what};
    if (m.rows != rows || m.cols != cols) return {MI_ERR_BAD_SIZE, what};
    if (m.step % 4 != 0 || m.step < (size_t)m.cols * 4) return {MI_ERR_BAD_ARG, what};
    return {MI_OK, nullptr};
}

// gftt.cpp:122: max(1000, (int)(area * 0.05)); the product in double
inline int gftt_capacity(int rows, int cols)
{
    const int c = (int)((double)((long long)rows * cols) * 0.05);
    return c > GFTT_MIN_CAPACITY ? c : GFTT_MIN_CAPACITY;
}

inline int gftt_pow2_ceil(int n)
{
    int p = 1;
    while (p < n) p <<= 1;
    return p;
}

// columns the caller's 1 x N CV_32FC2 output needs
inline int gftt_output_cols(int rows, int cols, int max_corners)
{
    const int cap = gftt_capacity(rows, cols);
    return max_corners > 0 && max_corners < cap ? max_corners : cap;
}

inline size_t gftt_fused_lds(int block_size)
{
    const size_t dw = GFTT_TILE_W + block_size - 1, dh = GFTT_TILE_H + block_size - 1;
    return ((dw + 2) * (dh + 2) + 2 * dw * dh) * sizeof(float);
}

inline GfttResponsePlan gftt_response_plan(int rows, int cols, int block_size, int form)
{
    GfttResponsePlan p = {};
    if (rows < 1 || cols < 1 || rows > GFTT_MAX_SIDE || cols > GFTT_MAX_SIDE) { p.err = {MI_ERR_BAD_SIZE, "1 <= rows, cols <= 32767"}; return p; }
    if (block_size < 1 || block_size > GFTT_MAX_BLOCK_SIZE) { p.err = {MI_ERR_BAD_ARG, "1 <= blockSize <= 255"}; return p; }
    if (form != GFTT_FORM_AUTO && form != GFTT_FORM_FUSED && form != GFTT_FORM_PLANES) { p.err = {MI_ERR_BAD_ARG, "form: 0, 1 or 2"}; return p; }
    const bool fits = gftt_fused_lds(block_size) <= GFTT_LDS_LIMIT;
    if (form == GFTT_FORM_FUSED && !fits) { p.err = {MI_ERR_BAD_ARG, "the fused form's tile exceeds the LDS at this blockSize"}; return p; }
    p.rows = rows; p.cols = cols; p.block_size = block_size;
    p.form = form != GFTT_FORM_AUTO ? form : fits ? GFTT_FORM_FUSED : GFTT_FORM_PLANES;
    p.lo = block_size / 2; p.hi = block_size - 1 - p.lo;
    p.tiles_x = (cols + GFTT_TILE_W - 1) / GFTT_TILE_W;
    p.tiles_y = (rows + GFTT_TILE_H - 1) / GFTT_TILE_H;
    p.ntiles = p.tiles_x * p.tiles_y;
    const GfttLaunch tile = {GFTT_K_RESPONSE, (unsigned)p.tiles_x, (unsigned)p.tiles_y, GFTT_BLOCK, 0, 0, 0};
    if (p.form == GFTT_FORM_FUSED) {
        p.dw = GFTT_TILE_W + block_size - 1; p.dh = GFTT_TILE_H + block_size - 1;
        p.sw = p.dw + 2; p.sh = p.dh + 2;
        p.lds_bytes = gftt_fused_lds(block_size);
        p.launches.push_back(tile);
        p.launches.back().lds = p.lds_bytes;
    } else {
        p.launches.push_back(tile);
        p.launches.back().kernel = GFTT_K_DERIV;
        p.launches.push_back(tile);
        p.launches.back().kernel = GFTT_K_WINDOW;
    }
    return p;
}

// the launches that sort `sort_cap` (a power of two >= GFTT_SORT_TILE) keys
inline void gftt_sort_launches(int sort_cap, std::vector<GfttLaunch> *out)
{
    const unsigned tiles = (unsigned)(sort_cap / GFTT_SORT_TILE);
    out->push_back({GFTT_K_SORT_LOCAL, tiles, 1, GFTT_SORT_THREADS, 0, 0, 0});
    for (int k = 2 * GFTT_SORT_TILE; k <= sort_cap && k > 0; k <<= 1) {
        for (int j = k / 2; j >= GFTT_SORT_TILE; j >>= 1)
            out->push_back({GFTT_K_SORT_GLOBAL, (unsigned)(sort_cap / 2 / GFTT_SORT_THREADS), 1, GFTT_SORT_THREADS, 0, k, j});
        out->push_back({GFTT_K_SORT_MERGE, tiles, 1, GFTT_SORT_THREADS, 0, k, 0});
    }
}

inline GfttPlan gftt_make_plan(int rows, int cols, int block_size, int form)
{
    GfttPlan p = {};
    p.resp = gftt_response_plan(rows, cols, block_size, form);
    if ((p.err = p.resp.err).code) return p;
    p.rows = rows; p.cols = cols;
    p.capacity = gftt_capacity(rows, cols);
    p.sort_cap = gftt_pow2_ceil(p.capacity > GFTT_SORT_TILE ? p.capacity : GFTT_SORT_TILE);
    p.segs_x = (cols + GFTT_SEG - 1) / GFTT_SEG;
    p.nseg = rows * p.segs_x;
    p.nfind = (p.nseg + GFTT_FIND_SEGS - 1) / GFTT_FIND_SEGS;
    size_t o = 0;
    const size_t plane = gftt_align((size_t)rows * cols * sizeof(float));
    p.off_resp = o;   o += plane;
    p.off_dx = o;     if (p.resp.form == GFTT_FORM_PLANES) o += plane;
    p.off_dy = o;     if (p.resp.form == GFTT_FORM_PLANES) o += plane;
    p.off_wgmax = o;  o += gftt_align((size_t)p.resp.ntiles * sizeof(float));
    p.off_ctl = o;    o += gftt_align(GFTT_CTL_INTS * sizeof(int));
    p.off_masks = o;  o += gftt_align((size_t)p.nseg * 8);
    p.off_bcount = o; o += gftt_align((size_t)p.nfind * sizeof(int));
    p.off_bbase = o;  o += gftt_align((size_t)p.nfind * sizeof(int));
    p.off_keys = o;   o += gftt_align((size_t)p.sort_cap * 8);
    p.off_pts = o;    o += gftt_align((size_t)p.capacity * 8);
    p.scratch_bytes = o;
    p.launches = p.resp.launches;
    p.launches.push_back({GFTT_K_THRESHOLD, 1, 1, GFTT_SCAN_THREADS, 0, 0, 0});
    p.launches.push_back({GFTT_K_FIND, (unsigned)p.nfind, 1, GFTT_BLOCK, 0, 0, 0});
    p.launches.push_back({GFTT_K_SCAN, 1, 1, GFTT_SCAN_THREADS, 0, 0, 0});
    p.launches.push_back({GFTT_K_EMIT, (unsigned)p.nfind, 1, GFTT_BLOCK, 0, 0, 0});
    gftt_sort_launches(p.sort_cap, &p.launches);
    p.launches.push_back({GFTT_K_POINTS, (unsigned)((p.capacity + GFTT_BLOCK - 1) / GFTT_BLOCK), 1, GFTT_BLOCK, 0, 0, 0});
    return p;
}

// cvRound of the main repository: to nearest, ties to even
inline int gftt_cv_round(double v) { return (int)std::nearbyint(v); }

// The host loop of gftt.cpp:140-207 for minDistance >= 1.  pts: `total` float2 {x, y}, sorted; out: the survivors in order.
inline void gftt_min_distance(const float *pts, int total, int rows, int cols, double min_distance, int max_corners, std::vector<float> *out)
{
    out->clear();
    const int cell_size = gftt_cv_round(min_distance);
    const int grid_width = (cols + cell_size - 1) / cell_size;
    const int grid_height = (rows + cell_size - 1) / cell_size;
    std::vector<std::vector<int>> grid((size_t)grid_width * grid_height);   // indices into pts
    size_t kept = 0;
    for (int i = 0; i < total; ++i) {
        const float px = pts[2 * i], py = pts[2 * i + 1];
        bool good = true;
        const int x_cell = (int)(px / cell_size), y_cell = (int)(py / cell_size);
        if (x_cell < 0 || x_cell >= grid_width || y_cell < 0 || y_cell >= grid_height) continue;   // no corner of an image is here
        const int x1 = x_cell - 1 > 0 ? x_cell - 1 : 0, y1 = y_cell - 1 > 0 ? y_cell - 1 : 0;
        const int x2 = x_cell + 1 < grid_width - 1 ? x_cell + 1 : grid_width - 1, y2 = y_cell + 1 < grid_height - 1 ? y_cell + 1 : grid_height - 1;
        for (int yy = y1; yy <= y2 && good; ++yy)
            for (int xx = x1; xx <= x2 && good; ++xx)
                for (const int j : grid[(size_t)yy * grid_width + xx]) {
                    const float dx = px - pts[2 * j], dy = py - pts[2 * j + 1];
                    const float d2 = dx * dx + dy * dy;   // float, compared in double (gftt.cpp:186)
                    if ((double)d2 < min_distance * min_distance) { good = false; break; }
                }
        if (!good) continue;
        grid[(size_t)y_cell * grid_width + x_cell].push_back(i);
        out->push_back(px); out->push_back(py);
        if (max_corners > 0 && ++kept == (size_t)max_corners) break;
    }
}

}  // namespace gftt
}  // namespace mi
