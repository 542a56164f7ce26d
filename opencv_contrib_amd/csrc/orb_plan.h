// The PLAN of cv::cuda::ORB (orb_kernels.hip): the validator (the asserts of cudafeatures2d/src/orb.cpp:500-501,535,666-667 and this
// library's documented deviations), cv::RNG and the two pattern generators (orb.cpp:431-477), n_features_per_level (:506-517), u_max
// (:519-534), level sizes and resize factors (:674-676, cudawarping/src/resize.cpp:82-105), the reach R of the reads around a keypoint,
// per-level capacities, the scratch layout and the ordered launch list.  orb_api.cpp only EXECUTES the list.  Pure arithmetic, no HIP types.
//
// One detectAndCompute is, for L levels (FAST's own list per level is fast_plan.h's):
//   CLEAR     one memset of the counts and histograms
//   LEVEL     per level: image (resize_linear's arithmetic) and mask (resize, THRESH_TOZERO at 254, AND with the border frame) in one launch
//   FAST      per level: SCORE, NMS, SCAN, EMIT of fast_plan.h with max_npoints = int(0.05 * area), into the level's keypoint area A
//   CULL      once with FAST_SCORE, twice with HARRIS_SCORE, ALL LEVELS in each launch: four digit histograms of the order-preserving
//             key (integer adds: the sums do not depend on arrival order), then RANK: every candidate that can still be kept counts the
//             candidates in front of it in the total order (response descending, index ascending) and writes itself to that slot
//   HARRIS, ANGLE, BLUR (per level), DESCRIPTORS, MERGE
// and ONE read-back of the per-level counts at the end.  Grids are sized by capacities; the kernels read the counts on the device.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>
#include "miflow/c_api.h"
#include "fast_plan.h"

namespace mi {
namespace orb {

constexpr int ORB_NPOINTS = 512;          // the pool of test points, orb.cpp:539
constexpr int ORB_DESC_BYTES = 32;        // cv::ORB::kBytes
constexpr int ORB_ROWS_COUNT = 6;         // X, Y, RESPONSE, ANGLE, OCTAVE, SIZE (cudafeatures2d.hpp:455-461)
constexpr int ORB_HARRIS_SCORE = 0, ORB_FAST_SCORE = 1;   // cv::ORB (main repository, features2d.hpp)
constexpr int ORB_HARRIS_BLOCK = 7;       // orb.cpp:773
constexpr int ORB_BLOCK = 256;
constexpr int ORB_KP_PER_BLOCK = ORB_BLOCK / 64;   // HARRIS, ANGLE, DESCRIPTORS: one wave per keypoint
constexpr int ORB_MAX_LEVELS = 32;
constexpr int ORB_UMAX_N = 32;            // orb.cpp:535: u_max.size() < 32
constexpr int ORB_DIGITS = 4, ORB_BINS = 256;      // the key's radix
constexpr int ORB_BLUR_TILE = 16;         // 16 x 16 pixels per workgroup
constexpr size_t ORB_ALIGN = 256;
constexpr size_t ORB_LEVEL_DEV_BYTES = 128;   // room for one level of the device table (orb_dev.h asserts it)

enum OrbKernel { ORB_K_CLEAR = 0, ORB_K_LEVEL, ORB_K_FAST, ORB_K_HIST, ORB_K_RANK, ORB_K_HARRIS, ORB_K_ANGLE, ORB_K_BLUR, ORB_K_DESC, ORB_K_MERGE,
                 ORB_K_READBACK };

struct OrbErr { int code; const char *msg; };
struct OrbLaunch { int kernel, level, arg; unsigned grid_x, grid_y, block; };   // arg: HIST digit / which cull / FAST's launch index

inline int cv_round(double v) { return (int)std::nearbyint(v); }   // cvRound: round half to even (the default rounding mode)
inline size_t orb_align(size_t n) { return (n + ORB_ALIGN - 1) / ORB_ALIGN * ORB_ALIGN; }

// cv::RNG (main repository, core.hpp): multiply-with-carry; uniform(int a, int b) = a + next() % (b - a)
struct OrbRng {
    uint64_t state;
    explicit OrbRng(uint64_t s) : state(s ? s : 0xffffffffull) {}
    unsigned next() { state = (uint64_t)(unsigned)state * 4164903690u + (unsigned)(state >> 32); return (unsigned)state; }
    int uniform(int a, int b) { return a == b ? a : (int)(next() % (unsigned)(b - a) + (unsigned)a); }
};

// makeRandomPattern, orb.cpp:466-477: pool[2 i], pool[2 i + 1] = x, y of point i
inline void orb_random_pool(int patch_size, int *pool)
{
    OrbRng rng(0x34985739);
    for (int i = 0; i < ORB_NPOINTS; ++i) {
        pool[2 * i] = rng.uniform(-patch_size / 2, patch_size / 2 + 1);
        pool[2 * i + 1] = rng.uniform(-patch_size / 2, patch_size / 2 + 1);
    }
}

inline int orb_pattern_cols(int wta_k) { return wta_k == 2 ? ORB_NPOINTS : ORB_DESC_BYTES * 4 * wta_k; }

// The 2 x N matrix the reference uploads (orb.cpp:548-568): out[0 .. N) = x, out[N .. 2 N) = y.  pool0 == null: the random pool.
inline void orb_make_pattern(int patch_size, int wta_k, const int *pool0, int *out)
{
    int pool_buf[2 * ORB_NPOINTS];
    if (!pool0) { orb_random_pool(patch_size, pool_buf); pool0 = pool_buf; }
    const int n = orb_pattern_cols(wta_k);
    int *px = out, *py = out + n;
    if (wta_k == 2) {
        for (int i = 0; i < n; ++i) { px[i] = pool0[2 * i]; py[i] = pool0[2 * i + 1]; }
        return;
    }
    // initializeOrbPattern, orb.cpp:431-464
    OrbRng rng(0x12345678);
    for (int i = 0; i < 2 * n; ++i) out[i] = 0;
    const int ntuples = ORB_DESC_BYTES * 4;
    for (int i = 0; i < ntuples; ++i)
        for (int k = 0; k < wta_k; ++k)
            for (;;) {
                const int idx = rng.uniform(0, ORB_NPOINTS);
                const int x = pool0[2 * idx], y = pool0[2 * idx + 1];
                int k1;
                for (k1 = 0; k1 < k; ++k1)
                    if (px[wta_k * i + k1] == x && py[wta_k * i + k1] == y) break;
                if (k1 == k) { px[wta_k * i + k] = x; py[wta_k * i + k] = y; break; }
            }
}

// How far a rotated test point lands from its keypoint at most: |x sin + y cos| <= hypot(x, y), rounded to nearest; the factor covers the
// f32 rounding of the two products, the sum and sin / cos.
inline int orb_pattern_reach(const int *pattern, int n)
{
    int r = 0;
    for (int i = 0; i < n; ++i) {
        const double h = std::sqrt((double)pattern[i] * pattern[i] + (double)pattern[n + i] * pattern[n + i]);
        const int ri = (int)std::floor(h * 1.00001 + 0.5);
        if (ri > r) r = ri;
    }
    return r;
}

// orb.cpp:519-534.  -> the number of entries (half_patch + 2)
inline int orb_u_max(int patch_size, int *u_max /*[ORB_UMAX_N]*/)
{
    const int half = patch_size / 2;
    for (int i = 0; i < ORB_UMAX_N; ++i) u_max[i] = 0;
    for (int v = 0; v <= half * std::sqrt(2.f) / 2 + 1; ++v) u_max[v] = cv_round(std::sqrt((float)(half * half - v * v)));
    for (int v = half, v0 = 0; v >= half * std::sqrt(2.f) / 2; --v) {
        while (u_max[v0] == u_max[v0 + 1]) ++v0;
        u_max[v] = v0;
        ++v0;
    }
    return half + 2;
}

// getScale, orb.cpp:573-576: std::pow(float, int) is evaluated in double and returned as float
inline float orb_get_scale(float scale_factor, int first_level, int level) { return (float)std::pow((double)scale_factor, (double)(level - first_level)); }

// orb.cpp:506-517.  The reference keeps the quotas in size_t; a negative last quota is rejected by the validator
inline void orb_features_per_level(int nfeatures, float scale_factor, int nlevels, int *quota)
{
    const float factor = 1.0f / scale_factor;
    float n_desired = (float)((double)(nfeatures * (1.0f - factor)) / (1.0 - std::pow((double)factor, (double)nlevels)));
    long long sum = 0;
    for (int level = 0; level < nlevels - 1; ++level) {
        quota[level] = cv_round(n_desired);
        sum += quota[level];
        n_desired *= factor;
    }
    quota[nlevels - 1] = (int)(nfeatures - sum);
}

// create / set_params.  Deviations from the reference: everything it would compute garbage with is rejected.
// detect = false (provided keypoints): the quotas are not used and not checked.
inline OrbErr orb_check_params(const mi_orb_params &p, bool detect = true)
{
    if (p.patch_size < 2) return {MI_ERR_BAD_ARG, "patchSize >= 2"};                                        // orb.cpp:500
    if (p.wta_k != 2 && p.wta_k != 3 && p.wta_k != 4) return {MI_ERR_BAD_ARG, "WTA_K == 2 || WTA_K == 3 || WTA_K == 4"};   // orb.cpp:501
    if (p.patch_size / 2 + 2 >= ORB_UMAX_N) return {MI_ERR_BAD_ARG, "u_max.size() < 32"};                    // orb.cpp:535
    if (p.nlevels < 1 || p.nlevels > ORB_MAX_LEVELS) return {MI_ERR_BAD_ARG, "1 <= nlevels <= 32"};
    if (!(p.scale_factor > 1.0f) || !(p.scale_factor <= 16.0f)) return {MI_ERR_BAD_ARG, "1 < scaleFactor <= 16"};
    if (p.nfeatures < 0) return {MI_ERR_BAD_ARG, "nfeatures >= 0"};
    if (p.first_level < 0 || p.first_level >= ORB_MAX_LEVELS) return {MI_ERR_BAD_ARG, "0 <= firstLevel < 32"};
    if (p.edge_threshold < 0) return {MI_ERR_BAD_ARG, "edgeThreshold >= 0"};
    if (p.score_type != ORB_HARRIS_SCORE && p.score_type != ORB_FAST_SCORE) return {MI_ERR_BAD_ARG, "scoreType is HARRIS_SCORE or FAST_SCORE"};
    if (p.fast_threshold < 0) return {MI_ERR_BAD_ARG, "fastThreshold >= 0"};
    if (!detect) return {MI_OK, nullptr};
    int quota[ORB_MAX_LEVELS];
    orb_features_per_level(p.nfeatures, p.scale_factor, p.nlevels, quota);
    for (int l = 0; l < p.nlevels; ++l)
        if (quota[l] < 0 || quota[l] > (1 << 29)) return {MI_ERR_BAD_ARG, "a level's feature quota is negative (the reference wraps it to a huge size_t)"};
    return {MI_OK, nullptr};
}

// The reach of the reads around a keypoint: the u_max disc (IC_Angle, orb.cu:192-211), the Harris window and its Sobel taps
// (orb.cu:106-123), the rotated pattern (orb.cu:250-252).  detect: the first two count only when keypoints are detected.
inline int orb_reach(const mi_orb_params &p, int pattern_reach, bool detect)
{
    int r = pattern_reach;
    if (detect) {
        if (p.patch_size / 2 > r) r = p.patch_size / 2;
        if (p.score_type == ORB_HARRIS_SCORE && ORB_HARRIS_BLOCK / 2 + 1 > r) r = ORB_HARRIS_BLOCK / 2 + 1;
    }
    return r;
}

struct OrbLevel {
    int rows, cols;
    float scale;              // getScale(level)
    float loc_scale;          // orb.cpp:854: level != firstLevel ? scale : 1
    float size;               // patchSize * scale, orb.cpp:862
    int src;                  // the level the image is resized from, -1: the caller's image (orb.cpp:683-709)
    int mask_mode;            // 0: copy, 1: resize, 2: resize and THRESH_TOZERO (orb.cpp:689-700)
    float fx, fy;             // resize_linear's arguments, resize.cpp:82-83,105
    int quota;                // n_features_per_level
    int fast_max;             // int(0.05 * area), orb.cpp:752
    int cap[3];               // keypoints at most: after FAST, after the first cull, after the second
    int pitch;                // bytes per row of the level's planes
    size_t off_img, off_mask, off_blur;           // from the start of the scratch
    size_t off_kp[3];         // keypoint areas: cap locations (int), then cap responses (float)
    size_t off_key;           // cap[0] keys
    size_t off_angle;         // cap[2] floats
    size_t off_fast;          // FAST's frame area
    fast::FastPlan fast;      // FAST's own plan of this level (one frame)
};

struct OrbPlan {
    OrbErr err;
    int nlevels, rows, cols, reach, ncull, detect, blur, describe;
    int max_total;            // keypoints of a call at most = sum of cap[2]
    std::vector<OrbLevel> levels;
    // the head of the scratch, cleared by CLEAR: per level 4 counts {FAST candidates, FAST emitted, after cull 1, after cull 2}, then per
    // cull and level ORB_DIGITS histograms and 2 * (ORB_DIGITS + 1) words of select state {prefix, k}
    size_t off_counts, off_hist, off_state, head_bytes, off_table, scratch_bytes;
    std::vector<OrbLaunch> launches;
    int host_waits;           // read-backs of a call: 1 when detecting, 0 with provided keypoints
};

// cull c reads the keypoint area and count cull_in(c) and writes cull_out(c); count k lives in counts[4 * level + 1 + k]
constexpr int orb_cull_in(int ncull, int c) { return ncull == 2 ? c : 0; }
constexpr int orb_cull_out(int ncull, int c) { return ncull == 2 ? c + 1 : 2; }

// rows, cols: the caller's image.  pattern_reach: orb_pattern_reach of the handle's pattern.  detect = 0: provided keypoints, whose
// per-level counts are `provided` (nlevels entries; the plan's levels are the provided octaves, orb.cpp:586-594).
inline OrbPlan orb_make_plan(const mi_orb_params &p, int pattern_reach, int rows, int cols, bool detect, bool describe, const int *provided = nullptr,
                             int provided_levels = 0)
{
    OrbPlan P = {};
    if ((P.err = orb_check_params(p, detect)).code) return P;
    if (rows < 1 || cols < 1) { P.err = {MI_ERR_BAD_SIZE, "empty image"}; return P; }
    if (rows > fast::FAST_MAX_SIDE || cols > fast::FAST_MAX_SIDE) { P.err = {MI_ERR_BAD_SIZE, "rows and cols must fit short2 locations (<= 32767)"}; return P; }
    const int L = detect ? p.nlevels : provided_levels;
    if (L < 1 || L > ORB_MAX_LEVELS) { P.err = {MI_ERR_BAD_ARG, "1 <= levels <= 32"}; return P; }
    P.nlevels = L; P.rows = rows; P.cols = cols; P.detect = detect; P.describe = describe;
    P.blur = describe && p.blur_for_descriptor;
    P.ncull = !detect ? 0 : p.score_type == ORB_HARRIS_SCORE ? 2 : 1;
    P.reach = orb_reach(p, describe ? pattern_reach : 0, detect);
    if (detect && p.edge_threshold < P.reach) {
        P.err = {MI_ERR_BAD_ARG, "edgeThreshold >= R, the reach of the disc, the Harris window and the rotated pattern (the reference reads out of bounds)"};
        return P;
    }
    int quota[ORB_MAX_LEVELS] = {};
    if (detect) orb_features_per_level(p.nfeatures, p.scale_factor, p.nlevels, quota);
    size_t o = 0;
    P.off_counts = o; o += orb_align((size_t)ORB_MAX_LEVELS * 4 * sizeof(int));
    P.off_hist = o;   o += orb_align((size_t)2 * ORB_MAX_LEVELS * ORB_DIGITS * ORB_BINS * sizeof(int));
    P.off_state = o;  o += orb_align((size_t)2 * ORB_MAX_LEVELS * 2 * (ORB_DIGITS + 1) * sizeof(unsigned));
    P.head_bytes = o;
    P.off_table = o; o += orb_align((size_t)ORB_MAX_LEVELS * ORB_LEVEL_DEV_BYTES);
    for (int l = 0; l < L; ++l) {
        OrbLevel v = {};
        v.scale = orb_get_scale(p.scale_factor, p.first_level, l);
        const float inv = 1.0f / v.scale;
        v.cols = cv_round(cols * inv); v.rows = cv_round(rows * inv);   // orb.cpp:674-676
        v.loc_scale = l != p.first_level ? v.scale : 1.0f;
        v.size = p.patch_size * v.scale;
        if (v.rows < 1 || v.cols < 1 || v.rows > fast::FAST_MAX_SIDE || v.cols > fast::FAST_MAX_SIDE) {
            P.err = {MI_ERR_BAD_SIZE, "a pyramid level is empty or exceeds 32767"};
            return P;
        }
        if (detect && (v.cols - 2 * p.edge_threshold <= 0 || v.rows - 2 * p.edge_threshold <= 0)) {
            P.err = {MI_ERR_BAD_SIZE, "a level's inner rectangle sz - 2 * edgeThreshold is empty (orb.cpp:714-715 throws)"};
            return P;
        }
        v.src = l <= p.first_level ? -1 : l - 1;
        v.mask_mode = l == p.first_level ? 0 : l < p.first_level ? 1 : 2;
        const int srows = v.src < 0 ? rows : P.levels[v.src].rows, scols = v.src < 0 ? cols : P.levels[v.src].cols;
        v.fx = (float)(1.0 / ((double)v.cols / scols));
        v.fy = (float)(1.0 / ((double)v.rows / srows));
        v.quota = quota[l];
        v.fast_max = (int)(0.05 * ((double)v.rows * v.cols));
        if (detect) {
            v.cap[0] = v.fast_max;
            v.cap[1] = P.ncull == 2 ? (int)std::min<long long>(v.cap[0], 2ll * v.quota) : v.cap[0];
            v.cap[2] = std::min(v.cap[1], v.quota);
        } else {
            v.cap[0] = v.cap[1] = v.cap[2] = provided ? provided[l] : 0;
        }
        v.pitch = (v.cols + 63) / 64 * 64;
        const size_t plane = orb_align((size_t)v.rows * v.pitch);
        v.off_img = o; o += plane;
        v.off_mask = o; if (detect) o += plane;
        v.off_blur = o; if (P.blur) o += plane;
        for (int k = 0; k < 3; ++k) {
            v.off_kp[k] = o;
            if (k == 0 || (k == 1 && P.ncull == 2) || (k == 2 && P.ncull >= 1)) o += orb_align((size_t)v.cap[k] * 8);
            else v.off_kp[k] = v.off_kp[k - 1];   // no cull in between: the same area
        }
        v.off_key = o;   if (detect) o += orb_align((size_t)v.cap[0] * 4);
        v.off_angle = o; o += orb_align((size_t)v.cap[2] * 4);
        v.off_fast = o;
        if (detect && v.fast_max >= 1) {
            const int sz[2] = {v.rows, v.cols};
            v.fast = fast::fast_make_plan(1, sz, p.fast_threshold, 1, v.fast_max);
            if (v.fast.err.code) { P.err = {v.fast.err.code, v.fast.err.msg}; return P; }
            o += orb_align(v.fast.scratch_bytes);
        }
        P.max_total += v.cap[2];
        P.levels.push_back(v);
    }
    P.scratch_bytes = o;

    // ---- the launch list
    auto per_kp = [](int cap) { return (unsigned)((cap + ORB_KP_PER_BLOCK - 1) / ORB_KP_PER_BLOCK); };
    auto max_cap = [&](int k) { int m = 0; for (const OrbLevel &v : P.levels) m = std::max(m, v.cap[k]); return m; };
    P.launches.push_back({ORB_K_CLEAR, -1, 0, 0, 0, 0});
    for (int l = 0; l < L; ++l) {
        const OrbLevel &v = P.levels[l];
        P.launches.push_back({ORB_K_LEVEL, l, 0, (unsigned)((v.cols + 63) / 64), (unsigned)((v.rows + 3) / 4), ORB_BLOCK});
    }
    if (detect) {
        for (int l = 0; l < L; ++l)
            for (size_t i = 0; i < P.levels[l].fast.launches.size(); ++i) {
                const fast::FastLaunch &k = P.levels[l].fast.launches[i];
                P.launches.push_back({ORB_K_FAST, l, (int)i, k.grid_x, k.grid_y, k.block});
            }
        for (int c = 0; c < P.ncull; ++c) {
            const int from = orb_cull_in(P.ncull, c);
            if (max_cap(from) > 0) {
                const unsigned gx = (unsigned)((max_cap(from) + ORB_BLOCK - 1) / ORB_BLOCK);
                for (int d = 0; d < ORB_DIGITS; ++d) P.launches.push_back({ORB_K_HIST, -1, c * ORB_DIGITS + d, gx, (unsigned)L, ORB_BLOCK});
                P.launches.push_back({ORB_K_RANK, -1, c, gx, (unsigned)L, ORB_BLOCK});
            }
            if (c == 0 && P.ncull == 2 && max_cap(1) > 0) P.launches.push_back({ORB_K_HARRIS, -1, 0, per_kp(max_cap(1)), (unsigned)L, ORB_BLOCK});
        }
        if (max_cap(2) > 0) P.launches.push_back({ORB_K_ANGLE, -1, 0, per_kp(max_cap(2)), (unsigned)L, ORB_BLOCK});
    }
    if (describe && max_cap(2) > 0) {
        if (P.blur)
            for (int l = 0; l < L; ++l) {
                const OrbLevel &v = P.levels[l];
                if (v.cap[2] > 0)
                    P.launches.push_back({ORB_K_BLUR, l, 0, (unsigned)((v.cols + ORB_BLUR_TILE - 1) / ORB_BLUR_TILE),
                                          (unsigned)((v.rows + ORB_BLUR_TILE - 1) / ORB_BLUR_TILE), ORB_BLOCK});
            }
        P.launches.push_back({ORB_K_DESC, -1, 0, per_kp(max_cap(2)), (unsigned)L, ORB_BLOCK});
    }
    if (detect) {
        if (max_cap(2) > 0) P.launches.push_back({ORB_K_MERGE, -1, 0, (unsigned)((max_cap(2) + ORB_BLOCK - 1) / ORB_BLOCK), (unsigned)L, ORB_BLOCK});
        P.launches.push_back({ORB_K_READBACK, -1, 0, 0, 0, 0});
        P.host_waits = 1;
    }
    return P;
}

}  // namespace orb
}  // namespace mi
