// cv::cuda::FastFeatureDetector for gfx950 (wave64).  Replaces calcKeypoints and nonmaxSuppression of cudafeatures2d/src/cuda/fast.cu.
//
// The reference tests a pixel with an 8 KB __constant__ table, finds its score by a binary search of eight 16-way compares, appends
// with atomicInc in arrival order into an int32 plane it clears first, and waits on the host twice.  Here (fast_plan.h has the list):
//   - the table test is "the 16-bit mask has a circular run of at least nine set bits", four shifts and ands;
//   - the score is max over both polarities and the 16 arcs of nine of the arc's smallest difference, minus one: the largest t at
//     which the pixel still is a candidate, which is what the reference's search converges to;
//   - a wave's ballot over a 64-pixel row segment is the segment's candidate set, so ORDER IS ROW-MAJOR (y, then x) and needs no
//     atomics; ranks and output positions come from one single-workgroup scan between launches, nothing spins on another workgroup;
//   - the score plane holds one byte per pixel (0 or score + 1) and every byte, mask and count is written, never accumulated.
// No __constant__ memory, no textures, no environment switches.
#include "fast_dev.h"

namespace mi {
namespace fast {

namespace {

constexpr int LDS_ROWS = FAST_TILE_H + 2 * FAST_HALO;
// a staged row starts at the dword that holds column x0 - 3: up to 3 bytes of slack in front of 64 + 6 columns
constexpr int LDS_DWORDS = (FAST_TILE_W + 2 * FAST_HALO + 3 + 3) / 4;
constexpr int LDS_ROW_BYTES = LDS_DWORDS * 4;

// the ring in the reference's bit order (fast.cu:223-252: C[0] byte 0 is bit 0 ... C[3] byte 3 is bit 15), a closed circle
__device__ __forceinline__ constexpr int ring_dy(int k)
{
    return k == 0 ? 3 : k == 1 ? 3 : k == 2 ? 2 : k == 3 ? 1 : k == 4 ? 0 : k == 5 ? -1 : k == 6 ? -2 : k == 7 ? -3 : k == 8 ? -3 : k == 9 ? -3
         : k == 10 ? -2 : k == 11 ? -1 : k == 12 ? 0 : k == 13 ? 1 : k == 14 ? 2 : 3;
}
__device__ __forceinline__ constexpr int ring_dx(int k)
{
    return k == 0 ? 0 : k == 1 ? 1 : k == 2 ? 2 : k == 3 ? 3 : k == 4 ? 3 : k == 5 ? 3 : k == 6 ? 2 : k == 7 ? 1 : k == 8 ? 0 : k == 9 ? -1
         : k == 10 ? -2 : k == 11 ? -3 : k == 12 ? -3 : k == 13 ? -3 : k == 14 ? -2 : -1;
}

// isKeyPoint's table test (fast.cu:187-191): a circular run of >= 9 set bits in the 16-bit mask
__device__ __forceinline__ bool run_of_nine(unsigned m)
{
    const unsigned d = m | (m << 16);
    const unsigned a = d & (d >> 1);
    const unsigned b = a & (a >> 2);
    const unsigned c = b & (b >> 4);
    return ((c & (d >> 8)) & 0xffffu) != 0;
}

// max over the 16 arcs of nine of the arc's minimum
__device__ __forceinline__ int best_arc(const int (&a)[16])
{
    int m2[16], m4[16], m8[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) m2[k] = min(a[k], a[(k + 1) & 15]);
#pragma unroll
    for (int k = 0; k < 16; ++k) m4[k] = min(m2[k], m2[(k + 2) & 15]);
#pragma unroll
    for (int k = 0; k < 16; ++k) m8[k] = min(m4[k], m4[(k + 4) & 15]);
    int best = -256;
#pragma unroll
    for (int k = 0; k < 16; ++k) best = max(best, min(m8[k], a[(k + 8) & 15]));
    return best;
}

__device__ __forceinline__ int score_of(unsigned char b) { return b ? (int)b - 1 : 0; }   // a pixel that is no candidate scores 0

__global__ __launch_bounds__(FAST_BLOCK) void k_fast_score(FastImage im, int th, unsigned char *plane, int pitch, unsigned long long *cand,
                                                            int segs_x)
{
    __shared__ unsigned tile[LDS_ROWS * LDS_DWORDS];
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * FAST_TILE_W, y0 = blockIdx.y * FAST_TILE_H;
    // Stage the tile and its halo.  A row's dwords are read whole only where all four bytes are columns of that row; the rest byte by
    // byte, so nothing outside [data + y * step, data + y * step + cols) of a row y in [0, rows) is touched, whatever base and step are.
    for (int it = tid; it < LDS_ROWS * LDS_DWORDS; it += FAST_BLOCK) {
        const int r = it / LDS_DWORDS, d = it - r * LDS_DWORDS;
        const int y = y0 - FAST_HALO + r;
        unsigned v = 0;
        if (y >= 0 && y < im.rows) {
            const unsigned char *row = im.data + (long long)y * im.step;
            const long long a = (long long)(uintptr_t)row + (x0 - FAST_HALO);
            const int c0 = (int)((a & ~3LL) + 4 * d - (long long)(uintptr_t)row);   // the column of the dword's byte 0
            if (c0 >= 0 && c0 + 3 < im.cols) {
                v = *(const unsigned *)(row + c0);
            } else {
#pragma unroll
                for (int b = 0; b < 4; ++b)
                    if (c0 + b >= 0 && c0 + b < im.cols) v |= (unsigned)row[c0 + b] << (8 * b);
            }
        }
        tile[it] = v;
    }
    __syncthreads();

    const unsigned char *tb = (const unsigned char *)tile;
    const int lane = tid & 63, wave = tid >> 6;
    const int x = x0 + lane;
    const unsigned base_lo = (unsigned)(uintptr_t)im.data + (unsigned)(x0 - FAST_HALO);   // the low bits decide a row's slack
    for (int k = 0; k < FAST_TILE_H / 4; ++k) {
        const int ry = wave * (FAST_TILE_H / 4) + k, y = y0 + ry;
        if (y >= im.rows) break;   // wave-uniform
        int out = 0;
        bool tested = x >= FAST_HALO && x < im.cols - FAST_HALO && y >= FAST_HALO && y < im.rows - FAST_HALO;
        if (tested && im.mask) tested = im.mask[(long long)y * im.mstep + x] != 0;
        if (tested) {
            int off[2 * FAST_HALO + 1];   // of (y + dy, x) in the tile, dy = -3 .. 3
#pragma unroll
            for (int j = 0; j < 2 * FAST_HALO + 1; ++j) {
                const unsigned slack = (base_lo + (unsigned)(y - FAST_HALO + j) * (unsigned)im.step) & 3u;
                off[j] = (ry + j) * LDS_ROW_BYTES + lane + FAST_HALO + (int)slack;
            }
            const int v = tb[off[FAST_HALO]];
            // the four compass points first: an arc of nine holds at least two of them (the reference rejects on two, fast.cu:236-240)
            const int c0 = tb[off[6]] - v, c4 = tb[off[3] + 3] - v, c8 = tb[off[0]] - v, c12 = tb[off[3] - 3] - v;
            const int dark = (c0 < -th) + (c4 < -th) + (c8 < -th) + (c12 < -th);
            const int bright = (c0 > th) + (c4 > th) + (c8 > th) + (c12 > th);
            if (dark >= 2 || bright >= 2) {
                int a[16], b[16];
                unsigned m1 = 0, m2 = 0;
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const int diff = (int)tb[off[ring_dy(i) + FAST_HALO] + ring_dx(i)] - v;
                    m1 |= (unsigned)(diff < -th) << i;
                    m2 |= (unsigned)(diff > th) << i;
                    a[i] = -diff; b[i] = diff;
                }
                if (run_of_nine(m1) || run_of_nine(m2)) out = max(best_arc(a), best_arc(b));   // = cornerScore + 1, in th + 1 .. 255
            }
        }
        if (x < im.cols) plane[(long long)y * pitch + x] = (unsigned char)out;
        const unsigned long long bits = __ballot(out != 0);
        if (lane == 0) cand[(long long)y * segs_x + blockIdx.x] = bits;
    }
}

__global__ __launch_bounds__(FAST_BLOCK) void k_fast_nms(const unsigned char *plane, int pitch, const unsigned long long *cand,
                                                          unsigned long long *surv, int segs_x, int nseg)
{
    const int lane = threadIdx.x & 63;
    const int seg = blockIdx.x * FAST_SEGS_PER_BLOCK + (threadIdx.x >> 6);
    if (seg >= nseg) return;
    const unsigned long long m = cand[seg];
    if (!m) {   // wave-uniform
        if (lane == 0) surv[seg] = 0;
        return;
    }
    bool keep = false;
    if ((m >> lane) & 1) {   // a candidate has a whole ring: its eight neighbours are inside the plane
        const int y = seg / segs_x, x = (seg - y * segs_x) * FAST_SEG + lane;
        const unsigned char *p = plane + (long long)y * pitch + x;
        const int s = score_of(p[0]);
        keep = s > score_of(p[-pitch - 1]) && s > score_of(p[-pitch]) && s > score_of(p[-pitch + 1]) && s > score_of(p[-1]) &&
               s > score_of(p[1]) && s > score_of(p[pitch - 1]) && s > score_of(p[pitch]) && s > score_of(p[pitch + 1]);
    }
    const unsigned long long bits = __ballot(keep);
    if (lane == 0) surv[seg] = bits;
}

// exclusive scan of one int per thread over the workgroup; -> the thread's prefix, *total = the sum
__device__ int block_exclusive(int v, int *sh, int *total)
{
    const int t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (int o = 1; o < FAST_SCAN_THREADS; o <<= 1) {
        const int add = t >= o ? sh[t - o] : 0;
        __syncthreads();
        sh[t] += add;
        __syncthreads();
    }
    const int incl = sh[t];
    *total = sh[FAST_SCAN_THREADS - 1];
    __syncthreads();
    return incl - v;
}

// ONE workgroup.  Thread t owns the contiguous run of segments [t * chunk, (t + 1) * chunk): ranks and positions are row-major.
__global__ __launch_bounds__(FAST_SCAN_THREADS) void k_fast_scan(const unsigned long long *cand, const unsigned long long *surv,
                                                                  unsigned long long *emit, int *pos, int nseg, int max_npoints, int *counts)
{
    __shared__ int sh[FAST_SCAN_THREADS];
    const int t = threadIdx.x;
    const int chunk = (nseg + FAST_SCAN_THREADS - 1) / FAST_SCAN_THREADS;
    const int lo = min(nseg, t * chunk), hi = min(nseg, lo + chunk);
    int n = 0;
    for (int i = lo; i < hi; ++i) n += __popcll(cand[i]);
    int total_cand, total_emit;
    int rank = block_exclusive(n, sh, &total_cand);
    // the first max_npoints candidates keep their slot (fast.cu:263-266); all of them have written their score
    int e = 0;
    for (int i = lo; i < hi; ++i) {
        unsigned long long m = cand[i];
        const int c = __popcll(m);
        const int kept = max(0, min(c, max_npoints - rank));
        while (__popcll(m) > kept) m &= ~(1ull << (63 - __clzll((long long)m)));   // at most one segment of the image loops here
        m &= surv[i];
        emit[i] = m;
        e += __popcll(m);
        rank += c;
    }
    int o = block_exclusive(e, sh, &total_emit);
    for (int i = lo; i < hi; ++i) {
        pos[i] = o;
        o += __popcll(emit[i]);
    }
    if (t == 0) { counts[0] = total_cand; counts[1] = total_emit; }
}

__global__ __launch_bounds__(FAST_BLOCK) void k_fast_emit(const unsigned char *plane, int pitch, const unsigned long long *emit, const int *pos,
                                                           int segs_x, int nseg, int with_score, short2 *loc, float *resp)
{
    const int lane = threadIdx.x & 63;
    const int seg = blockIdx.x * FAST_SEGS_PER_BLOCK + (threadIdx.x >> 6);
    if (seg >= nseg) return;
    const unsigned long long m = emit[seg];
    if (!((m >> lane) & 1)) return;
    const int y = seg / segs_x, x = (seg - y * segs_x) * FAST_SEG + lane;
    const int at = pos[seg] + __popcll(m & ((1ull << lane) - 1));
    loc[at] = make_short2((short)x, (short)y);
    resp[at] = with_score ? (float)score_of(plane[(long long)y * pitch + x]) : 0.0f;   // fast.cpp:171: zero without suppression
}

__global__ __launch_bounds__(FAST_BLOCK) void k_fast_plane_to_scores(const unsigned char *plane, int pitch, int *scores, long long ostep, int rows,
                                                                      int cols)
{
    const int x = blockIdx.x * FAST_BLOCK + threadIdx.x, y = blockIdx.y;
    if (x < cols && y < rows) *(int *)((char *)scores + (long long)y * ostep + 4ll * x) = score_of(plane[(long long)y * pitch + x]);
}

__global__ __launch_bounds__(FAST_BLOCK) void k_fast_points(const short2 *loc, int n, float2 *points)
{
    const int i = blockIdx.x * FAST_BLOCK + threadIdx.x;
    if (i < n) points[i] = make_float2((float)loc[i].x, (float)loc[i].y);
}

}  // namespace

int score(const FastLaunch &k, const FastFrame &f, const FastImage &im, int threshold, const FastScratch &s, hipStream_t st)
{
    hipLaunchKernelGGL(k_fast_score, dim3(k.grid_x, k.grid_y), dim3(k.block), 0, st, im, threshold, s.plane, f.pitch, s.cand, f.segs_x);
    MI_HIP_TRY(hipGetLastError());
    return MI_OK;
}

int nms(const FastLaunch &k, const FastFrame &f, const FastScratch &s, hipStream_t st)
{
    hipLaunchKernelGGL(k_fast_nms, dim3(k.grid_x), dim3(k.block), 0, st, s.plane, f.pitch, s.cand, s.surv, f.segs_x, f.nseg);
    MI_HIP_TRY(hipGetLastError());
    return MI_OK;
}

int scan(const FastLaunch &k, const FastFrame &f, const FastScratch &s, bool use_nms, int max_npoints, hipStream_t st)
{
    hipLaunchKernelGGL(k_fast_scan, dim3(k.grid_x), dim3(k.block), 0, st, s.cand, use_nms ? s.surv : s.cand, s.emit, s.pos, f.nseg, max_npoints,
                       s.counts);
    MI_HIP_TRY(hipGetLastError());
    return MI_OK;
}

int emit(const FastLaunch &k, const FastFrame &f, const FastScratch &s, bool use_nms, void *loc, float *resp, hipStream_t st)
{
    hipLaunchKernelGGL(k_fast_emit, dim3(k.grid_x), dim3(k.block), 0, st, s.plane, f.pitch, s.emit, s.pos, f.segs_x, f.nseg, use_nms ? 1 : 0,
                       (short2 *)loc, resp);
    MI_HIP_TRY(hipGetLastError());
    return MI_OK;
}

int plane_to_scores(const FastFrame &f, const unsigned char *plane, int *scores, long long ostep, hipStream_t st)
{
    hipLaunchKernelGGL(k_fast_plane_to_scores, dim3(div_up(f.cols, FAST_BLOCK), f.rows), dim3(FAST_BLOCK), 0, st, plane, f.pitch, scores, ostep,
                       f.rows, f.cols);
    MI_HIP_TRY(hipGetLastError());
    return MI_OK;
}

int locations_to_points(const void *loc, int n, float *points, hipStream_t st)
{
    hipLaunchKernelGGL(k_fast_points, dim3(div_up(n, FAST_BLOCK)), dim3(FAST_BLOCK), 0, st, (const short2 *)loc, n, (float2 *)points);
    MI_HIP_TRY(hipGetLastError());
    return MI_OK;
}

}  // namespace fast
}  // namespace mi
