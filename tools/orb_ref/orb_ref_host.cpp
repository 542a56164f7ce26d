/* tools/orb_ref/orb_ref_host.cpp -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.
 * The host arithmetic of the reference's modules/cudafeatures2d/src/orb.cpp, run from its own text: tools/make_golden_orb.py cuts line
 * ranges out of that file with oracle/refshim/cu2host.py --slice into its temporary directory, and they are #included below, verbatim:
 *   orb_table.gen.inc    the initializer of bit_pattern_31_ (the learned test pairs of patch 31)
 *   orb_pattern.gen.inc  initializeOrbPattern and makeRandomPattern
 *   orb_ctor.gen.inc     the constructor's quota and u_max statements (orb.cpp:505-535)
 *   orb_calc.gen.inc     the constructor's "Calc pattern" statements (orb.cpp:538-566), up to the upload
 *   orb_scale.gen.inc    getScale
 *   orb_size.gen.inc     the level-size statements of buildScalePyramids (orb.cpp:674-676)
 * The whole file cannot be compiled against oracle/refshim/cudahost: its stub core lacks cv::RNG, Mat::setTo / rowRange / the
 * (rows, cols, type) constructor, Range, GpuMat::rowRange / setTo(Scalar) / operator()(Range, Range), ensureSizeIsEnough(Size, ...),
 * OutputArray::needed, cuda::threshold, cuda::bitwise_and, THRESH_TOZERO and NORM_HAMMING (21 errors), and nothing under oracle/ is edited.
 * Written here, because they are main-repository pieces: cv::RNG (multiply-with-carry; the fixtures do NOT pin it), Point, Size, a Mat
 * that holds ints, cvRound, CV_Assert. */
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <vector>

namespace {
struct Point { int x, y; };
struct Size { int width, height; Size(int w, int h) : width(w), height(h) {} };
struct Scalar { int v; static Scalar all(int a) { Scalar s = {a}; return s; } };
enum { CV_32SC1 = 4 };
struct Mat {
    int rows = 0, cols = 0;
    std::vector<int> d;
    void create(int r, int c, int) { rows = r; cols = c; d.assign((size_t)r * c, 0x7fffffff); }
    void setTo(Scalar s) { for (int &v : d) v = s.v; }
    template <typename T> T *ptr(int r) { return (T *)(d.data() + (size_t)r * cols); }
};
struct RNG {   /* main repository, core.hpp / operations.hpp */
    uint64_t state;
    explicit RNG(uint64_t s) : state(s ? s : 0xffffffffu) {}
    unsigned next() { state = (uint64_t)(unsigned)state * 4164903690U + (unsigned)(state >> 32); return (unsigned)state; }
    int uniform(int a, int b) { return a == b ? a : (int)(next() % (b - a) + a); }
};
inline int cvRound(double v) { return (int)std::nearbyint(v); }   /* main repository, fast_math.hpp: round half to even */
#define CV_Assert(expr) do { if (!(expr)) throw std::runtime_error(#expr); } while (0)

#include "orb_table.gen.inc"
#include "orb_pattern.gen.inc"
#include "orb_scale.gen.inc"

struct Image { int rows, cols; };
}  // namespace

extern "C" {
/* table: 1024 ints, the learned pool as {x, y} points */
void orb_ref_table31(int *table) { memcpy(table, bit_pattern_31_, sizeof(bit_pattern_31_)); }

/* the constructor's host tables.  quota: nLevels entries; u_max: *n_u_max entries (room for 64) */
int orb_ref_ctor(int nFeatures, float scaleFactor, int nLevels, int patchSize, int *quota, int *u_max_out, int *n_u_max)
{
    try {
        const int nFeatures_ = nFeatures, nLevels_ = nLevels, patchSize_ = patchSize;
        const float scaleFactor_ = scaleFactor;
        std::vector<size_t> n_features_per_level_;
#include "orb_ctor.gen.inc"
        for (int l = 0; l < nLevels; ++l) quota[l] = static_cast<int>(n_features_per_level_[l]);   /* as orb.cpp:765 reads them */
        *n_u_max = (int)u_max.size();
        for (size_t i = 0; i < u_max.size(); ++i) u_max_out[i] = u_max[i];
        return 0;
    } catch (const std::exception &) { return -1; }
}

/* the matrix the constructor uploads: out = 2 x *cols ints (room for 1024) */
int orb_ref_pattern(int patchSize, int WTA_K, int *out, int *cols)
{
    try {
        const int patchSize_ = patchSize, WTA_K_ = WTA_K;
        auto descriptorSize = []() { return 32; };   /* cv::ORB::kBytes, orb.cpp:357 */
#include "orb_calc.gen.inc"
        *cols = h_pattern.cols;
        memcpy(out, h_pattern.d.data(), sizeof(int) * h_pattern.d.size());
        return 0;
    } catch (const std::exception &) { return -1; }
}

float orb_ref_scale(float scaleFactor, int firstLevel, int level) { return getScale(scaleFactor, firstLevel, level); }

void orb_ref_level_size(int rows, int cols, float scaleFactor, int firstLevel, int level, int *out_rows, int *out_cols)
{
    const Image image = {rows, cols};
    const float scaleFactor_ = scaleFactor;
    const int firstLevel_ = firstLevel;
#include "orb_size.gen.inc"
    *out_rows = sz.height; *out_cols = sz.width;
}
}
