/* tools/sgm_ref/sgm_ref_stage.cpp -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.
 * C entry points over the kernel wrappers of the reference's modules/cudastereo/src/cuda/stereosgm.cu (rewritten only at its launch
 * sites by oracle/refshim/cu2host.py and run on the CPU through oracle/refshim/cudashim), each on its own.  Matrices arrive and leave
 * dense; inside they are GpuMats of the stub core, so rows have the pitch a device allocation would give them and a matrix the wrapper
 * only writes starts out filled with the byte sgm_ref_set_fill chose. */
#include <cstring>
#include "opencv2/cudev/common.hpp"
#include "opencv2/cudastereo.hpp"
#include "cuda/stereosgm.hpp"

using cv::cuda::GpuMat;
using cv::cuda::Stream;
namespace sgm = cv::cuda::device::stereosgm;

/* the path wrappers are not in stereosgm.hpp; the reference's own test declares them like this (test/test_sgm_funcs.cpp) */
namespace cv { namespace cuda { namespace device { namespace stereosgm { namespace path_aggregation {
#define SGM_REF_PATH(space, name) namespace space { template <unsigned int MAX_DISPARITY> void name(const GpuMat &left, const GpuMat &right, \
    GpuMat &dest, unsigned int p1, unsigned int p2, int min_disp, Stream &stream); }
SGM_REF_PATH(vertical, aggregateUp2DownPath)
SGM_REF_PATH(vertical, aggregateDown2UpPath)
SGM_REF_PATH(horizontal, aggregateLeft2RightPath)
SGM_REF_PATH(horizontal, aggregateRight2LeftPath)
SGM_REF_PATH(oblique, aggregateUpleft2DownrightPath)
SGM_REF_PATH(oblique, aggregateUpright2DownleftPath)
SGM_REF_PATH(oblique, aggregateDownright2UpleftPath)
SGM_REF_PATH(oblique, aggregateDownleft2UprightPath)
}}}}}

namespace {
GpuMat up(const void *p, int rows, int cols, int type)
{
    GpuMat m(rows, cols, type);
    const size_t rb = (size_t)cols * cv::elem_size_of(type);
    for (int y = 0; y < rows; ++y) memcpy(m.ptr<unsigned char>(y), (const unsigned char *)p + y * rb, rb);
    return m;
}
void down(const GpuMat &m, void *p)
{
    const size_t rb = (size_t)m.cols * cv::elem_size_of(m.type());
    for (int y = 0; y < m.rows; ++y) memcpy((unsigned char *)p + y * rb, m.ptr<unsigned char>(y), rb);
}

template <unsigned int D> void path(int dir, const GpuMat &l, const GpuMat &r, GpuMat &dest, unsigned p1, unsigned p2, int min_disp)
{
    namespace pa = sgm::path_aggregation;
    Stream &st = Stream::Null();
    switch (dir) {   /* the order PathAggregation::operator() gives its eight buffers */
    case 0: pa::vertical::aggregateUp2DownPath<D>(l, r, dest, p1, p2, min_disp, st); break;
    case 1: pa::vertical::aggregateDown2UpPath<D>(l, r, dest, p1, p2, min_disp, st); break;
    case 2: pa::horizontal::aggregateLeft2RightPath<D>(l, r, dest, p1, p2, min_disp, st); break;
    case 3: pa::horizontal::aggregateRight2LeftPath<D>(l, r, dest, p1, p2, min_disp, st); break;
    case 4: pa::oblique::aggregateUpleft2DownrightPath<D>(l, r, dest, p1, p2, min_disp, st); break;
    case 5: pa::oblique::aggregateUpright2DownleftPath<D>(l, r, dest, p1, p2, min_disp, st); break;
    case 6: pa::oblique::aggregateDownright2UpleftPath<D>(l, r, dest, p1, p2, min_disp, st); break;
    default: pa::oblique::aggregateDownleft2UprightPath<D>(l, r, dest, p1, p2, min_disp, st); break;
    }
}
}  // namespace

extern "C" {
void sgm_ref_set_fill(int byte) { cv::cudahost_alloc_fill() = (unsigned char)byte; }

/* every entry: 0, or 1 if the reference threw */
int sgm_ref_census(const void *src, int rows, int cols, int is16, int *dst)
{
    try {
        GpuMat s = up(src, rows, cols, is16 ? CV_16UC1 : CV_8UC1), d(rows, cols, CV_32SC1);
        sgm::census_transform::censusTransform(s, d, Stream::Null());
        down(d, dst);
        return 0;
    } catch (const std::exception &) { return 1; }
}

/* one path; dst: rows * cols * ndisp bytes */
int sgm_ref_path(const int *left, const int *right, int rows, int cols, int ndisp, int dir, int p1, int p2, int min_disp, unsigned char *dst)
{
    try {
        GpuMat l = up(left, rows, cols, CV_32SC1), r = up(right, rows, cols, CV_32SC1), d(1, rows * cols * ndisp, CV_8UC1);
        if (ndisp == 64) path<64>(dir, l, r, d, p1, p2, min_disp);
        else if (ndisp == 128) path<128>(dir, l, r, d, p1, p2, min_disp);
        else if (ndisp == 256) path<256>(dir, l, r, d, p1, p2, min_disp);
        else return 1;
        down(d, dst);
        return 0;
    } catch (const std::exception &) { return 1; }
}

/* cost: paths * rows * cols * ndisp bytes; mode: StereoSGBM::MODE_HH (8 paths) or MODE_HH4 (4) */
int sgm_ref_wta(const unsigned char *cost, int rows, int cols, int ndisp, int mode, float uniqueness, int subpixel, unsigned short *left,
                unsigned short *right)
{
    try {
        const int paths = mode == cv::StereoSGBM::MODE_HH4 ? 4 : 8;
        GpuMat c = up(cost, 1, paths * rows * cols * ndisp, CV_8UC1), l(rows, cols, CV_16SC1), r(rows, cols, CV_16SC1);
        namespace w = sgm::winner_takes_all;
        if (ndisp == 64) w::winnerTakesAll<64>(c, l, r, uniqueness, subpixel != 0, mode, Stream::Null());
        else if (ndisp == 128) w::winnerTakesAll<128>(c, l, r, uniqueness, subpixel != 0, mode, Stream::Null());
        else if (ndisp == 256) w::winnerTakesAll<256>(c, l, r, uniqueness, subpixel != 0, mode, Stream::Null());
        else return 1;
        down(l, left);
        down(r, right);
        return 0;
    } catch (const std::exception &) { return 1; }
}

/* *pitch: the bytes between rows of the source, which is what the reference picks its kernel by */
int sgm_ref_median(const unsigned short *src, int rows, int cols, unsigned short *dst, int *pitch)
{
    try {
        GpuMat s = up(src, rows, cols, CV_16SC1), d(rows, cols, CV_16SC1);
        *pitch = (int)s.step;
        sgm::median_filter::medianFilter(s, d, Stream::Null());
        down(d, dst);
        return 0;
    } catch (const std::exception &) { return 1; }
}

int sgm_ref_check(unsigned short *left_disp, const unsigned short *right_disp, const void *src_left, int is16, int rows, int cols, int subpixel)
{
    try {
        GpuMat l = up(left_disp, rows, cols, CV_16SC1), r = up(right_disp, rows, cols, CV_16SC1);
        GpuMat s = up(src_left, rows, cols, is16 ? CV_16UC1 : CV_8UC1);
        sgm::check_consistency::checkConsistency(l, r, s, subpixel != 0, Stream::Null());
        down(l, left_disp);
        return 0;
    } catch (const std::exception &) { return 1; }
}

int sgm_ref_range(unsigned short *disp, int rows, int cols, int subpixel, int min_disp)
{
    try {
        GpuMat d = up(disp, rows, cols, CV_16SC1);
        sgm::correct_disparity_range::correctDisparityRange(d, subpixel != 0, min_disp, Stream::Null());
        down(d, disp);
        return 0;
    } catch (const std::exception &) { return 1; }
}
}
