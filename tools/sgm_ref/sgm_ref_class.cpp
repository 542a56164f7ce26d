/* tools/sgm_ref/sgm_ref_class.cpp -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.
 * C entry point over the reference's host class cv::cuda::StereoSGM: modules/cudastereo/src/stereosgm.cpp is compiled as it lies into its
 * own object and driven through its public interface (createStereoSGM, compute).
 *
 * The class keeps its maps before the median to itself and overwrites the left map after the median in place.  To see them, that one
 * object is compiled with the name of the namespace median_filter replaced on the command line (-Dmedian_filter=median_filter_seen), so
 * its two calls of medianFilter arrive here: this function copies the source, calls the reference's medianFilter and copies the result.
 * Nothing the class computes is touched.
 *
 * censusTransform arrives here the same way (-Dcensus_transform=census_transform_seen).  The reference's census kernel writes only the
 * pixels a whole 9 x 7 window fits around and the class never clears the buffer, so the 4 / 3 pixel border of both census images is
 * whatever the allocation held; every cost next to it depends on that.  With zero_census_border set the destination is cleared before
 * the reference's censusTransform runs: the value the reference's own CPU twin gives the border, and what a fresh device allocation
 * holds in practice.  Without it the border keeps the allocation's fill byte, which is how the fixtures measure what hangs on it. */
#include <cstring>
#include <vector>
#include "opencv2/cudastereo.hpp"
#include "opencv2/core/private.cuda.hpp"
#include "cuda/stereosgm.hpp"

using cv::cuda::GpuMat;

namespace {
std::vector<GpuMat> g_seen;   /* source and result of every medianFilter call of the running compute(), in call order */
int g_zero_census_border = 1;
int g_pitch;                  /* bytes between the rows of the first source */
GpuMat copy_of(const GpuMat &m)
{
    GpuMat c(m.rows, m.cols, m.type());
    const size_t rb = (size_t)m.cols * cv::elem_size_of(m.type());
    for (int y = 0; y < m.rows; ++y) memcpy(c.ptr<unsigned char>(y), m.ptr<unsigned char>(y), rb);
    return c;
}
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
}  // namespace

namespace cv { namespace cuda { namespace device { namespace stereosgm { namespace median_filter_seen {
void medianFilter(const GpuMat &src, GpuMat &dst, Stream &stream)
{
    if (g_seen.empty()) g_pitch = (int)src.step;
    g_seen.push_back(copy_of(src));
    median_filter::medianFilter(src, dst, stream);
    g_seen.push_back(copy_of(dst));
}
}}}}}

namespace cv { namespace cuda { namespace device { namespace stereosgm { namespace census_transform_seen {
void censusTransform(const GpuMat &src, GpuMat &dest, Stream &stream)
{
    if (g_zero_census_border)
        for (int y = 0; y < dest.rows; ++y) memset(dest.ptr<unsigned char>(y), 0, (size_t)dest.cols * cv::elem_size_of(dest.type()));
    census_transform::censusTransform(src, dest, stream);
}
}}}}}

extern "C" {
void sgm_ref_zero_census_border(int on) { g_zero_census_border = on; }

/* left: rows x cols, right: rrows x rcols, both dense, 8 or 16 bits; ip: minDisparity, numDisparities, P1, P2, uniquenessRatio, mode.
 * disp and the four maps (left before / after the median, right before / after): rows x cols of 16 bits.  *pitch: bytes between the rows
 * of the maps the median reads.  1 if the class threw. */
int sgm_ref_compute(const void *left, const void *right, int rows, int cols, int rrows, int rcols, int is16, const int *ip, unsigned short *disp,
                    unsigned short *maps, int *pitch)
{
    try {
        const int type = is16 ? CV_16UC1 : CV_8UC1;
        GpuMat l = up(left, rows, cols, type), r = up(right, rrows, rcols, type), d;
        g_seen.clear();
        cv::Ptr<cv::cuda::StereoSGM> sgm = cv::cuda::createStereoSGM(ip[0], ip[1], ip[2], ip[3], ip[4], ip[5]);
        sgm->compute(l, r, d);
        if (d.rows != rows || d.cols != cols || d.type() != CV_16SC1 || g_seen.size() != 4) return 2;
        down(d, disp);
        for (int k = 0; k < 4; ++k) down(g_seen[k], maps + (size_t)k * rows * cols);
        *pitch = g_pitch;
        return 0;
    } catch (const std::exception &) { return 1; }
}
}
