/* tools/stereocsbp_ref/csbp_ref_class.cpp -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.
 * C entry points over the reference's host class cv::cuda::StereoConstantSpaceBP: modules/cudastereo/src/stereocsbp.cpp is compiled as it
 * lies into its own object; this file drives it through its public interface (createStereoConstantSpaceBP, the setters, compute,
 * getNumLevels, estimateRecommendedParams). */
#include <cstring>
#include <cmath>
#include "opencv2/cudastereo.hpp"
#include "opencv2/core/private.cuda.hpp"

using cv::cuda::GpuMat;

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
}  // namespace

extern "C" {
/* left, right: dense rows x cols x cn bytes (right: rrows x rcols x rcn, read only when it matches left); ip: ndisp, iters, levels,
 * nr_plane, msg_type, min_disp, use_local_init_data_cost; w: max_data_term, data_weight, max_disc_term, disc_single_jump; disp: rows x
 * cols of out_type (CV_16SC1 = 3: the class's own choice; another type: handed over as a fixed-type output).  1 if the class threw. */
int csbp_ref_compute(const unsigned char *left, const unsigned char *right, int rows, int cols, int cn, int rrows, int rcols, int rcn,
                     const int *ip, const float *w, int out_type, void *disp, int *levels_after)
{
    try {
        GpuMat l = left ? up(left, rows, cols, CV_MAKETYPE(CV_8U, cn)) : GpuMat(rows, cols, CV_MAKETYPE(CV_8U, cn));
        GpuMat r = right ? up(right, rrows, rcols, CV_MAKETYPE(CV_8U, rcn)) : GpuMat(rrows, rcols, CV_MAKETYPE(CV_8U, rcn));
        GpuMat d;
        cv::cuda::Stream st;
        if (out_type != CV_16SC1) d.create(rows, cols, out_type);
        cv::Ptr<cv::cuda::StereoConstantSpaceBP> bp = cv::cuda::createStereoConstantSpaceBP(ip[0], ip[1], ip[2], ip[3], ip[4]);
        bp->setMinDisparity(ip[5]);
        bp->setUseLocalInitDataCost(ip[6] != 0);
        bp->setMaxDataTerm(w[0]); bp->setDataWeight(w[1]); bp->setMaxDiscTerm(w[2]); bp->setDiscSingleJump(w[3]);
        bp->compute(l, r, cv::_OutputArray(d, out_type != CV_16SC1), st);
        *levels_after = bp->getNumLevels();
        if (d.rows != rows || d.cols != cols || d.type() != out_type) return 2;
        if (disp) down(d, disp);
        return 0;
    } catch (const std::exception &) { return 1; }
}
void csbp_ref_estimate(int width, int height, int *ndisp, int *iters, int *levels, int *nr_plane)
{
    cv::cuda::StereoConstantSpaceBP::estimateRecommendedParams(width, height, *ndisp, *iters, *levels, *nr_plane);
}
}
