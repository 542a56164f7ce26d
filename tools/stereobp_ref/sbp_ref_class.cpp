/* tools/stereobp_ref/sbp_ref_class.cpp -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.
 * C entry points over the reference's host class cv::cuda::StereoBeliefPropagation: modules/cudastereo/src/stereobp.cpp is compiled as
 * it lies into its own object; this file drives it through its public interface (createStereoBeliefPropagation, the setters, the two
 * compute overloads) and supplies the three GpuMat operations of the stub core that the class calls on 16-bit matrices (the stub's own
 * definitions serve 32-bit types only, so oracle/refshim/cudahost/cudahost.cpp is not linked). */
#include <cstring>
#include <cmath>
#include <algorithm>
#include "opencv2/cudastereo.hpp"
#include "opencv2/core/private.cuda.hpp"

using cv::cuda::GpuMat;

namespace cv { namespace cuda {
GpuMat &GpuMat::setTo(Scalar s, Stream &)
{
    CV_Assert(s[0] == 0);
    for (int y = 0; y < rows; ++y) memset(ptr<unsigned char>(y), 0, (size_t)cols * elem_size_of(type()));
    return *this;
}
void GpuMat::copyTo(GpuMat &dst, Stream &) const
{
    dst.create(rows, cols, type());
    if (dst.data == data) return;
    for (int y = 0; y < rows; ++y) memcpy(dst.ptr<unsigned char>(y), ptr<unsigned char>(y), (size_t)cols * elem_size_of(type()));
}
// convertTo of a CV_16SC1 map: saturate_cast<D>(short)
void GpuMat::convertTo(GpuMat &dst, int rtype, Stream &) const
{
    CV_Assert(type() == CV_16SC1);
    const int dd = rtype & 7;
    CV_Assert(dd == CV_8U || dd == CV_32S || dd == CV_32F);
    GpuMat out;
    out.create(rows, cols, CV_MAKETYPE(dd, 1));
    for (int y = 0; y < rows; ++y) {
        const short *s = ptr<short>(y);
        for (int x = 0; x < cols; ++x) {
            if (dd == CV_8U) out.ptr<unsigned char>(y)[x] = (unsigned char)std::min(std::max((int)s[x], 0), 255);
            else if (dd == CV_32S) out.ptr<int>(y)[x] = s[x];
            else out.ptr<float>(y)[x] = (float)s[x];
        }
    }
    dst = out;
}
}}

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
cv::Ptr<cv::cuda::StereoBeliefPropagation> make(int ndisp, int iters, int levels, int msg_type, const float *w)
{
    cv::Ptr<cv::cuda::StereoBeliefPropagation> bp = cv::cuda::createStereoBeliefPropagation(ndisp, iters, levels, msg_type);
    bp->setMaxDataTerm(w[0]); bp->setDataWeight(w[1]); bp->setMaxDiscTerm(w[2]); bp->setDiscSingleJump(w[3]);
    return bp;
}
}  // namespace

extern "C" {
/* left, right: dense rows x cols x cn bytes; w: max_data_term, data_weight, max_disc_term, disc_single_jump; disp: rows x cols of
 * out_type (CV_16SC1 = 3: the class's own choice; another type: handed over as a fixed-type output).  1 if the class threw. */
int sbp_ref_compute(const unsigned char *left, const unsigned char *right, int rows, int cols, int cn, int ndisp, int iters, int levels,
                    int msg_type, const float *w, int out_type, void *disp)
{
    try {
        GpuMat l = up(left, rows, cols, CV_MAKETYPE(CV_8U, cn)), r = up(right, rows, cols, CV_MAKETYPE(CV_8U, cn)), d;
        cv::cuda::Stream st;
        if (out_type != CV_16SC1) d.create(rows, cols, out_type);
        make(ndisp, iters, levels, msg_type, w)->compute(l, r, cv::_OutputArray(d, out_type != CV_16SC1), st);
        if (d.rows != rows || d.cols != cols || d.type() != out_type) return 2;
        down(d, disp);
        return 0;
    } catch (const std::exception &) { return 1; }
}
/* the same with mismatched images: right is rrows x rcols x rcn */
int sbp_ref_compute_mismatched(int rows, int cols, int cn, int rrows, int rcols, int rcn, int ndisp, int iters, int levels, int msg_type)
{
    try {
        GpuMat l(rows, cols, CV_MAKETYPE(CV_8U, cn)), r(rrows, rcols, CV_MAKETYPE(CV_8U, rcn)), d;
        const float w[4] = {10.0f, 0.07f, 1.7f, 1.0f};
        make(ndisp, iters, levels, msg_type, w)->compute(l, r, cv::_OutputArray(d));
        return 0;
    } catch (const std::exception &) { return 1; }
}
/* data: dense drows x cols of data_type */
int sbp_ref_compute_data(const void *data, int drows, int cols, int data_type, int ndisp, int iters, int levels, int msg_type, const float *w,
                         short *disp)
{
    try {
        GpuMat m = up(data, drows, cols, data_type), d;
        cv::cuda::Stream st;
        make(ndisp, iters, levels, msg_type, w)->compute(m, cv::_OutputArray(d), st);
        if (d.rows != drows / ndisp || d.cols != cols || d.type() != CV_16SC1) return 2;
        down(d, disp);
        return 0;
    } catch (const std::exception &) { return 1; }
}
void sbp_ref_estimate(int width, int height, int *ndisp, int *iters, int *levels)
{
    cv::cuda::StereoBeliefPropagation::estimateRecommendedParams(width, height, *ndisp, *iters, *levels);
}
}
