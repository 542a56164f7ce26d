/* tools/stereobp_ref/sbp_ref_stage.cpp -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.
 * C entry points over the kernel wrappers of the reference's modules/cudastereo/src/cuda/stereobp.cu (rewritten only at its launch sites
 * by oracle/refshim/cu2host.py and run on the CPU through oracle/refshim/cudashim), each on its own, called the way the host class calls
 * them (modules/cudastereo/src/stereobp.cpp:60-72).  Dense matrices, step = cols * element size. */
#include "opencv2/core/cuda/common.hpp"

namespace cv { namespace cuda { namespace device { namespace stereobp {
void load_constants(int ndisp, float max_data_term, float data_weight, float max_disc_term, float disc_single_jump);
template <typename T, typename D> void comp_data_gpu(const PtrStepSzb &left, const PtrStepSzb &right, const PtrStepSzb &data, cudaStream_t stream);
template <typename T> void data_step_down_gpu(int dst_cols, int dst_rows, int src_cols, int src_rows, const PtrStepSzb &src, const PtrStepSzb &dst, cudaStream_t stream);
template <typename T> void level_up_messages_gpu(int dst_idx, int dst_cols, int dst_rows, int src_rows, PtrStepSzb *mus, PtrStepSzb *mds, PtrStepSzb *mls, PtrStepSzb *mrs, cudaStream_t stream);
template <typename T> void calc_all_iterations_gpu(int cols, int rows, int iters, const PtrStepSzb &u, const PtrStepSzb &d, const PtrStepSzb &l, const PtrStepSzb &r, const PtrStepSzb &data, cudaStream_t stream);
template <typename T> void output_gpu(const PtrStepSzb &u, const PtrStepSzb &d, const PtrStepSzb &l, const PtrStepSzb &r, const PtrStepSzb &data, const PtrStepSz<short> &disp, cudaStream_t stream);
}}}}

using namespace cv::cuda;
namespace bp = cv::cuda::device::stereobp;

namespace {
PtrStepSzb mat(const void *p, int rows, int cols, int elem) { return PtrStepSzb(rows, cols, (unsigned char *)p, (size_t)cols * elem); }
}

extern "C" {
/* f32: 1 = float messages, 0 = short; planar matrices are (ndisp * rows) x cols */
void sbp_ref_load_constants(int ndisp, float max_data_term, float data_weight, float max_disc_term, float disc_single_jump)
{
    bp::load_constants(ndisp, max_data_term, data_weight, max_disc_term, disc_single_jump);
}
int sbp_ref_comp_data(const unsigned char *left, const unsigned char *right, int rows, int cols, int cn, int f32, int ndisp, void *data)
{
    const PtrStepSzb l = mat(left, rows, cols, cn), r = mat(right, rows, cols, cn), d = mat(data, rows * ndisp, cols, f32 ? 4 : 2);
    // PtrStepSzb of an image: cols counts pixels (GpuMat's conversion), the step carries the channels
    const PtrStepSzb lp(rows, cols, l.data, l.step), rp(rows, cols, r.data, r.step);
    if (cn == 1) { if (f32) bp::comp_data_gpu<unsigned char, float>(lp, rp, d, 0); else bp::comp_data_gpu<unsigned char, short>(lp, rp, d, 0); }
    else if (cn == 3) { if (f32) bp::comp_data_gpu<uchar3, float>(lp, rp, d, 0); else bp::comp_data_gpu<uchar3, short>(lp, rp, d, 0); }
    else if (cn == 4) { if (f32) bp::comp_data_gpu<uchar4, float>(lp, rp, d, 0); else bp::comp_data_gpu<uchar4, short>(lp, rp, d, 0); }
    else return 1;
    return 0;
}
int sbp_ref_step_down(int f32, int ndisp, const void *src, int src_rows, int src_cols, void *dst, int dst_rows, int dst_cols)
{
    const int e = f32 ? 4 : 2;
    const PtrStepSzb s = mat(src, src_rows * ndisp, src_cols, e), d = mat(dst, dst_rows * ndisp, dst_cols, e);
    if (f32) bp::data_step_down_gpu<float>(dst_cols, dst_rows, src_cols, src_rows, s, d, 0);
    else bp::data_step_down_gpu<short>(dst_cols, dst_rows, src_cols, src_rows, s, d, 0);
    return 0;
}
/* src / dst: four matrices u, d, l, r one behind the other */
int sbp_ref_level_up(int f32, int ndisp, const void *src, int src_rows, int src_cols, void *dst, int dst_rows, int dst_cols)
{
    const int e = f32 ? 4 : 2;
    const size_t sn = (size_t)src_rows * ndisp * src_cols * e, dn = (size_t)dst_rows * ndisp * dst_cols * e;
    PtrStepSzb m[4][2];
    for (int k = 0; k < 4; ++k) {
        m[k][0] = mat((unsigned char *)dst + k * dn, dst_rows * ndisp, dst_cols, e);   // dst_idx = 0
        m[k][1] = mat((const unsigned char *)src + k * sn, src_rows * ndisp, src_cols, e);
    }
    if (f32) bp::level_up_messages_gpu<float>(0, dst_cols, dst_rows, src_rows, m[0], m[1], m[2], m[3], 0);
    else bp::level_up_messages_gpu<short>(0, dst_cols, dst_rows, src_rows, m[0], m[1], m[2], m[3], 0);
    return 0;
}
/* msgs: u, d, l, r one behind the other, updated in place */
int sbp_ref_iterations(int f32, int ndisp, void *msgs, const void *data, int rows, int cols, int iters)
{
    const int e = f32 ? 4 : 2;
    const size_t n = (size_t)rows * ndisp * cols * e;
    unsigned char *b = (unsigned char *)msgs;
    const PtrStepSzb u = mat(b, rows * ndisp, cols, e), d = mat(b + n, rows * ndisp, cols, e), l = mat(b + 2 * n, rows * ndisp, cols, e),
                     r = mat(b + 3 * n, rows * ndisp, cols, e), dt = mat(data, rows * ndisp, cols, e);
    if (f32) bp::calc_all_iterations_gpu<float>(cols, rows, iters, u, d, l, r, dt, 0);
    else bp::calc_all_iterations_gpu<short>(cols, rows, iters, u, d, l, r, dt, 0);
    return 0;
}
int sbp_ref_output(int f32, int ndisp, const void *msgs, const void *data, int rows, int cols, short *disp)
{
    const int e = f32 ? 4 : 2;
    const size_t n = (size_t)rows * ndisp * cols * e;
    const unsigned char *b = (const unsigned char *)msgs;
    const PtrStepSzb u = mat(b, rows * ndisp, cols, e), d = mat(b + n, rows * ndisp, cols, e), l = mat(b + 2 * n, rows * ndisp, cols, e),
                     r = mat(b + 3 * n, rows * ndisp, cols, e), dt = mat(data, rows * ndisp, cols, e);
    const PtrStepSz<short> o(rows, cols, disp, (size_t)cols * 2);
    if (f32) bp::output_gpu<float>(u, d, l, r, dt, o, 0);
    else bp::output_gpu<short>(u, d, l, r, dt, o, 0);
    return 0;
}
}
