/* tools/stereocsbp_ref/csbp_ref_stage.cpp -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.
 * C entry points over the kernel wrappers of the reference's modules/cudastereo/src/cuda/stereocsbp.cu (rewritten only at its launch
 * sites by oracle/refshim/cu2host.py and run on the CPU through oracle/refshim/cudashim), each on its own, called the way the host class
 * calls them (modules/cudastereo/src/stereocsbp.cpp:246-324).  Matrices arrive dense, (planes * level rows) x level cols.  The wrappers
 * take ONE msg_step for a level and its parent, so the parent's matrices are copied into matrices of the level's step first. */
#include <cstring>
#include <vector>
#include "opencv2/core/cuda/common.hpp"
#include "cuda/stereocsbp.hpp"

using namespace cv::cuda;
namespace cs = cv::cuda::device::stereocsbp;

namespace {
/* dense (rows x cols) -> rows of `step` elements */
template <typename T> std::vector<T> widen(const void *p, int rows, int cols, int step)
{
    std::vector<T> v((size_t)rows * step + step, T(0));
    for (int y = 0; y < rows; ++y) memcpy(&v[(size_t)y * step], (const T *)p + (size_t)y * cols, (size_t)cols * sizeof(T));
    return v;
}

template <typename T>
void init_data_cost_t(const unsigned char *left, const unsigned char *right, int rows, int cols, int cn, int level, int nr_plane, int ndisp,
                      const float *w, int min_disp, int local, void *sel_cost, void *sel_disp)
{
    const int h = rows >> level, wd = cols >> level;
    std::vector<T> temp((size_t)(ndisp + 1) * h * wd, T(0));   /* + 1: the local form reads plane 2 when ndisp == 2 */
    cs::init_data_cost<T>(left, right, (unsigned char *)temp.data(), (size_t)cols * cn, rows, cols, (T *)sel_disp, (T *)sel_cost, wd, h, wd, level,
                          nr_plane, ndisp, cn, w[1], w[0], min_disp, local != 0, 0);
}

template <typename T>
void compute_data_cost_t(const unsigned char *left, const unsigned char *right, int rows, int cols, int cn, int level, int n2, const float *w,
                         int min_disp, const void *disp_parent, void *data_cost)
{
    const int h = rows >> level, wd = cols >> level, h2 = h / 2, w2 = wd / 2;
    const std::vector<T> dp = widen<T>(disp_parent, n2 * h2, w2, wd);
    cs::compute_data_cost<T>(left, right, (size_t)cols * cn, dp.data(), (T *)data_cost, wd, rows, cols, h, wd, h2, level, n2, cn, w[1], w[0], min_disp, 0);
}

template <typename T>
void init_message_t(const void *cur, void *nw, const void *data_cost, void *sel_cost, int h, int w, int n, int n2)
{
    const int h2 = h / 2, w2 = w / 2;
    const size_t cn = (size_t)n2 * h2 * w2, nn = (size_t)n * h * w;
    std::vector<T> c[5];
    for (int k = 0; k < 5; ++k) c[k] = widen<T>((const T *)cur + k * cn, n2 * h2, w2, w);
    std::vector<T> temp((size_t)n2 * h * w, T(0));
    T *o = (T *)nw;
    cs::init_message<T>((unsigned char *)temp.data(), o, o + nn, o + 2 * nn, o + 3 * nn, c[0].data(), c[1].data(), c[2].data(), c[3].data(), o + 4 * nn,
                        c[4].data(), (T *)sel_cost, (const T *)data_cost, w, h, w, n, h2, w2, n2, 0);
}

template <typename T>
void iterations_t(void *msgs, const void *sel_disp, const void *sel_cost, int h, int w, int n, int iters, int max_disc_term, float jump)
{
    const size_t nn = (size_t)n * h * w;
    std::vector<T> temp(nn, T(0));
    T *m = (T *)msgs;
    cs::calc_all_iterations<T>((unsigned char *)temp.data(), m, m + nn, m + 2 * nn, m + 3 * nn, (const T *)sel_cost, (const T *)sel_disp, w, h, w, n, iters,
                               max_disc_term, jump, 0);
}

template <typename T>
void compute_disp_t(const void *msgs, const void *sel_disp, const void *sel_cost, int rows, int cols, int n, short *disp)
{
    const size_t nn = (size_t)n * rows * cols;
    const T *m = (const T *)msgs;
    cs::compute_disp<T>(m, m + nn, m + 2 * nn, m + 3 * nn, (const T *)sel_cost, (const T *)sel_disp, cols, PtrStepSz<short>(rows, cols, disp, (size_t)cols * 2), n, 0);
}
}  // namespace

extern "C" {
/* f32: 1 = float messages, 0 = short.  w: max_data_term, data_weight.  Images dense, rows x cols x cn. */
void csbp_ref_init_data_cost(int f32, const unsigned char *left, const unsigned char *right, int rows, int cols, int cn, int level, int nr_plane,
                             int ndisp, const float *w, int min_disp, int local, void *sel_cost, void *sel_disp)
{
    if (f32) init_data_cost_t<float>(left, right, rows, cols, cn, level, nr_plane, ndisp, w, min_disp, local, sel_cost, sel_disp);
    else init_data_cost_t<short>(left, right, rows, cols, cn, level, nr_plane, ndisp, w, min_disp, local, sel_cost, sel_disp);
}
void csbp_ref_compute_data_cost(int f32, const unsigned char *left, const unsigned char *right, int rows, int cols, int cn, int level, int n2,
                                const float *w, int min_disp, const void *disp_parent, void *data_cost)
{
    if (f32) compute_data_cost_t<float>(left, right, rows, cols, cn, level, n2, w, min_disp, disp_parent, data_cost);
    else compute_data_cost_t<short>(left, right, rows, cols, cn, level, n2, w, min_disp, disp_parent, data_cost);
}
/* cur: u, d, l, r, disp_selected of the parent level ((n2 * h / 2) x (w / 2) each) one behind the other; nw: the five of the level */
void csbp_ref_init_message(int f32, const void *cur, void *nw, const void *data_cost, void *sel_cost, int h, int w, int n, int n2)
{
    if (f32) init_message_t<float>(cur, nw, data_cost, sel_cost, h, w, n, n2);
    else init_message_t<short>(cur, nw, data_cost, sel_cost, h, w, n, n2);
}
/* msgs: u, d, l, r one behind the other, updated in place; half-sweeps t = 0 .. iters - 1 */
void csbp_ref_iterations(int f32, void *msgs, const void *sel_disp, const void *sel_cost, int h, int w, int n, int iters, int max_disc_term, float jump)
{
    if (f32) iterations_t<float>(msgs, sel_disp, sel_cost, h, w, n, iters, max_disc_term, jump);
    else iterations_t<short>(msgs, sel_disp, sel_cost, h, w, n, iters, max_disc_term, jump);
}
/* disp: rows x cols shorts, zeroed by the caller as the class does */
void csbp_ref_compute_disp(int f32, const void *msgs, const void *sel_disp, const void *sel_cost, int rows, int cols, int n, short *disp)
{
    if (f32) compute_disp_t<float>(msgs, sel_disp, sel_cost, rows, cols, n, disp);
    else compute_disp_t<short>(msgs, sel_disp, sel_cost, rows, cols, n, disp);
}
}
