// cv::cuda::StereoBeliefPropagation: handle + C-ABI entry points.  Host-side twin of StereoBPImpl
// (modules/cudastereo/src/stereobp.cpp:78-378): validation, the plan (sbp_plan.h), scratch, and the plan's launches in order on the
// caller's stream, with no host wait in between.
#include "stereobp_dev.h"
#include <cmath>

using namespace mi;

struct mi_stereobp {
    mi_stereobp_params P;
    // scratch owned by the handle, grown on demand and reused (stereobp.cpp:142-144: u_ .. r_, u2_ .. r2_, datas_)
    DevBuf<unsigned char> set[2];   // message set s: u, d, l, r one behind the other
    DevBuf<unsigned char> data;     // the data-cost pyramid
};

namespace {

// load_constants' arguments, stereobp.cpp:176,271: the products in f32
sbp::BpConst consts_of(const mi_stereobp_params &P)
{
    const float scale = P.msg_type == sbp::SBP_MSG_32F ? 1.0f : 10.0f;
    return {P.ndisp, P.max_data_term, scale * P.data_weight, scale * P.max_disc_term, scale * P.disc_single_jump};
}

int elem_of(int type) { return type == MI_32FC1 || type == MI_32SC1 ? 4 : type == MI_16SC1 ? 2 : 1; }
int msg_mat_type(int msg_type) { return msg_type == sbp::SBP_MSG_32F ? MI_32FC1 : MI_16SC1; }

int check_mat(const mi_mat *m, const char *name)
{
    MI_REQUIRE(m && m->data, MI_ERR_BAD_ARG, "%s: null matrix", name);
    MI_REQUIRE(m->rows > 0 && m->cols > 0, MI_ERR_BAD_SIZE, "%s: empty", name);
    return MI_OK;
}

int image_channels(int type) { return type == MI_8UC1 ? 1 : type == MI_8UC3 ? 3 : type == MI_8UC4 ? 4 : 0; }

// a planar cost / message matrix of the reference: (ndisp * rows) x cols of T
int check_planar(const mi_mat *m, const char *name, int msg_type, int ndisp, int rows, int cols)
{
    MI_TRY(check_mat(m, name));
    MI_REQUIRE(m->type == msg_mat_type(msg_type), MI_ERR_BAD_TYPE, "%s: must be of the message type", name);
    const int e = elem_of(m->type);
    MI_REQUIRE(m->step % e == 0 && m->step >= (size_t)m->cols * e, MI_ERR_BAD_ARG, "%s: bad step", name);
    MI_REQUIRE((long long)m->rows == (long long)ndisp * rows && m->cols == cols, MI_ERR_BAD_SIZE, "%s: must be (ndisp * rows) x cols", name);
    return MI_OK;
}

int check_disp(const mi_mat *d, int rows, int cols)
{
    MI_TRY(check_mat(d, "disparity"));
    MI_REQUIRE(d->type == MI_16SC1 || d->type == MI_8UC1 || d->type == MI_32SC1 || d->type == MI_32FC1, MI_ERR_BAD_TYPE,
               "disparity: must be CV_16SC1, CV_8UC1, CV_32SC1 or CV_32FC1");
    MI_REQUIRE(d->rows == rows && d->cols == cols, MI_ERR_BAD_SIZE, "disparity.size() != left.size()");
    MI_REQUIRE(d->step >= (size_t)cols * elem_of(d->type) && d->step % elem_of(d->type) == 0, MI_ERR_BAD_ARG, "disparity: bad step");
    return MI_OK;
}

// four message matrices u, d, l, r of one level with one step
int msgs_of_mats(const mi_mat *m, int msg_type, int ndisp, int rows, int cols, sbp::BpMsgs *out)
{
    MI_REQUIRE(m, MI_ERR_BAD_ARG, "null messages");
    static const char *names[4] = {"u", "d", "l", "r"};
    for (int k = 0; k < 4; ++k) {
        MI_TRY(check_planar(&m[k], names[k], msg_type, ndisp, rows, cols));
        MI_REQUIRE(m[k].step == m[0].step, MI_ERR_BAD_ARG, "the four messages must have one step");
    }
    *out = {m[0].data, m[1].data, m[2].data, m[3].data, (long long)(m[0].step / elem_of(m[0].type))};
    return MI_OK;
}

sbp::BpMsgs level_msgs(mi_stereobp *h, const sbp::SbpPlan &plan, int level)
{
    const sbp::SbpLevel &L = plan.lv[level];
    const size_t one = plan.set_elems[L.set] * plan.elem;
    unsigned char *b = h->set[L.set].p;
    return {b, b + one, b + 2 * one, b + 3 * one, L.pitch};
}

// calcBP, stereobp.cpp:282-359.  data0 / dstep0: the caller's cost volume (compute_data) or null (level 0 lives in the scratch).
int run(mi_stereobp *h, const sbp::SbpPlan &plan, const mi_mat *left, const mi_mat *right, const void *data0, long long dstep0,
        mi_mat *disp, hipStream_t st)
{
    const sbp::BpConst c = consts_of(h->P);
    for (int s = 0; s < 2; ++s) MI_TRY(h->set[s].ensure(4 * plan.set_elems[s] * plan.elem));
    MI_TRY(h->data.ensure(plan.data_elems * plan.elem));
    const auto data_of = [&](int level, long long *step) -> void * {
        if (level == 0 && data0) { *step = dstep0; return const_cast<void *>(data0); }
        *step = plan.lv[level].pitch;
        return h->data.p + plan.lv[level].data_off * plan.elem;
    };
    for (const sbp::SbpLaunch &k : plan.launches) {
        const sbp::SbpLevel &L = plan.lv[k.level];
        long long dstep = 0, sstep = 0;
        void *dt = data_of(k.level, &dstep);
        switch (k.kernel) {
        case sbp::SBP_K_COMP_DATA:
            MI_TRY(sbp::comp_data(plan.msg_type, plan.channels, (const unsigned char *)left->data, (long long)left->step,
                                  (const unsigned char *)right->data, (long long)right->step, dt, dstep, L.rows, L.cols, c, st));
            break;
        case sbp::SBP_K_STEP_DOWN: {
            const sbp::SbpLevel &S = plan.lv[k.level - 1];
            const void *src = data_of(k.level - 1, &sstep);
            MI_TRY(sbp::data_step_down(plan.msg_type, src, sstep, S.rows, S.cols, dt, dstep, L.rows, L.cols, plan.ndisp, st));
            break;
        }
        case sbp::SBP_K_ZERO: {   // of the coarsest level's planes only: that is all any kernel reads of the zeroed set
            const sbp::BpMsgs m = level_msgs(h, plan, k.level);
            const size_t bytes = (size_t)plan.ndisp * L.rows * L.pitch * plan.elem;
            for (void *p : {m.u, m.d, m.l, m.r}) MI_HIP_TRY(hipMemsetAsync(p, 0, bytes, st));
            break;
        }
        case sbp::SBP_K_LEVEL_UP:
            MI_TRY(sbp::level_up(plan.msg_type, level_msgs(h, plan, k.level + 1), plan.lv[k.level + 1].rows, level_msgs(h, plan, k.level),
                                 L.rows, L.cols, plan.ndisp, st));
            break;
        case sbp::SBP_K_ITERATE:
            MI_TRY(sbp::iterate(plan.msg_type, k.form, plan.cap, level_msgs(h, plan, k.level), dt, dstep, L.rows, L.cols, k.t, c, st));
            break;
        case sbp::SBP_K_OUTPUT:
            MI_TRY(sbp::output(plan.msg_type, level_msgs(h, plan, 0), dt, dstep, L.rows, L.cols, plan.ndisp, disp->data, (long long)disp->step,
                               disp->type, st));
            break;
        }
    }
    return MI_OK;
}

}  // namespace

extern "C" {

void mi_stereobp_default_params(mi_stereobp_params *p)
{
    if (!p) return;
    // createStereoBeliefPropagation(64, 5, 5, CV_32F) cudastereo.hpp:189; StereoBPImpl ctor + DEFAULT_* stereobp.cpp:147-158
    p->ndisp = 64; p->iters = 5; p->levels = 5;
    p->max_data_term = 10.0f; p->data_weight = 0.07f; p->max_disc_term = 1.7f; p->disc_single_jump = 1.0f;
    p->msg_type = sbp::SBP_MSG_32F;
}

int mi_stereobp_create(const mi_stereobp_params *p, mi_stereobp **out)
{
    MI_REQUIRE(out, MI_ERR_BAD_ARG, "null out");
    *out = nullptr;
    MI_TRY(require_device());
    mi_stereobp *h = new mi_stereobp();
    if (p) h->P = *p; else mi_stereobp_default_params(&h->P);
    *out = h;
    return MI_OK;
}

int mi_stereobp_set_params(mi_stereobp *h, const mi_stereobp_params *p)
{
    MI_REQUIRE(h && p, MI_ERR_BAD_ARG, "null argument");
    h->P = *p;   // like the reference's setters: validated at compute() (stereobp.cpp:178-180)
    return MI_OK;
}

int mi_stereobp_get_params(const mi_stereobp *h, mi_stereobp_params *p)
{
    MI_REQUIRE(h && p, MI_ERR_BAD_ARG, "null argument");
    *p = h->P;
    return MI_OK;
}

void mi_stereobp_destroy(mi_stereobp *h)
{
    delete h;
}

int mi_stereobp_scratch_bytes(const mi_stereobp *h, size_t *bytes)
{
    MI_REQUIRE(h && bytes, MI_ERR_BAD_ARG, "null argument");
    *bytes = h->set[0].n + h->set[1].n + h->data.n;
    return MI_OK;
}

int mi_stereobp_compute(mi_stereobp *h, const mi_mat *left, const mi_mat *right, mi_mat *disp, void *stream)
{
    MI_REQUIRE(h, MI_ERR_BAD_ARG, "null handle");
    const mi_stereobp_params &P = h->P;
    MI_TRY(sbp::sbp_fail(sbp::sbp_check_params(P.ndisp, P.iters, P.levels, P.msg_type, P.max_data_term)));
    MI_TRY(check_mat(left, "left")); MI_TRY(check_mat(right, "right"));
    const int cn = image_channels(left->type);
    MI_REQUIRE(cn, MI_ERR_BAD_TYPE, "left.type() == CV_8UC1 || left.type() == CV_8UC3 || left.type() == CV_8UC4");   // stereobp.cpp:185
    MI_REQUIRE(left->rows == right->rows && left->cols == right->cols && left->type == right->type, MI_ERR_BAD_SIZE,
               "left.size() == right.size() && left.type() == right.type()");                                      // :186
    MI_REQUIRE(left->step >= (size_t)left->cols * cn && right->step >= (size_t)right->cols * cn, MI_ERR_BAD_ARG, "step < cols * channels");
    const sbp::SbpPlan plan = sbp::sbp_make_plan(left->rows, left->cols, P.ndisp, P.iters, P.levels, P.msg_type, cn, P.max_data_term);
    MI_TRY(sbp::sbp_fail(plan.err));
    MI_TRY(check_disp(disp, left->rows, left->cols));
    return run(h, plan, left, right, nullptr, 0, disp, (hipStream_t)stream);
}

int mi_stereobp_compute_data(mi_stereobp *h, const mi_mat *data, mi_mat *disp, void *stream)
{
    MI_REQUIRE(h, MI_ERR_BAD_ARG, "null handle");
    const mi_stereobp_params &P = h->P;
    MI_TRY(sbp::sbp_fail(sbp::sbp_check_params(P.ndisp, P.iters, P.levels, P.msg_type, P.max_data_term)));
    MI_TRY(check_mat(data, "data"));
    MI_REQUIRE(data->type == msg_mat_type(P.msg_type) && data->rows % P.ndisp == 0, MI_ERR_BAD_ARG,
               "%s", "(data.type() == msg_type_) && (data.rows % ndisp_ == 0)");   // stereobp.cpp:216
    const int rows = data->rows / P.ndisp, cols = data->cols, e = elem_of(data->type);
    MI_REQUIRE(data->step % e == 0 && data->step >= (size_t)cols * e, MI_ERR_BAD_ARG, "data: bad step");
    const sbp::SbpPlan plan = sbp::sbp_make_plan(rows, cols, P.ndisp, P.iters, P.levels, P.msg_type, 0, P.max_data_term);
    MI_TRY(sbp::sbp_fail(plan.err));
    MI_TRY(check_disp(disp, rows, cols));
    // the reference copies the volume into datas_[0] (:229); nothing writes level 0, so it is read where it lies
    return run(h, plan, nullptr, nullptr, data->data, (long long)(data->step / e), disp, (hipStream_t)stream);
}

int mi_stereobp_estimate_recommended_params(int width, int height, int *ndisp, int *iters, int *levels)
{
    MI_REQUIRE(ndisp && iters && levels, MI_ERR_BAD_ARG, "null argument");
    MI_REQUIRE(width > 0 && height > 0, MI_ERR_BAD_SIZE, "empty image");
    sbp::sbp_estimate(width, height, std::log((double)(width > height ? width : height)), ndisp, iters, levels);
    return MI_OK;
}

// ---- stage-level entry points: the reference's device-layer functions (stereobp.cpp:60-72) on the reference's planar matrices
int mi_stereobp_comp_data(const mi_stereobp_params *p, const mi_mat *left, const mi_mat *right, mi_mat *data, void *stream)
{
    MI_REQUIRE(p, MI_ERR_BAD_ARG, "null argument");
    MI_TRY(sbp::sbp_fail(sbp::sbp_check_params(p->ndisp, 1, 1, p->msg_type, 0.f)));
    MI_TRY(check_mat(left, "left")); MI_TRY(check_mat(right, "right"));
    const int cn = image_channels(left->type);
    MI_REQUIRE(cn, MI_ERR_BAD_TYPE, "left.type() == CV_8UC1 || left.type() == CV_8UC3 || left.type() == CV_8UC4");
    MI_REQUIRE(left->rows == right->rows && left->cols == right->cols && left->type == right->type, MI_ERR_BAD_SIZE,
               "left.size() == right.size() && left.type() == right.type()");
    MI_REQUIRE(left->step >= (size_t)left->cols * cn && right->step >= (size_t)right->cols * cn, MI_ERR_BAD_ARG, "step < cols * channels");
    MI_TRY(check_planar(data, "data", p->msg_type, p->ndisp, left->rows, left->cols));
    return sbp::comp_data(p->msg_type, cn, (const unsigned char *)left->data, (long long)left->step, (const unsigned char *)right->data,
                          (long long)right->step, data->data, (long long)(data->step / elem_of(data->type)), left->rows, left->cols,
                          consts_of(*p), (hipStream_t)stream);
}

static int msg_type_of(const mi_mat *m, const char *name, int *msg_type)
{
    MI_TRY(check_mat(m, name));
    MI_REQUIRE(m->type == MI_16SC1 || m->type == MI_32FC1, MI_ERR_BAD_TYPE, "%s: must be CV_16SC1 or CV_32FC1", name);
    *msg_type = m->type == MI_32FC1 ? sbp::SBP_MSG_32F : sbp::SBP_MSG_16S;
    return MI_OK;
}

int mi_stereobp_data_step_down(const mi_mat *src, mi_mat *dst, int ndisp, void *stream)
{
    int mt;
    MI_TRY(msg_type_of(src, "src", &mt));
    MI_REQUIRE(ndisp > 0 && src->rows % ndisp == 0, MI_ERR_BAD_ARG, "%s", "src.rows % ndisp == 0");
    const int srows = src->rows / ndisp, drows = (srows + 1) / 2, dcols = (src->cols + 1) / 2;
    MI_TRY(check_planar(src, "src", mt, ndisp, srows, src->cols));
    MI_TRY(check_planar(dst, "dst", mt, ndisp, drows, dcols));
    const int e = elem_of(src->type);
    return sbp::data_step_down(mt, src->data, (long long)(src->step / e), srows, src->cols, dst->data, (long long)(dst->step / e), drows, dcols,
                               ndisp, (hipStream_t)stream);
}

int mi_stereobp_level_up(const mi_mat *src_udlr, mi_mat *dst_udlr, int ndisp, void *stream)
{
    MI_REQUIRE(src_udlr && dst_udlr, MI_ERR_BAD_ARG, "null messages");
    int mt;
    MI_TRY(msg_type_of(&src_udlr[0], "u", &mt));
    MI_TRY(check_mat(&dst_udlr[0], "u"));
    MI_REQUIRE(ndisp > 0 && src_udlr[0].rows % ndisp == 0 && dst_udlr[0].rows % ndisp == 0, MI_ERR_BAD_ARG, "%s", "rows % ndisp == 0");
    const int srows = src_udlr[0].rows / ndisp, drows = dst_udlr[0].rows / ndisp, dcols = dst_udlr[0].cols;
    MI_REQUIRE(srows == (drows + 1) / 2 && src_udlr[0].cols == (dcols + 1) / 2, MI_ERR_BAD_SIZE, "src must be the next coarser level of dst");
    sbp::BpMsgs s, d;
    MI_TRY(msgs_of_mats(src_udlr, mt, ndisp, srows, src_udlr[0].cols, &s));
    MI_TRY(msgs_of_mats(dst_udlr, mt, ndisp, drows, dcols, &d));
    return sbp::level_up(mt, s, srows, d, drows, dcols, ndisp, (hipStream_t)stream);
}

int mi_stereobp_iterate(const mi_stereobp_params *p, mi_mat *udlr, const mi_mat *data, int t0, int n_iters, int form, void *stream)
{
    MI_REQUIRE(p && udlr, MI_ERR_BAD_ARG, "null argument");
    MI_TRY(sbp::sbp_fail(sbp::sbp_check_params(p->ndisp, 1, 1, p->msg_type, 0.f)));
    MI_REQUIRE(t0 >= 0 && n_iters >= 0, MI_ERR_BAD_ARG, "t0 >= 0 && n_iters >= 0");
    MI_TRY(check_mat(data, "data"));
    MI_REQUIRE(data->rows % p->ndisp == 0, MI_ERR_BAD_ARG, "%s", "data.rows % ndisp == 0");
    const int rows = data->rows / p->ndisp, cols = data->cols;
    MI_TRY(check_planar(data, "data", p->msg_type, p->ndisp, rows, cols));
    sbp::BpMsgs m;
    MI_TRY(msgs_of_mats(udlr, p->msg_type, p->ndisp, rows, cols, &m));
    // the plan's form rule (and its rejection of a register form beyond its capacities); the level geometry is the caller's
    const int cap = sbp::sbp_reg_cap(p->ndisp);
    if (form == sbp::SBP_FORM_AUTO) form = cap ? sbp::SBP_FORM_REG : sbp::SBP_FORM_GEN;
    MI_REQUIRE(form == sbp::SBP_FORM_GEN || (form == sbp::SBP_FORM_REG && cap), MI_ERR_BAD_ARG, "form: the register form holds at most 64 disparities");
    const sbp::BpConst c = consts_of(*p);
    for (int t = t0; t < t0 + n_iters; ++t)
        MI_TRY(sbp::iterate(p->msg_type, form, form == sbp::SBP_FORM_REG ? cap : 0, m, data->data, (long long)(data->step / elem_of(data->type)),
                            rows, cols, t, c, (hipStream_t)stream));
    return MI_OK;
}

int mi_stereobp_output(const mi_mat *udlr, const mi_mat *data, int ndisp, mi_mat *disp, void *stream)
{
    int mt;
    MI_TRY(msg_type_of(data, "data", &mt));
    MI_REQUIRE(ndisp > 0 && data->rows % ndisp == 0, MI_ERR_BAD_ARG, "%s", "data.rows % ndisp == 0");
    const int rows = data->rows / ndisp, cols = data->cols;
    MI_TRY(check_planar(data, "data", mt, ndisp, rows, cols));
    sbp::BpMsgs m;
    MI_TRY(msgs_of_mats(const_cast<mi_mat *>(udlr), mt, ndisp, rows, cols, &m));
    MI_TRY(check_disp(disp, rows, cols));
    return sbp::output(mt, m, data->data, (long long)(data->step / elem_of(data->type)), rows, cols, ndisp, disp->data, (long long)disp->step,
                       disp->type, (hipStream_t)stream);
}

}  // extern "C"
