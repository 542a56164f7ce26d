// cv::cuda::StereoConstantSpaceBP: handle + C-ABI entry points.  Host-side twin of StereoCSBPImpl
// (modules/cudastereo/src/stereocsbp.cpp:60-355): validation, the plan (scsbp_plan.h), scratch, and the plan's launches in order on the
// caller's stream, with no host wait in between.
#include "stereocsbp_dev.h"
#include "mi_buf.h"

using namespace mi;

struct mi_stereocsbp {
    mi_stereocsbp_params P;
    // scratch owned by the handle, grown on demand and reused (stereocsbp.cpp:127-129: mbuf_, temp_)
    DevBuf<unsigned char> set[2];   // set s: u, d, l, r, disp_selected one behind the other
    DevBuf<unsigned char> cost;     // data_cost
    DevBuf<unsigned char> sel;      // data_cost_selected
    DevBuf<unsigned char> temp;     // temp_
};

namespace {

// stereocsbp.cpp:266-268: calc_all_iterations takes max_disc_term as int, the float is truncated toward zero at the call
int trunc_int(float v) { return v >= 2147483648.0f ? 2147483647 : v <= -2147483648.0f ? (-2147483647 - 1) : (int)v; }
scsbp::CsbpConst consts_of(const mi_stereocsbp_params &P)
{
    return {P.max_data_term, P.data_weight, P.min_disp_th, trunc_int(P.max_disc_term), P.disc_single_jump};
}

int elem_of(int type) { return type == MI_32FC1 || type == MI_32SC1 ? 4 : type == MI_16SC1 ? 2 : 1; }
int msg_mat_type(int msg_type) { return msg_type == scsbp::CSBP_MSG_32F ? MI_32FC1 : MI_16SC1; }
int image_channels(int type) { return type == MI_8UC1 ? 1 : type == MI_8UC3 ? 3 : type == MI_8UC4 ? 4 : 0; }

int check_mat(const mi_mat *m, const char *name)
{
    MI_REQUIRE(m && m->data, MI_ERR_BAD_ARG, "%s: null matrix", name);
    MI_REQUIRE(m->rows > 0 && m->cols > 0, MI_ERR_BAD_SIZE, "%s: empty", name);
    return MI_OK;
}

int check_msg_type(int msg_type)
{
    MI_REQUIRE(msg_type == scsbp::CSBP_MSG_32F || msg_type == scsbp::CSBP_MSG_16S, MI_ERR_BAD_ARG, "%s", "msg_type_ == CV_32F || msg_type_ == CV_16S");
    return MI_OK;
}

// stereocsbp.cpp:160-161
int check_images(const mi_mat *left, const mi_mat *right, scsbp::CsbpImages *im)
{
    MI_TRY(check_mat(left, "left")); MI_TRY(check_mat(right, "right"));
    const int cn = image_channels(left->type);
    MI_REQUIRE(cn, MI_ERR_BAD_TYPE, "left.type() == CV_8UC1 || left.type() == CV_8UC3 || left.type() == CV_8UC4");
    MI_REQUIRE(left->rows == right->rows && left->cols == right->cols && left->type == right->type, MI_ERR_BAD_SIZE,
               "left.size() == right.size() && left.type() == right.type()");
    MI_REQUIRE(left->step >= (size_t)left->cols * cn && right->step >= (size_t)right->cols * cn, MI_ERR_BAD_ARG, "step < cols * channels");
    *im = {(const unsigned char *)left->data, (const unsigned char *)right->data, (long long)left->step, (long long)right->step, left->rows,
           left->cols, cn};
    return MI_OK;
}

// a planar matrix of the reference: (planes * rows) x cols of T
int check_planar(const mi_mat *m, const char *name, int msg_type, int planes, int rows, int cols)
{
    MI_TRY(check_mat(m, name));
    MI_REQUIRE(m->type == msg_mat_type(msg_type), MI_ERR_BAD_TYPE, "%s: must be of the message type", name);
    const int e = elem_of(m->type);
    MI_REQUIRE(m->step % e == 0 && m->step >= (size_t)m->cols * e, MI_ERR_BAD_ARG, "%s: bad step", name);
    MI_REQUIRE((long long)m->rows == (long long)planes * rows && m->cols == cols, MI_ERR_BAD_SIZE, "%s: must be (%d * %d) x %d", name, planes, rows, cols);
    return MI_OK;
}

int msg_type_of(const mi_mat *m, const char *name, int *msg_type)
{
    MI_TRY(check_mat(m, name));
    MI_REQUIRE(m->type == MI_16SC1 || m->type == MI_32FC1, MI_ERR_BAD_TYPE, "%s: must be CV_16SC1 or CV_32FC1", name);
    *msg_type = m->type == MI_32FC1 ? scsbp::CSBP_MSG_32F : scsbp::CSBP_MSG_16S;
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

// k matrices (u, d, l, r[, disp_selected]) of one level with one step; step != 0: the step (in bytes) they must have
int set_of_mats(const mi_mat *m, int k, int msg_type, int planes, int rows, int cols, size_t step, scsbp::CsbpSet *out)
{
    MI_REQUIRE(m, MI_ERR_BAD_ARG, "null messages");
    static const char *names[5] = {"u", "d", "l", "r", "disp_selected"};
    for (int i = 0; i < k; ++i) {
        MI_TRY(check_planar(&m[i], names[i], msg_type, planes, rows, cols));
        MI_REQUIRE(m[i].step == (step ? step : m[0].step), MI_ERR_BAD_ARG, "the matrices of a level must have one step");
    }
    *out = {m[0].data, m[1].data, m[2].data, m[3].data, k > 4 ? m[4].data : nullptr, (long long)(m[0].step / elem_of(m[0].type))};
    return MI_OK;
}

scsbp::CsbpSet level_set(mi_stereocsbp *h, const scsbp::CsbpPlan &plan, int level)
{
    const scsbp::CsbpLevel &L = plan.lv[level];
    const size_t one = plan.set_elems[L.set] * plan.elem;
    unsigned char *b = h->set[L.set].p;
    return {b, b + one, b + 2 * one, b + 3 * one, b + 4 * one, L.pitch};
}

// stereocsbp.cpp:225-325
int run(mi_stereocsbp *h, const scsbp::CsbpPlan &plan, const scsbp::CsbpImages &im, mi_mat *disp, hipStream_t st)
{
    const scsbp::CsbpConst c = consts_of(h->P);
    for (int s = 0; s < 2; ++s) MI_TRY(h->set[s].ensure(5 * plan.set_elems[s] * plan.elem));
    MI_TRY(h->cost.ensure(plan.cost_elems * plan.elem));
    MI_TRY(h->sel.ensure(plan.sel_elems * plan.elem));
    MI_TRY(h->temp.ensure(plan.temp_elems * plan.elem));
    for (const scsbp::CsbpLaunch &k : plan.launches) {
        const scsbp::CsbpLevel &L = plan.lv[k.level];
        const scsbp::CsbpSet m = level_set(h, plan, k.level);
        switch (k.kernel) {
        case scsbp::CSBP_K_ZERO:   // both sets, whole: reads past a level with odd sizes land in them (scsbp_plan.h, set_elems)
            for (int s = 0; s < 2; ++s) MI_HIP_TRY(hipMemsetAsync(h->set[s].p, 0, 5 * plan.set_elems[s] * plan.elem, st));
            break;
        case scsbp::CSBP_K_INIT_DATA_COST:
            MI_TRY(scsbp::data_cost(plan.msg_type, im, nullptr, 0, 0, h->temp.p, L.pitch, L.rows, L.cols, k.level, plan.ndisp, c, st));
            break;
        case scsbp::CSBP_K_FIRST_K:
            MI_TRY(scsbp::first_k(plan.msg_type, plan.local, h->temp.p, h->sel.p, m.disp, L.pitch, L.rows, L.cols, L.planes, plan.ndisp, st));
            break;
        case scsbp::CSBP_K_COMP_DATA_COST: {
            const scsbp::CsbpLevel &U = plan.lv[k.level + 1];
            const scsbp::CsbpSet up = level_set(h, plan, k.level + 1);
            MI_TRY(scsbp::data_cost(plan.msg_type, im, up.disp, up.step, U.rows, h->cost.p, L.pitch, L.rows, L.cols, k.level, U.planes, c, st));
            break;
        }
        case scsbp::CSBP_K_INIT_MESSAGE: {
            const scsbp::CsbpLevel &U = plan.lv[k.level + 1];
            MI_TRY(scsbp::init_message(plan.msg_type, h->temp.p, m, level_set(h, plan, k.level + 1), h->sel.p, h->cost.p, L.rows, L.cols, L.planes,
                                       U.rows, U.cols, U.planes, st));
            break;
        }
        case scsbp::CSBP_K_ITERATE:
            MI_TRY(scsbp::iterate(plan.msg_type, k.form, L.cap, m, h->sel.p, h->temp.p, L.rows, L.cols, L.planes, k.t, c, st));
            break;
        case scsbp::CSBP_K_DISP:
            MI_TRY(scsbp::compute_disp(plan.msg_type, m, h->sel.p, L.rows, L.cols, L.planes, disp->data, (long long)disp->step, disp->type, st));
            break;
        }
    }
    return MI_OK;
}

}  // namespace

extern "C" {

void mi_stereocsbp_default_params(mi_stereocsbp_params *p)
{
    if (!p) return;
    // createStereoConstantSpaceBP(128, 8, 4, 4, CV_32F) cudastereo.hpp; StereoCSBPImpl ctor + DEFAULT_* stereocsbp.cpp:132-143
    p->ndisp = 128; p->iters = 8; p->levels = 4; p->nr_plane = 4;
    p->max_data_term = 30.0f; p->data_weight = 1.0f; p->max_disc_term = 160.0f; p->disc_single_jump = 10.0f;
    p->min_disp_th = 0; p->msg_type = scsbp::CSBP_MSG_32F; p->use_local_init_data_cost = 1;
}

int mi_stereocsbp_create(const mi_stereocsbp_params *p, mi_stereocsbp **out)
{
    MI_REQUIRE(out, MI_ERR_BAD_ARG, "null out");
    *out = nullptr;
    MI_TRY(require_device());
    mi_stereocsbp *h = new mi_stereocsbp();
    if (p) h->P = *p; else mi_stereocsbp_default_params(&h->P);
    *out = h;
    return MI_OK;
}

int mi_stereocsbp_set_params(mi_stereocsbp *h, const mi_stereocsbp_params *p)
{
    MI_REQUIRE(h && p, MI_ERR_BAD_ARG, "null argument");
    h->P = *p;   // like the reference's setters: validated at compute() (stereocsbp.cpp:154-155)
    return MI_OK;
}

int mi_stereocsbp_get_params(const mi_stereocsbp *h, mi_stereocsbp_params *p)
{
    MI_REQUIRE(h && p, MI_ERR_BAD_ARG, "null argument");
    *p = h->P;
    return MI_OK;
}

void mi_stereocsbp_destroy(mi_stereocsbp *h)
{
    delete h;
}

int mi_stereocsbp_scratch_bytes(const mi_stereocsbp *h, size_t *bytes)
{
    MI_REQUIRE(h && bytes, MI_ERR_BAD_ARG, "null argument");
    *bytes = h->set[0].n + h->set[1].n + h->cost.n + h->sel.n + h->temp.n;
    return MI_OK;
}

int mi_stereocsbp_compute(mi_stereocsbp *h, const mi_mat *left, const mi_mat *right, mi_mat *disp, void *stream)
{
    MI_REQUIRE(h, MI_ERR_BAD_ARG, "null handle");
    const mi_stereocsbp_params &P = h->P;
    int levels = P.levels;
    MI_TRY(scsbp::csbp_fail(scsbp::csbp_check_params(P.ndisp, P.iters, &levels, P.nr_plane, P.msg_type)));   // stereocsbp.cpp:154-155
    scsbp::CsbpImages im;
    MI_TRY(check_images(left, right, &im));
    const scsbp::CsbpPlan plan = scsbp::csbp_make_plan(im.rows, im.cols, im.cn, P.ndisp, P.iters, P.levels, P.nr_plane, P.msg_type,
                                                       P.use_local_init_data_cost);
    MI_TRY(scsbp::csbp_fail(plan.err));
    MI_TRY(check_disp(disp, im.rows, im.cols));
    h->P.levels = plan.levels;   // the clamp is the object's state from here on (stereocsbp.cpp:171)
    return run(h, plan, im, disp, (hipStream_t)stream);
}

int mi_stereocsbp_estimate_recommended_params(int width, int height, int *ndisp, int *iters, int *levels, int *nr_plane)
{
    MI_REQUIRE(ndisp && iters && levels && nr_plane, MI_ERR_BAD_ARG, "null argument");
    MI_REQUIRE(width > 0 && height > 0, MI_ERR_BAD_SIZE, "empty image");
    scsbp::csbp_estimate(width, height, ndisp, iters, levels, nr_plane);
    return MI_OK;
}

// ---- stage-level entry points: the reference's device-layer functions (cuda/stereocsbp.hpp) on caller-owned planar matrices
int mi_stereocsbp_init_data_cost(const mi_stereocsbp_params *p, const mi_mat *left, const mi_mat *right, int level, int nr_plane, mi_mat *temp,
                                 mi_mat *data_cost_selected, mi_mat *disp_selected, void *stream)
{
    MI_REQUIRE(p, MI_ERR_BAD_ARG, "null argument");
    MI_TRY(check_msg_type(p->msg_type));
    MI_REQUIRE(p->ndisp > 0 && nr_plane > 0 && level >= 0 && level < scsbp::CSBP_MAX_LEVELS, MI_ERR_BAD_ARG, "0 < ndisp, 0 < nr_plane, 0 <= level < 8");
    scsbp::CsbpImages im;
    MI_TRY(check_images(left, right, &im));
    const int h = im.rows >> level, w = im.cols >> level;
    MI_REQUIRE(h > 0 && w > 0, MI_ERR_BAD_SIZE, "the level is empty");
    MI_TRY(check_planar(temp, "temp", p->msg_type, p->ndisp, h, w));
    MI_TRY(check_planar(data_cost_selected, "data_cost_selected", p->msg_type, nr_plane, h, w));
    MI_TRY(check_planar(disp_selected, "disp_selected", p->msg_type, nr_plane, h, w));
    MI_REQUIRE(temp->step == data_cost_selected->step && temp->step == disp_selected->step, MI_ERR_BAD_ARG, "the matrices of a level must have one step");
    const long long step = (long long)(temp->step / elem_of(temp->type));
    MI_TRY(scsbp::data_cost(p->msg_type, im, nullptr, 0, 0, temp->data, step, h, w, level, p->ndisp, consts_of(*p), (hipStream_t)stream));
    return scsbp::first_k(p->msg_type, p->use_local_init_data_cost != 0, temp->data, data_cost_selected->data, disp_selected->data, step, h, w,
                          nr_plane, p->ndisp, (hipStream_t)stream);
}

int mi_stereocsbp_compute_data_cost(const mi_stereocsbp_params *p, const mi_mat *left, const mi_mat *right, int level, int nr_plane2,
                                    const mi_mat *disp_selected_parent, mi_mat *data_cost, void *stream)
{
    MI_REQUIRE(p, MI_ERR_BAD_ARG, "null argument");
    MI_TRY(check_msg_type(p->msg_type));
    MI_REQUIRE(nr_plane2 > 0 && level >= 0 && level < scsbp::CSBP_MAX_LEVELS - 1, MI_ERR_BAD_ARG, "0 < nr_plane2, 0 <= level < 7");
    scsbp::CsbpImages im;
    MI_TRY(check_images(left, right, &im));
    const int h = im.rows >> level, w = im.cols >> level, h2 = h / 2, w2 = w / 2;
    MI_REQUIRE(h2 > 0 && w2 > 0, MI_ERR_BAD_SIZE, "the parent level is empty");
    MI_TRY(check_planar(disp_selected_parent, "disp_selected_parent", p->msg_type, nr_plane2, h2, w2));
    MI_TRY(check_planar(data_cost, "data_cost", p->msg_type, nr_plane2, h, w));
    // a pixel of an odd last row / column has no parent (y / 2 == h2); the reference reads beyond the parent level there
    MI_REQUIRE(h == 2 * h2 && w == 2 * w2, MI_ERR_BAD_SIZE, "the level must be twice its parent (even rows and cols of the level)");
    return scsbp::data_cost(p->msg_type, im, disp_selected_parent->data, (long long)(disp_selected_parent->step / elem_of(data_cost->type)), h2,
                            data_cost->data, (long long)(data_cost->step / elem_of(data_cost->type)), h, w, level, nr_plane2, consts_of(*p),
                            (hipStream_t)stream);
}

int mi_stereocsbp_init_message(const mi_mat *cur_udlrs, mi_mat *new_udlrs, const mi_mat *data_cost, mi_mat *data_cost_selected, mi_mat *temp,
                               int nr_plane, int nr_plane2, void *stream)
{
    MI_REQUIRE(cur_udlrs && new_udlrs, MI_ERR_BAD_ARG, "null messages");
    int mt;
    MI_TRY(msg_type_of(&cur_udlrs[0], "u", &mt));
    MI_TRY(check_mat(&new_udlrs[0], "u"));
    MI_REQUIRE(nr_plane > 0 && nr_plane2 > 0 && nr_plane <= nr_plane2, MI_ERR_BAD_ARG, "0 < nr_plane <= nr_plane2");
    MI_REQUIRE(cur_udlrs[0].rows % nr_plane2 == 0 && new_udlrs[0].rows % nr_plane == 0, MI_ERR_BAD_ARG, "%s", "rows % planes == 0");
    const int h2 = cur_udlrs[0].rows / nr_plane2, w2 = cur_udlrs[0].cols, h = new_udlrs[0].rows / nr_plane, w = new_udlrs[0].cols;
    MI_REQUIRE(h2 == h / 2 && w2 == w / 2 && h == 2 * h2 && w == 2 * w2, MI_ERR_BAD_SIZE, "the new level must be twice the current one");
    scsbp::CsbpSet cur, nw;
    MI_TRY(set_of_mats(cur_udlrs, 5, mt, nr_plane2, h2, w2, 0, &cur));
    MI_TRY(set_of_mats(new_udlrs, 5, mt, nr_plane, h, w, 0, &nw));
    MI_TRY(check_planar(data_cost, "data_cost", mt, nr_plane2, h, w));
    MI_TRY(check_planar(temp, "temp", mt, nr_plane2, h, w));
    MI_TRY(check_planar(data_cost_selected, "data_cost_selected", mt, nr_plane, h, w));
    const size_t step = new_udlrs[0].step;
    MI_REQUIRE(data_cost->step == step && temp->step == step && data_cost_selected->step == step, MI_ERR_BAD_ARG,
               "the matrices of a level must have one step");
    return scsbp::init_message(mt, temp->data, nw, cur, data_cost_selected->data, data_cost->data, h, w, nr_plane, h2, w2, nr_plane2,
                               (hipStream_t)stream);
}

int mi_stereocsbp_iterate(const mi_stereocsbp_params *p, mi_mat *udlr, const mi_mat *disp_selected, const mi_mat *data_cost_selected, mi_mat *temp,
                          int nr_plane, int t0, int n_iters, int form, void *stream)
{
    MI_REQUIRE(p && udlr, MI_ERR_BAD_ARG, "null argument");
    MI_TRY(check_msg_type(p->msg_type));
    MI_REQUIRE(nr_plane > 0 && t0 >= 0 && n_iters >= 0, MI_ERR_BAD_ARG, "nr_plane > 0 && t0 >= 0 && n_iters >= 0");
    MI_TRY(check_mat(data_cost_selected, "data_cost_selected"));
    MI_REQUIRE(data_cost_selected->rows % nr_plane == 0, MI_ERR_BAD_ARG, "%s", "data_cost_selected.rows % nr_plane == 0");
    const int h = data_cost_selected->rows / nr_plane, w = data_cost_selected->cols;
    MI_TRY(check_planar(data_cost_selected, "data_cost_selected", p->msg_type, nr_plane, h, w));
    MI_TRY(check_planar(disp_selected, "disp_selected", p->msg_type, nr_plane, h, w));
    scsbp::CsbpSet m;
    MI_TRY(set_of_mats(udlr, 4, p->msg_type, nr_plane, h, w, data_cost_selected->step, &m));
    MI_REQUIRE(disp_selected->step == data_cost_selected->step, MI_ERR_BAD_ARG, "the matrices of a level must have one step");
    m.disp = disp_selected->data;
    // the plan's form rule, and its rejection of a register form beyond its capacities
    const int cap = scsbp::csbp_reg_cap(nr_plane);
    if (form == scsbp::CSBP_FORM_AUTO) form = cap ? scsbp::CSBP_FORM_REG : scsbp::CSBP_FORM_GEN;
    MI_REQUIRE(form == scsbp::CSBP_FORM_GEN || (form == scsbp::CSBP_FORM_REG && cap), MI_ERR_BAD_ARG, "form: the register form holds at most 64 planes");
    void *tp = nullptr;
    if (form == scsbp::CSBP_FORM_GEN) {
        MI_TRY(check_planar(temp, "temp", p->msg_type, nr_plane, h, w));
        MI_REQUIRE(temp->step == data_cost_selected->step, MI_ERR_BAD_ARG, "the matrices of a level must have one step");
        tp = temp->data;
    }
    const scsbp::CsbpConst c = consts_of(*p);
    for (int t = t0; t < t0 + n_iters; ++t)
        MI_TRY(scsbp::iterate(p->msg_type, form, form == scsbp::CSBP_FORM_REG ? cap : 0, m, data_cost_selected->data, tp, h, w, nr_plane, t, c,
                              (hipStream_t)stream));
    return MI_OK;
}

int mi_stereocsbp_compute_disp(const mi_mat *udlr, const mi_mat *disp_selected, const mi_mat *data_cost_selected, int nr_plane, mi_mat *disp,
                               void *stream)
{
    int mt;
    MI_TRY(msg_type_of(data_cost_selected, "data_cost_selected", &mt));
    MI_REQUIRE(nr_plane > 0 && data_cost_selected->rows % nr_plane == 0, MI_ERR_BAD_ARG, "%s", "data_cost_selected.rows % nr_plane == 0");
    const int rows = data_cost_selected->rows / nr_plane, cols = data_cost_selected->cols;
    MI_TRY(check_planar(data_cost_selected, "data_cost_selected", mt, nr_plane, rows, cols));
    MI_TRY(check_planar(disp_selected, "disp_selected", mt, nr_plane, rows, cols));
    scsbp::CsbpSet m;
    MI_TRY(set_of_mats(udlr, 4, mt, nr_plane, rows, cols, data_cost_selected->step, &m));
    MI_REQUIRE(disp_selected->step == data_cost_selected->step, MI_ERR_BAD_ARG, "the matrices of a level must have one step");
    m.disp = disp_selected->data;
    MI_TRY(check_disp(disp, rows, cols));
    return scsbp::compute_disp(mt, m, data_cost_selected->data, rows, cols, nr_plane, disp->data, (long long)disp->step, disp->type,
                               (hipStream_t)stream);
}

}  // extern "C"
