// cv::cuda::BroxOpticalFlow: handle + C-ABI entry points.  Host-side twin of BroxOpticalFlowImpl::calc (modules/cudaoptflow/src/brox.cpp:
// 129-188) and NCVBroxOpticalFlow (modules/cudalegacy/src/cuda/NCVBroxOpticalFlow.cu:598-985): validation, the plan (brox_plan.h), scratch,
// and the plan's launches in order on the caller's stream.  The reference's internal strides and its five stream synchronisations are
// not semantics: planes are padded as the kernels like and calc waits nowhere.
#include <cstdint>
#include <utility>
#include "brox_dev.h"

using namespace mi;
using namespace mi::brox;

struct mi_brox {
    mi_brox_params P;
    int form = MI_BROX_FORM_AUTO;
    DevBuf<unsigned char> scratch;   // brox_plan.h
};

namespace {

int check_f32(const mi_mat *m, int type, int rows, int cols, const char *what)
{
    MI_REQUIRE(m && m->data, MI_ERR_BAD_ARG, "%s: null matrix", what);
    MI_REQUIRE(m->type == type, MI_ERR_BAD_TYPE, "%s must be %s", what, type == MI_32FC1 ? "CV_32FC1" : "CV_32FC2");
    MI_REQUIRE(m->rows == rows && m->cols == cols, MI_ERR_BAD_SIZE, "%s must be %d x %d (rows x cols)", what, rows, cols);
    const size_t elem = type == MI_32FC1 ? 4 : 8;
    MI_REQUIRE(m->step >= (size_t)cols * elem && m->step % 4 == 0 && (uintptr_t)m->data % 4 == 0, MI_ERR_BAD_ARG,
               "%s: step must cover a row and, like data, be a multiple of 4 bytes", what);
    return MI_OK;
}

CPlane cplane(const mi_mat *m) { return {(const float *)m->data, (long long)(m->step / 4)}; }
Plane plane(const mi_mat *m) { return {(float *)m->data, (long long)(m->step / 4)}; }

BroxLaunch grid2(int kernel, int w, int h, unsigned gz, int arg = 0)
{
    return {kernel, 0, brox_div_up(w, BROX_BLOCK_X), brox_div_up(h, BROX_BLOCK_Y), gz, BROX_BLOCK_X * BROX_BLOCK_Y, arg};
}

// the two launches of the seven derivative planes (NCVBroxOpticalFlow.cu:842-868): Ix0, Iy0, Ix, Iy, then Ixx, Iyy, Ixy of Ix and Iy
int run_derivatives(const BroxLaunch &k1, const BroxLaunch &k2, const CPlane &i0, const CPlane &i1, const Plane &ix0, const Plane &iy0,
                    const Plane &ix, const Plane &iy, const Plane &ixx, const Plane &iyy, const Plane &ixy, int w, int h, hipStream_t st)
{
    DerivJobs a = {}, b = {};
    a.j[0] = {i0, ix0, 0}; a.j[1] = {i0, iy0, 1}; a.j[2] = {i1, ix, 0}; a.j[3] = {i1, iy, 1};
    b.j[0] = {cp(ix), ixx, 0}; b.j[1] = {cp(iy), iyy, 1}; b.j[2] = {cp(iy), ixy, 0};
    MI_TRY(derivatives(k1, a, w, h, st));
    return derivatives(k2, b, w, h, st);
}

// the reference's two factors of a prolongation (NCVBroxOpticalFlow.cu:952-955, NPP_staging.cu:2272): the kernel's scale is
// 1 / (1 / scale_factor), the flow is multiplied by 1 / scale_factor; binary32 both
void up_factors(float scale_factor, float *scale, float *mul)
{
    const float x_factor = 1.0f / scale_factor;
    *scale = 1.0f / x_factor;
    *mul = 1.0f / scale_factor;
}

}  // namespace

extern "C" {

void mi_brox_default_params(mi_brox_params *p)
{
    if (!p) return;
    p->alpha = 0.197f; p->gamma = 50.0f; p->scale_factor = 0.8f; p->inner_iterations = 5; p->outer_iterations = 150; p->solver_iterations = 10;
}

int mi_brox_create(const mi_brox_params *p, mi_brox **out)
{
    MI_REQUIRE(out, MI_ERR_BAD_ARG, "null out");
    *out = nullptr;
    mi_brox_params P;
    if (p) P = *p; else mi_brox_default_params(&P);
    MI_TRY(brox_fail(brox_check_params(P)));
    MI_TRY(require_device());
    mi_brox *h = new mi_brox();
    h->P = P;
    *out = h;
    return MI_OK;
}

int mi_brox_set_params(mi_brox *h, const mi_brox_params *p)
{
    MI_REQUIRE(h && p, MI_ERR_BAD_ARG, "null argument");
    MI_TRY(brox_fail(brox_check_params(*p)));
    h->P = *p;
    return MI_OK;
}

int mi_brox_get_params(const mi_brox *h, mi_brox_params *p)
{
    MI_REQUIRE(h && p, MI_ERR_BAD_ARG, "null argument");
    *p = h->P;
    return MI_OK;
}

int mi_brox_set_form(mi_brox *h, int form)
{
    MI_REQUIRE(h, MI_ERR_BAD_ARG, "null handle");
    MI_REQUIRE(form >= MI_BROX_FORM_AUTO && form <= MI_BROX_FORM_BLOCKED, MI_ERR_BAD_ARG, "form is 0 (auto), 1 (plain) or 2 (blocked)");
    h->form = form;
    return MI_OK;
}

int mi_brox_scratch_bytes(const mi_brox *h, size_t *bytes)
{
    MI_REQUIRE(h && bytes, MI_ERR_BAD_ARG, "null argument");
    *bytes = h->scratch.n;
    return MI_OK;
}

int mi_brox_plan_info(const mi_brox_params *p, int rows, int cols, int form, int *levels, int *launches, int *sor_launches)
{
    MI_REQUIRE(p && levels && launches && sor_launches, MI_ERR_BAD_ARG, "null argument");
    MI_REQUIRE(form >= MI_BROX_FORM_AUTO && form <= MI_BROX_FORM_BLOCKED, MI_ERR_BAD_ARG, "form is 0 (auto), 1 (plain) or 2 (blocked)");
    const BroxPlan plan = brox_make_plan(rows, cols, *p, form);
    MI_TRY(brox_fail(plan.err));
    *levels = (int)plan.levels.size(); *launches = (int)plan.launches.size(); *sor_launches = plan.sor_launches;
    return MI_OK;
}

void mi_brox_destroy(mi_brox *h)
{
    delete h;
}

int mi_brox_calc(mi_brox *h, const mi_mat *frame0, const mi_mat *frame1, mi_mat *flow, void *stream)
{
    MI_REQUIRE(h, MI_ERR_BAD_ARG, "null handle");
    MI_REQUIRE(frame0 && frame1 && flow, MI_ERR_BAD_ARG, "null matrix");
    MI_TRY(brox_fail(brox_check_size(frame0->rows, frame0->cols)));
    const int rows = frame0->rows, cols = frame0->cols;
    MI_TRY(check_f32(frame0, MI_32FC1, rows, cols, "frame0"));
    MI_TRY(check_f32(frame1, MI_32FC1, rows, cols, "frame1"));
    MI_TRY(check_f32(flow, MI_32FC2, rows, cols, "flow"));
    const BroxPlan plan = brox_make_plan(rows, cols, h->P, h->form);
    MI_TRY(brox_fail(plan.err));
    MI_TRY(h->scratch.ensure(plan.scratch_bytes));
    hipStream_t st = (hipStream_t)stream;
    float *s = (float *)h->scratch.p;
    auto slot = [&](int id, int level) { return Plane{s + plan.off_slot[id], (long long)plan.levels[level].ld}; };
    auto image = [&](int level, int which) {
        if (level == 0) return cplane(which ? frame1 : frame0);
        const BroxLevel &L = plan.levels[level];
        return CPlane{s + (which ? L.off_i1 : L.off_i0), (long long)L.ld};
    };
    float up_scale, up_mul;
    up_factors(h->P.scale_factor, &up_scale, &up_mul);
    int su = S_U, sv = S_V, su2 = S_U2, sv2 = S_V2;       // ptrU / ptrUNew: swapped by a prolongation
    int sdu = S_DU, sdv = S_DV, sdu2 = S_DU2, sdv2 = S_DV2;   // where the increments are: swapped by a blocked launch
    for (const BroxLaunch &k : plan.launches) {
        const BroxLevel &L = plan.levels[k.level];
        const int l = k.level;
        switch (k.kernel) {
        case BROX_K_RESIZE_DOWN: {
            const BroxLevel &S = plan.levels[l - 1];
            const CPlane src[2] = {image(l - 1, 0), image(l - 1, 1)};
            const Plane dst[2] = {{s + L.off_i0, (long long)L.ld}, {s + L.off_i1, (long long)L.ld}};
            MI_TRY(resize_down(k, src, S.w, S.h, dst, L.w, L.h, 1.0f / h->P.scale_factor, st));
            break;
        }
        case BROX_K_ZERO:
            if (k.arg == S_U) MI_TRY(zero2(k, slot(su, l), slot(sv, l), L.w, L.h, st));
            else { sdu = S_DU; sdv = S_DV; sdu2 = S_DU2; sdv2 = S_DV2; MI_TRY(zero2(k, slot(sdu, l), slot(sdv, l), L.w, L.h, st)); }
            break;
        case BROX_K_DERIV1: {
            DerivJobs a = {};
            a.j[0] = {image(l, 0), slot(S_IX0, l), 0}; a.j[1] = {image(l, 0), slot(S_IY0, l), 1};
            a.j[2] = {image(l, 1), slot(S_IX, l), 0}; a.j[3] = {image(l, 1), slot(S_IY, l), 1};
            MI_TRY(derivatives(k, a, L.w, L.h, st));
            break;
        }
        case BROX_K_DERIV2: {
            DerivJobs b = {};
            b.j[0] = {cp(slot(S_IX, l)), slot(S_IXX, l), 0}; b.j[1] = {cp(slot(S_IY, l)), slot(S_IYY, l), 1};
            b.j[2] = {cp(slot(S_IY, l)), slot(S_IXY, l), 0};
            MI_TRY(derivatives(k, b, L.w, L.h, st));
            break;
        }
        case BROX_K_PREPARE1:
        case BROX_K_PREPARE2: {
            const Coeffs c = {slot(S_DIFFX, l), slot(S_DIFFY, l), slot(S_DENU, l), slot(S_DENV, l), slot(S_NDUDV, l), slot(S_NU, l), slot(S_NV, l)};
            if (k.kernel == BROX_K_PREPARE2) { MI_TRY(prepare2(k, c, L.w, L.h, st)); break; }
            const Images im = {image(l, 0), image(l, 1), cp(slot(S_IX, l)), cp(slot(S_IXX, l)), cp(slot(S_IX0, l)), cp(slot(S_IY, l)),
                               cp(slot(S_IYY, l)), cp(slot(S_IY0, l)), cp(slot(S_IXY, l))};
            MI_TRY(prepare1(k, cp(slot(su, l)), cp(slot(sv, l)), cp(slot(sdu, l)), cp(slot(sdv, l)), im, c, L.w, L.h, h->P.alpha, h->P.gamma, st));
            break;
        }
        case BROX_K_SOR_PLAIN:
        case BROX_K_SOR_BLOCKED: {
            // sor_pass<0>: du -> du_new, sor_pass<1>: du_new -> du (NCVBroxOpticalFlow.cu:915-922); a blocked launch: du -> du_new
            const bool back = k.kernel == BROX_K_SOR_PLAIN && k.arg == 1;
            const int a = back ? sdu2 : sdu, b = back ? sdv2 : sdv, c = back ? sdu : sdu2, d = back ? sdv : sdv2;
            const SorArgs A = {cp(slot(su, l)), cp(slot(sv, l)), cp(slot(a, l)), cp(slot(b, l)), slot(c, l), slot(d, l),
                               cp(slot(S_DIFFX, l)), cp(slot(S_DIFFY, l)), cp(slot(S_DENU, l)), cp(slot(S_DENV, l)), cp(slot(S_NDUDV, l)),
                               cp(slot(S_NU, l)), cp(slot(S_NV, l)), L.w, L.h};
            if (k.kernel == BROX_K_SOR_PLAIN) MI_TRY(sor_plain(k, A, st));
            else {
                MI_TRY(sor_blocked(k, A, st));
                std::swap(sdu, sdu2); std::swap(sdv, sdv2);
            }
            break;
        }
        case BROX_K_RESIZE_UP: {   // k.level is the destination; the source is the level below it in resolution
            const BroxLevel &S = plan.levels[l + 1];
            const CPlane a[2] = {cp(slot(su, l + 1)), cp(slot(sv, l + 1))}, b[2] = {cp(slot(sdu, l + 1)), cp(slot(sdv, l + 1))};
            const Plane dst[2] = {slot(su2, l), slot(sv2, l)};
            MI_TRY(resize_up(k, a, b, S.w, S.h, dst, L.w, L.h, up_scale, up_mul, st));
            std::swap(su, su2); std::swap(sv, sv2);
            break;
        }
        default:
            MI_TRY(add_out(k, cp(slot(su, 0)), cp(slot(sdu, 0)), cp(slot(sv, 0)), cp(slot(sdv, 0)), (float *)flow->data, (long long)(flow->step / 4),
                           L.w, L.h, st));
            break;
        }
    }
    return MI_OK;
}

int mi_brox_resize_down(const mi_mat *src, mi_mat *dst, float scale_factor, void *stream)
{
    MI_REQUIRE(src && dst, MI_ERR_BAD_ARG, "null matrix");
    MI_REQUIRE(scale_factor > 0.f && scale_factor < 1.f, MI_ERR_BAD_ARG, "0 < scale_factor < 1");
    MI_TRY(brox_fail(brox_check_size(src->rows, src->cols)));
    MI_TRY(check_f32(src, MI_32FC1, src->rows, src->cols, "src"));
    MI_REQUIRE(dst->rows >= 1 && dst->cols >= 1, MI_ERR_BAD_SIZE, "dst is empty");
    MI_TRY(check_f32(dst, MI_32FC1, dst->rows, dst->cols, "dst"));
    MI_REQUIRE(brox_resize_down_fits(src->cols, dst->cols, scale_factor) && brox_resize_down_fits(src->rows, dst->rows, scale_factor),
               MI_ERR_BAD_SIZE, "dst is too large for src at this scale_factor: the supersample window of its last pixel leaves src");
    MI_TRY(require_device());
    const CPlane s[2] = {cplane(src), {}};
    const Plane d[2] = {plane(dst), {}};
    hipStream_t st = (hipStream_t)stream;
    MI_TRY(resize_down(grid2(BROX_K_RESIZE_DOWN, dst->cols, dst->rows, 1), s, src->cols, src->rows, d, dst->cols, dst->rows, 1.0f / scale_factor, st));
    MI_HIP_TRY(hipStreamSynchronize(st));
    return MI_OK;
}

int mi_brox_resize_up(const mi_mat *src, mi_mat *dst, float scale_factor, void *stream)
{
    MI_REQUIRE(src && dst, MI_ERR_BAD_ARG, "null matrix");
    MI_REQUIRE(scale_factor > 0.f && scale_factor < 1.f, MI_ERR_BAD_ARG, "0 < scale_factor < 1");
    MI_REQUIRE(src->rows >= 1 && src->cols >= 1 && dst->rows >= 1 && dst->cols >= 1, MI_ERR_BAD_SIZE, "empty matrix");
    MI_TRY(check_f32(src, MI_32FC1, src->rows, src->cols, "src"));
    MI_TRY(check_f32(dst, MI_32FC1, dst->rows, dst->cols, "dst"));
    MI_TRY(require_device());
    float scale, mul;
    up_factors(scale_factor, &scale, &mul);
    const CPlane a[2] = {cplane(src), {}};
    const Plane d[2] = {plane(dst), {}};
    hipStream_t st = (hipStream_t)stream;
    MI_TRY(resize_up(grid2(BROX_K_RESIZE_UP, dst->cols, dst->rows, 1), a, nullptr, src->cols, src->rows, d, dst->cols, dst->rows, scale, mul, st));
    MI_HIP_TRY(hipStreamSynchronize(st));
    return MI_OK;
}

int mi_brox_derivatives(const mi_mat *i0, const mi_mat *i1, mi_mat *planes, void *stream)
{
    MI_REQUIRE(i0 && i1 && planes, MI_ERR_BAD_ARG, "null matrix");
    MI_TRY(brox_fail(brox_check_size(i0->rows, i0->cols)));
    const int rows = i0->rows, cols = i0->cols;
    MI_TRY(check_f32(i0, MI_32FC1, rows, cols, "i0"));
    MI_TRY(check_f32(i1, MI_32FC1, rows, cols, "i1"));
    for (int i = 0; i < 7; ++i) MI_TRY(check_f32(planes + i, MI_32FC1, rows, cols, "a derivative plane"));
    MI_TRY(require_device());
    hipStream_t st = (hipStream_t)stream;
    MI_TRY(run_derivatives(grid2(BROX_K_DERIV1, cols, rows, 4), grid2(BROX_K_DERIV2, cols, rows, 3), cplane(i0), cplane(i1), plane(planes + 0),
                           plane(planes + 1), plane(planes + 2), plane(planes + 3), plane(planes + 4), plane(planes + 5), plane(planes + 6), cols,
                           rows, st));
    MI_HIP_TRY(hipStreamSynchronize(st));
    return MI_OK;
}

int mi_brox_prepare(const mi_mat *u, const mi_mat *v, const mi_mat *du, const mi_mat *dv, const mi_mat *images, float alpha, float gamma,
                    mi_mat *coeffs, void *stream)
{
    MI_REQUIRE(u && v && du && dv && images && coeffs, MI_ERR_BAD_ARG, "null matrix");
    MI_REQUIRE(alpha > 0.f && gamma >= 0.f, MI_ERR_BAD_ARG, "alpha > 0, gamma >= 0");
    MI_TRY(brox_fail(brox_check_size(u->rows, u->cols)));
    const int rows = u->rows, cols = u->cols;
    const mi_mat *flows[4] = {u, v, du, dv};
    for (const mi_mat *m : flows) MI_TRY(check_f32(m, MI_32FC1, rows, cols, "u, v, du, dv"));
    for (int i = 0; i < 9; ++i) MI_TRY(check_f32(images + i, MI_32FC1, rows, cols, "an image plane"));
    for (int i = 0; i < 7; ++i) MI_TRY(check_f32(coeffs + i, MI_32FC1, rows, cols, "a coefficient plane"));
    MI_TRY(require_device());
    const Images im = {cplane(images + 0), cplane(images + 1), cplane(images + 2), cplane(images + 3), cplane(images + 4), cplane(images + 5),
                       cplane(images + 6), cplane(images + 7), cplane(images + 8)};
    const Coeffs c = {plane(coeffs + 0), plane(coeffs + 1), plane(coeffs + 2), plane(coeffs + 3), plane(coeffs + 4), plane(coeffs + 5),
                      plane(coeffs + 6)};
    hipStream_t st = (hipStream_t)stream;
    MI_TRY(prepare1(grid2(BROX_K_PREPARE1, cols, rows, 1), cplane(u), cplane(v), cplane(du), cplane(dv), im, c, cols, rows, alpha, gamma, st));
    MI_TRY(prepare2(grid2(BROX_K_PREPARE2, cols, rows, 1), c, cols, rows, st));
    MI_HIP_TRY(hipStreamSynchronize(st));
    return MI_OK;
}

int mi_brox_sor(const mi_mat *u, const mi_mat *v, mi_mat *du, mi_mat *dv, const mi_mat *coeffs, int form, int solver_iterations, void *stream)
{
    MI_REQUIRE(u && v && du && dv && coeffs, MI_ERR_BAD_ARG, "null matrix");
    MI_REQUIRE(form >= MI_BROX_FORM_AUTO && form <= MI_BROX_FORM_BLOCKED, MI_ERR_BAD_ARG, "form is 0 (auto), 1 (plain) or 2 (blocked)");
    MI_REQUIRE(solver_iterations > 0, MI_ERR_BAD_ARG, "solver_iterations > 0");
    MI_TRY(brox_fail(brox_check_size(u->rows, u->cols)));
    const int rows = u->rows, cols = u->cols;
    const mi_mat *flows[4] = {u, v, du, dv};
    for (const mi_mat *m : flows) MI_TRY(check_f32(m, MI_32FC1, rows, cols, "u, v, du, dv"));
    for (int i = 0; i < 7; ++i) MI_TRY(check_f32(coeffs + i, MI_32FC1, rows, cols, "a coefficient plane"));
    MI_TRY(require_device());
    DevTmp tmp;
    float *t;
    const int ld = brox_ld(cols);
    const size_t pl = brox_plane(cols, rows);
    MI_TRY(tmp.alloc(&t, 2 * pl));
    Plane cur[2] = {plane(du), plane(dv)}, alt[2] = {{t, (long long)ld}, {t + pl, (long long)ld}};
    std::vector<BroxLaunch> launches;
    brox_sor_launches(cols, rows, 0, solver_iterations, form, &launches);
    hipStream_t st = (hipStream_t)stream;
    bool in_alt = false;
    for (const BroxLaunch &k : launches) {
        const bool back = k.kernel == BROX_K_SOR_PLAIN && k.arg == 1;   // reads the other buffer, writes the current one
        const Plane *rd = back ? alt : cur, *wr = back ? cur : alt;
        const SorArgs A = {cplane(u), cplane(v), cp(rd[0]), cp(rd[1]), wr[0], wr[1], cplane(coeffs + 0), cplane(coeffs + 1), cplane(coeffs + 2),
                           cplane(coeffs + 3), cplane(coeffs + 4), cplane(coeffs + 5), cplane(coeffs + 6), cols, rows};
        if (k.kernel == BROX_K_SOR_PLAIN) MI_TRY(sor_plain(k, A, st));
        else {
            MI_TRY(sor_blocked(k, A, st));
            std::swap(cur[0], alt[0]); std::swap(cur[1], alt[1]);
            in_alt = !in_alt;
        }
    }
    if (in_alt) {   // an odd number of blocked launches left the result in the temporary planes
        MI_HIP_TRY(hipMemcpy2DAsync(du->data, du->step, cur[0].p, (size_t)ld * 4, (size_t)cols * 4, rows, hipMemcpyDeviceToDevice, st));
        MI_HIP_TRY(hipMemcpy2DAsync(dv->data, dv->step, cur[1].p, (size_t)ld * 4, (size_t)cols * 4, rows, hipMemcpyDeviceToDevice, st));
    }
    MI_HIP_TRY(hipStreamSynchronize(st));
    return MI_OK;
}

}  // extern "C"
