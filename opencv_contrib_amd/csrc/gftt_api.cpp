// cv::cuda::CornernessCriteria and cv::cuda::CornersDetector: handles + C-ABI entry points.  Host-side twin of CornerBase / Harris /
// MinEigenVal (modules/cudaimgproc/src/corners.cpp:83-176) and GoodFeaturesToTrackDetector (src/gftt.cpp:90-214): validation, the plan
// (gftt_plan.h), scratch, the plan's launches in order on the caller's stream, and ONE read-back of the count at the end of a detect
// (the reference waits for minMax, for findCorners' count and, with minDistance >= 1, for the download).
#include <cstring>
#include "gftt_dev.h"
#include "mi_buf.h"

using namespace mi;

struct mi_corner {
    mi_corner_params P;
    gftt::GfttCorner c;
    DevBuf<unsigned char> scratch;   // per-workgroup maxima; Dx / Dy planes in the two-launch form
};

struct mi_gftt {
    mi_gftt_params P;
    gftt::GfttCorner c;
    DevBuf<unsigned char> scratch;                // gftt_plan.h
    PinnedBuf<int, hipHostMallocDefault> ctl;     // the read-back's landing place
    PinnedBuf<float, hipHostMallocDefault> pts;   // minDistance >= 1: the sorted points, then the survivors
};

namespace {

gftt::GfttMatDesc desc_of(const mi_mat *m) { return {m->rows, m->cols, m->type, m->step, m->data != nullptr}; }

// corners.cpp:93-101 and filtering.cpp:524-545 for ksize == 3: [-1 0 1] and [1 2 1] * scale, the product taken in double (Mat *= double)
gftt::GfttCorner corner_of(int type, int block_size, int border, int harris, double k)
{
    double scale = (double)(1 << (3 - 1)) * block_size;
    if (type == MI_8UC1) scale *= 255.;
    scale = 1. / scale;
    gftt::GfttCorner c = {};
    c.deriv[0] = -1.f; c.deriv[1] = 0.f; c.deriv[2] = 1.f;
    c.smooth[0] = (float)(1. * scale); c.smooth[1] = (float)(2. * scale); c.smooth[2] = (float)(1. * scale);
    c.block_size = block_size; c.border = border; c.harris = harris ? 1 : 0; c.k = (float)k;
    return c;
}

int check_frame(const mi_mat *img, int type, const mi_mat *mask, gftt::GfttImage *im, gftt::GfttMask *mk)
{
    MI_REQUIRE(img, MI_ERR_BAD_ARG, "null image");
    const bool masked = mask && mask->data;
    gftt::GfttMatDesc md = {};
    if (masked) md = desc_of(mask);
    MI_TRY(gftt::gftt_fail(gftt::gftt_check_image(desc_of(img), type, masked ? &md : nullptr)));
    *im = {(const unsigned char *)img->data, (long long)img->step, img->rows, img->cols, img->type};
    if (mk) *mk = {masked ? (const unsigned char *)mask->data : nullptr, masked ? (long long)mask->step : 0};
    return MI_OK;
}

// the response's launches; area: wgmax at 0, then the planes
int run_response(const gftt::GfttResponsePlan &rp, const gftt::GfttImage &im, const gftt::GfttCorner &c, const gftt::GfttPlane &dst, float *wgmax,
                 float *dx, float *dy, hipStream_t st)
{
    for (const gftt::GfttLaunch &k : rp.launches) {
        if (k.kernel == gftt::GFTT_K_RESPONSE) MI_TRY(gftt::response_fused(k, rp, im, c, dst, wgmax, st));
        else if (k.kernel == gftt::GFTT_K_DERIV) MI_TRY(gftt::response_deriv(k, im, c, dx, dy, st));
        else MI_TRY(gftt::response_window(k, rp, c, dx, dy, dst, wgmax, st));
    }
    return MI_OK;
}

// scratch of a response on its own: {wgmax, dx, dy}
struct ResponseArea { size_t off_dx, off_dy, bytes; };
ResponseArea response_area(const gftt::GfttResponsePlan &rp)
{
    ResponseArea a = {};
    size_t o = gftt::gftt_align((size_t)rp.ntiles * sizeof(float)) + gftt::gftt_align(gftt::GFTT_CTL_INTS * sizeof(int));
    const size_t plane = gftt::gftt_align((size_t)rp.rows * rp.cols * sizeof(float));
    a.off_dx = o; if (rp.form == gftt::GFTT_FORM_PLANES) o += plane;
    a.off_dy = o; if (rp.form == gftt::GFTT_FORM_PLANES) o += plane;
    a.bytes = o;
    return a;
}

int check_taps(const float *t)
{
    for (int i = 0; i < 3; ++i) MI_REQUIRE(t[i] == t[i] && t[i] - t[i] == 0.f, MI_ERR_BAD_ARG, "taps must be finite");
    return MI_OK;
}

}  // namespace

extern "C" {

int mi_corner_create(const mi_corner_params *p, mi_corner **out)
{
    MI_REQUIRE(out, MI_ERR_BAD_ARG, "null out");
    *out = nullptr;
    MI_REQUIRE(p, MI_ERR_BAD_ARG, "null params");
    MI_TRY(gftt::gftt_fail(gftt::gftt_check_corner(p->type, p->block_size, p->ksize, p->border_type)));
    MI_TRY(require_device());
    mi_corner *h = new mi_corner();
    h->P = *p;
    h->c = corner_of(p->type, p->block_size, p->border_type, p->harris, p->k);
    *out = h;
    return MI_OK;
}

void mi_corner_destroy(mi_corner *h)
{
    delete h;
}

int mi_corner_compute(mi_corner *h, const mi_mat *src, mi_mat *dst, void *stream)
{
    MI_REQUIRE(h && dst, MI_ERR_BAD_ARG, "null argument");
    gftt::GfttImage im;
    MI_TRY(check_frame(src, h->P.type, nullptr, &im, nullptr));
    MI_TRY(gftt::gftt_fail(gftt::gftt_check_f32(desc_of(dst), src->rows, src->cols, "dst must be CV_32FC1 of the source's size")));
    const gftt::GfttResponsePlan rp = gftt::gftt_response_plan(im.rows, im.cols, h->P.block_size, gftt::GFTT_FORM_AUTO);
    MI_TRY(gftt::gftt_fail(rp.err));
    const ResponseArea a = response_area(rp);
    MI_TRY(h->scratch.ensure(a.bytes));
    return run_response(rp, im, h->c, {(float *)dst->data, (long long)dst->step}, (float *)h->scratch.p, (float *)(h->scratch.p + a.off_dx),
                        (float *)(h->scratch.p + a.off_dy), (hipStream_t)stream);
}

void mi_gftt_default_params(mi_gftt_params *p)
{
    if (!p) return;
    // createGoodFeaturesToTrackDetector, cudaimgproc.hpp:617-618
    p->type = MI_8UC1; p->max_corners = 1000; p->quality_level = 0.01; p->min_distance = 0.0; p->block_size = 3; p->use_harris = 0; p->harris_k = 0.04;
}

static int check_gftt_params(const mi_gftt_params &P)
{
    MI_TRY(gftt::gftt_fail(gftt::gftt_check_params(P.max_corners, P.quality_level, P.min_distance)));
    return gftt::gftt_fail(gftt::gftt_check_corner(P.type, P.block_size, 3, gftt::GFTT_BORDER_REFLECT101));
}

int mi_gftt_create(const mi_gftt_params *p, mi_gftt **out)
{
    MI_REQUIRE(out, MI_ERR_BAD_ARG, "null out");
    *out = nullptr;
    mi_gftt_params P;
    if (p) P = *p; else mi_gftt_default_params(&P);
    MI_TRY(check_gftt_params(P));
    MI_TRY(require_device());
    mi_gftt *h = new mi_gftt();
    h->P = P;
    h->c = corner_of(P.type, P.block_size, gftt::GFTT_BORDER_REFLECT101, P.use_harris, P.harris_k);   // gftt.cpp:96-98; the factories' default border, cudaimgproc.hpp:562,575
    *out = h;
    return MI_OK;
}

int mi_gftt_set_params(mi_gftt *h, const mi_gftt_params *p)
{
    MI_REQUIRE(h && p, MI_ERR_BAD_ARG, "null argument");
    MI_TRY(check_gftt_params(*p));
    h->P = *p;
    h->c = corner_of(p->type, p->block_size, gftt::GFTT_BORDER_REFLECT101, p->use_harris, p->harris_k);
    return MI_OK;
}

int mi_gftt_get_params(const mi_gftt *h, mi_gftt_params *p)
{
    MI_REQUIRE(h && p, MI_ERR_BAD_ARG, "null argument");
    *p = h->P;
    return MI_OK;
}

void mi_gftt_destroy(mi_gftt *h)
{
    delete h;
}

int mi_gftt_scratch_bytes(const mi_gftt *h, size_t *bytes)
{
    MI_REQUIRE(h && bytes, MI_ERR_BAD_ARG, "null argument");
    *bytes = h->scratch.n;
    return MI_OK;
}

int mi_gftt_detect(mi_gftt *h, const mi_mat *img, const mi_mat *mask, mi_mat *corners, int *n, void *stream)
{
    MI_REQUIRE(h, MI_ERR_BAD_ARG, "null handle");
    MI_REQUIRE(corners && n, MI_ERR_BAD_ARG, "null corners or n");
    const mi_gftt_params &P = h->P;
    gftt::GfttImage im;
    gftt::GfttMask mk;
    MI_TRY(check_frame(img, P.type, mask, &im, &mk));
    const gftt::GfttPlan plan = gftt::gftt_make_plan(im.rows, im.cols, P.block_size, gftt::GFTT_FORM_AUTO);
    MI_TRY(gftt::gftt_fail(plan.err));
    MI_REQUIRE(corners->data && corners->type == MI_32FC2 && corners->rows == 1, MI_ERR_BAD_TYPE, "corners must be 1 x N CV_32FC2");
    MI_REQUIRE(corners->cols >= gftt::gftt_output_cols(im.rows, im.cols, P.max_corners), MI_ERR_BAD_SIZE,
               "corners needs min(maxCorners > 0 ? maxCorners : capacity, capacity) columns, capacity = max(1000, (int)(area * 0.05))");
    *n = 0;
    hipStream_t st = (hipStream_t)stream;
    const bool head = P.min_distance < 1;   // gftt.cpp:134
    MI_TRY(h->scratch.ensure(plan.scratch_bytes));
    MI_TRY(h->ctl.ensure(gftt::GFTT_CTL_INTS));
    if (!head) MI_TRY(h->pts.ensure((size_t)2 * plan.capacity));
    unsigned char *s = h->scratch.p;
    const gftt::GfttPlane resp = {(float *)(s + plan.off_resp), (long long)im.cols * 4};
    float *wgmax = (float *)(s + plan.off_wgmax);
    int *ctl = (int *)(s + plan.off_ctl);
    unsigned long long *masks = (unsigned long long *)(s + plan.off_masks), *keys = (unsigned long long *)(s + plan.off_keys);
    int *bcount = (int *)(s + plan.off_bcount), *bbase = (int *)(s + plan.off_bbase);
    float *spts = (float *)(s + plan.off_pts);
    for (const gftt::GfttLaunch &k : plan.launches) {
        switch (k.kernel) {
        case gftt::GFTT_K_RESPONSE: MI_TRY(gftt::response_fused(k, plan.resp, im, h->c, resp, wgmax, st)); break;
        case gftt::GFTT_K_DERIV: MI_TRY(gftt::response_deriv(k, im, h->c, (float *)(s + plan.off_dx), (float *)(s + plan.off_dy), st)); break;
        case gftt::GFTT_K_WINDOW:
            MI_TRY(gftt::response_window(k, plan.resp, h->c, (float *)(s + plan.off_dx), (float *)(s + plan.off_dy), resp, wgmax, st));
            break;
        case gftt::GFTT_K_THRESHOLD: MI_TRY(gftt::threshold(k, wgmax, plan.resp.ntiles, P.quality_level, ctl, st)); break;
        case gftt::GFTT_K_FIND: MI_TRY(gftt::find(k, resp, im.rows, im.cols, mk, ctl, 0.f, masks, plan.segs_x, plan.nseg, bcount, st)); break;
        case gftt::GFTT_K_SCAN: MI_TRY(gftt::scan(k, bcount, bbase, plan.nfind, plan.capacity, ctl, st)); break;
        case gftt::GFTT_K_EMIT:
            MI_TRY(gftt::emit(k, resp, im.cols, masks, plan.segs_x, plan.nseg, bbase, plan.capacity, keys, nullptr, st));
            break;
        case gftt::GFTT_K_POINTS:
            MI_TRY(gftt::points(k, keys, im.cols, head ? P.max_corners : 0, head ? (float *)corners->data : spts, ctl, st));
            break;
        default: MI_TRY(gftt::sort_step(k, keys, ctl, st)); break;
        }
    }
    MI_HIP_TRY(hipMemcpyAsync(h->ctl.p, ctl, gftt::GFTT_CTL_INTS * sizeof(int), hipMemcpyDeviceToHost, st));
    MI_HIP_TRY(hipStreamSynchronize(st));
    const int total = h->ctl.p[gftt::GFTT_CTL_NOUT];
    if (head || total == 0) {   // total == 0: the reference releases the output (gftt.cpp:126-130)
        *n = total;
        return MI_OK;
    }
    // gftt.cpp:140-212: the sorted points come down, the grid loop runs here, the survivors go up
    MI_HIP_TRY(hipMemcpyAsync(h->pts.p, spts, (size_t)total * 2 * sizeof(float), hipMemcpyDeviceToHost, st));
    MI_HIP_TRY(hipStreamSynchronize(st));
    std::vector<float> kept;
    gftt::gftt_min_distance(h->pts.p, total, im.rows, im.cols, P.min_distance, P.max_corners, &kept);
    const int m = (int)(kept.size() / 2);
    std::memcpy(h->pts.p, kept.data(), kept.size() * sizeof(float));
    MI_HIP_TRY(hipMemcpyAsync(corners->data, h->pts.p, kept.size() * sizeof(float), hipMemcpyHostToDevice, st));
    MI_HIP_TRY(hipStreamSynchronize(st));   // the pinned buffer is the handle's: the next call may write it
    *n = m;
    return MI_OK;
}

int mi_gftt_response(const mi_mat *src, const float *deriv, const float *smooth, int block_size, int border_type, int harris, float k, int form,
                     mi_mat *dst, double quality_level, float *threshold, void *stream)
{
    MI_REQUIRE(src && deriv && smooth && dst, MI_ERR_BAD_ARG, "null argument");
    MI_TRY(gftt::gftt_fail(gftt::gftt_check_corner(src->type, block_size, 3, border_type)));
    MI_TRY(check_taps(deriv));
    MI_TRY(check_taps(smooth));
    gftt::GfttImage im;
    MI_TRY(check_frame(src, src->type, nullptr, &im, nullptr));
    MI_TRY(gftt::gftt_fail(gftt::gftt_check_f32(desc_of(dst), src->rows, src->cols, "dst must be CV_32FC1 of the source's size")));
    MI_REQUIRE(!threshold || quality_level > 0, MI_ERR_BAD_ARG, "qualityLevel > 0");
    const gftt::GfttResponsePlan rp = gftt::gftt_response_plan(im.rows, im.cols, block_size, form);
    MI_TRY(gftt::gftt_fail(rp.err));
    MI_TRY(require_device());
    gftt::GfttCorner c = {};
    for (int i = 0; i < 3; ++i) { c.deriv[i] = deriv[i]; c.smooth[i] = smooth[i]; }
    c.block_size = block_size; c.border = border_type; c.harris = harris ? 1 : 0; c.k = k;
    const ResponseArea a = response_area(rp);
    DevTmp tmp;
    unsigned char *s;
    MI_TRY(tmp.alloc(&s, a.bytes));
    hipStream_t st = (hipStream_t)stream;
    MI_TRY(run_response(rp, im, c, {(float *)dst->data, (long long)dst->step}, (float *)s, (float *)(s + a.off_dx), (float *)(s + a.off_dy), st));
    int ctl_host[gftt::GFTT_CTL_INTS] = {};
    if (threshold) {
        int *ctl = (int *)(s + gftt::gftt_align((size_t)rp.ntiles * sizeof(float)));
        MI_TRY(gftt::threshold({gftt::GFTT_K_THRESHOLD, 1, 1, gftt::GFTT_SCAN_THREADS, 0, 0, 0}, (const float *)s, rp.ntiles, quality_level, ctl, st));
        MI_HIP_TRY(hipMemcpyAsync(ctl_host, ctl, sizeof(int), hipMemcpyDeviceToHost, st));
    }
    MI_HIP_TRY(hipStreamSynchronize(st));   // the temporary scratch goes with this call
    if (threshold) std::memcpy(threshold, ctl_host, sizeof(float));
    return MI_OK;
}

int mi_gftt_find_corners(const mi_mat *response, float threshold, const mi_mat *mask, mi_mat *corners, int *count, void *stream)
{
    MI_REQUIRE(response && corners && count, MI_ERR_BAD_ARG, "null argument");
    MI_TRY(gftt::gftt_fail(gftt::gftt_check_f32(desc_of(response), response->rows, response->cols, "response must be CV_32FC1")));
    gftt::GfttImage im;
    gftt::GfttMask mk;
    MI_TRY(check_frame(response, MI_32FC1, mask, &im, &mk));
    MI_REQUIRE(corners->data && corners->type == MI_32FC2 && corners->rows == 1 && corners->cols >= 1, MI_ERR_BAD_SIZE,
               "corners must be 1 x max_count CV_32FC2");
    MI_TRY(require_device());
    const int segs_x = div_up(im.cols, gftt::GFTT_SEG), nseg = im.rows * segs_x, nfind = div_up(nseg, gftt::GFTT_FIND_SEGS);
    const size_t o_masks = gftt::gftt_align(gftt::GFTT_CTL_INTS * sizeof(int)), o_bcount = o_masks + gftt::gftt_align((size_t)nseg * 8),
                 o_bbase = o_bcount + gftt::gftt_align((size_t)nfind * 4), bytes = o_bbase + gftt::gftt_align((size_t)nfind * 4);
    DevTmp tmp;
    unsigned char *s;
    MI_TRY(tmp.alloc(&s, bytes));
    hipStream_t st = (hipStream_t)stream;
    const gftt::GfttPlane resp = {(float *)response->data, (long long)response->step};
    unsigned long long *masks = (unsigned long long *)(s + o_masks);
    int *ctl = (int *)s, *bcount = (int *)(s + o_bcount), *bbase = (int *)(s + o_bbase);
    const gftt::GfttLaunch per_find = {gftt::GFTT_K_FIND, (unsigned)nfind, 1, gftt::GFTT_BLOCK, 0, 0, 0};
    MI_TRY(gftt::find(per_find, resp, im.rows, im.cols, mk, nullptr, threshold, masks, segs_x, nseg, bcount, st));
    MI_TRY(gftt::scan({gftt::GFTT_K_SCAN, 1, 1, gftt::GFTT_SCAN_THREADS, 0, 0, 0}, bcount, bbase, nfind, corners->cols, ctl, st));
    MI_TRY(gftt::emit(per_find, resp, im.cols, masks, segs_x, nseg, bbase, corners->cols, nullptr, (float *)corners->data, st));
    int ctl_host[gftt::GFTT_CTL_INTS] = {};
    MI_HIP_TRY(hipMemcpyAsync(ctl_host, ctl, sizeof(ctl_host), hipMemcpyDeviceToHost, st));
    MI_HIP_TRY(hipStreamSynchronize(st));
    *count = ctl_host[gftt::GFTT_CTL_COUNT];
    return MI_OK;
}

int mi_gftt_sort(const mi_mat *response, const mi_mat *corners, int n, mi_mat *sorted, void *stream)
{
    MI_REQUIRE(response && corners && sorted, MI_ERR_BAD_ARG, "null argument");
    MI_TRY(gftt::gftt_fail(gftt::gftt_check_f32(desc_of(response), response->rows, response->cols, "response must be CV_32FC1")));
    gftt::GfttImage im;
    MI_TRY(check_frame(response, MI_32FC1, nullptr, &im, nullptr));
    MI_REQUIRE(n >= 1 && n <= (1 << 30), MI_ERR_BAD_SIZE, "1 <= n <= 2^30");
    MI_REQUIRE(corners->data && corners->type == MI_32FC2 && corners->rows == 1 && corners->cols >= n, MI_ERR_BAD_SIZE,
               "corners must be 1 x (at least n) CV_32FC2");
    MI_REQUIRE(sorted->data && sorted->type == MI_32FC2 && sorted->rows == 1 && sorted->cols >= n, MI_ERR_BAD_SIZE,
               "sorted must be 1 x (at least n) CV_32FC2");
    MI_TRY(require_device());
    hipStream_t st = (hipStream_t)stream;
    // a point outside the plane would be read outside it: look first (a stage entry; the class sorts what it found itself)
    std::vector<float> hp((size_t)2 * n);
    MI_HIP_TRY(hipMemcpyAsync(hp.data(), corners->data, hp.size() * sizeof(float), hipMemcpyDeviceToHost, st));
    MI_HIP_TRY(hipStreamSynchronize(st));
    for (int i = 0; i < n; ++i)
        MI_REQUIRE(hp[2 * i] >= 0 && hp[2 * i] < im.cols && hp[2 * i + 1] >= 0 && hp[2 * i + 1] < im.rows, MI_ERR_BAD_ARG,
                   "corner %d lies outside the response plane", i);
    const int sort_cap = gftt::gftt_pow2_ceil(n > gftt::GFTT_SORT_TILE ? n : gftt::GFTT_SORT_TILE);
    const size_t o_keys = gftt::gftt_align(gftt::GFTT_CTL_INTS * sizeof(int));
    DevTmp tmp;
    unsigned char *s;
    MI_TRY(tmp.alloc(&s, o_keys + (size_t)sort_cap * 8));
    int *ctl = (int *)s;
    unsigned long long *keys = (unsigned long long *)(s + o_keys);
    MI_TRY(gftt::make_keys({(float *)response->data, (long long)response->step}, im.cols, (const float *)corners->data, n, keys, ctl, st));
    std::vector<gftt::GfttLaunch> launches;
    gftt::gftt_sort_launches(sort_cap, &launches);
    for (const gftt::GfttLaunch &k : launches) MI_TRY(gftt::sort_step(k, keys, ctl, st));
    MI_TRY(gftt::points({gftt::GFTT_K_POINTS, (unsigned)div_up(n, gftt::GFTT_BLOCK), 1, gftt::GFTT_BLOCK, 0, 0, 0}, keys, im.cols, 0,
                        (float *)sorted->data, ctl, st));
    MI_HIP_TRY(hipStreamSynchronize(st));
    return MI_OK;
}

int mi_gftt_min_distance(const float *points, int total, int rows, int cols, double min_distance, int max_corners, float *out, int *n_out)
{
    MI_REQUIRE(points && out && n_out, MI_ERR_BAD_ARG, "null argument");
    MI_REQUIRE(total >= 0 && rows >= 1 && cols >= 1, MI_ERR_BAD_SIZE, "total >= 0, rows >= 1, cols >= 1");
    MI_REQUIRE(min_distance >= 1 && min_distance < 1073741824.0 && max_corners >= 0, MI_ERR_BAD_ARG,
               "1 <= minDistance < 2^30 (below 1 the reference copies the head, gftt.cpp:134-137), maxCorners >= 0");
    std::vector<float> kept;
    gftt::gftt_min_distance(points, total, rows, cols, min_distance, max_corners, &kept);
    std::memcpy(out, kept.data(), kept.size() * sizeof(float));
    *n_out = (int)(kept.size() / 2);
    return MI_OK;
}

}  // extern "C"
