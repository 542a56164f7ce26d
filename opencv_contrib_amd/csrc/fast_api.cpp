// cv::cuda::FastFeatureDetector: handle + C-ABI entry points.  Host-side twin of FAST_Impl (modules/cudafeatures2d/src/fast.cpp:96-215):
// validation, the plan (fast_plan.h), scratch, the plan's launches in order on the caller's stream, and ONE read-back of the counts at
// the end of a call (the reference waits twice: fast.cu:297-301, :364-368).
#include "fast_dev.h"
#include "mi_buf.h"

using namespace mi;

struct mi_fast {
    mi_fast_params P;
    DevBuf<unsigned char> scratch;                 // counts, then one frame area (fast_plan.h)
    PinnedBuf<int, hipHostMallocDefault> counts;   // the read-back's landing place
};

namespace {

fast::FastMatDesc desc_of(const mi_mat *m) { return {m->rows, m->cols, m->type, m->step, m->data != nullptr}; }

int check_frame(const mi_mat *img, const mi_mat *mask, fast::FastImage *im)
{
    MI_REQUIRE(img, MI_ERR_BAD_ARG, "null image");
    const bool masked = mask && mask->data;
    fast::FastMatDesc md = {};
    if (masked) md = desc_of(mask);
    MI_TRY(fast::fast_fail(fast::fast_check_image(desc_of(img), masked ? &md : nullptr)));
    *im = {(const unsigned char *)img->data, (long long)img->step, masked ? (const unsigned char *)mask->data : nullptr,
           masked ? (long long)mask->step : 0, img->rows, img->cols};
    return MI_OK;
}

fast::FastScratch frame_scratch(unsigned char *base, const fast::FastPlan &plan, int frame)
{
    const fast::FastFrame &f = plan.frames[frame];
    unsigned char *a = base + plan.counts_bytes;
    return {a + f.off_plane, (unsigned long long *)(a + f.off_cand), (unsigned long long *)(a + f.off_surv), (unsigned long long *)(a + f.off_emit),
            (int *)(a + f.off_pos), (int *)base + 2 * frame};
}

int run_launch(const fast::FastPlan &plan, const fast::FastLaunch &k, const fast::FastImage &im, unsigned char *scratch, const mi_mat *kp,
               hipStream_t st)
{
    const fast::FastFrame &f = plan.frames[k.frame];
    const fast::FastScratch s = frame_scratch(scratch, plan, k.frame);
    switch (k.kernel) {
    case fast::FAST_K_SCORE: return fast::score(k, f, im, plan.threshold, s, st);
    case fast::FAST_K_NMS: return fast::nms(k, f, s, st);
    case fast::FAST_K_SCAN: return fast::scan(k, f, s, plan.nms != 0, plan.max_npoints, st);
    case fast::FAST_K_EMIT:
        return fast::emit(k, f, s, plan.nms != 0, (unsigned char *)kp->data + fast::FAST_LOCATION_ROW * kp->step,
                          (float *)((unsigned char *)kp->data + fast::FAST_RESPONSE_ROW * kp->step), st);
    }
    MI_REQUIRE(false, MI_ERR_BAD_ARG, "unknown launch");
    return MI_OK;
}

int detect_n(mi_fast *h, int n, const mi_mat *imgs, const mi_mat *masks, mi_mat *kps, int *ns, void *stream)
{
    MI_REQUIRE(h, MI_ERR_BAD_ARG, "null handle");
    MI_REQUIRE(n >= 1 && imgs && kps && ns, MI_ERR_BAD_ARG, "n >= 1 and non-null imgs, keypoints, ns");
    const mi_fast_params &P = h->P;
    std::vector<fast::FastImage> im(n);
    std::vector<int> sizes(2 * n);
    for (int i = 0; i < n; ++i) {
        MI_TRY(check_frame(&imgs[i], masks ? &masks[i] : nullptr, &im[i]));
        MI_TRY(fast::fast_fail(fast::fast_check_keypoints(desc_of(&kps[i]), P.max_npoints)));
        sizes[2 * i] = imgs[i].rows; sizes[2 * i + 1] = imgs[i].cols;
    }
    const fast::FastPlan plan = fast::fast_make_plan(n, sizes.data(), P.threshold, P.nonmax_suppression, P.max_npoints);
    MI_TRY(fast::fast_fail(plan.err));
    for (int i = 0; i < n; ++i) ns[i] = 0;
    if (plan.launches.empty()) return MI_OK;   // every frame is smaller than a ring
    hipStream_t st = (hipStream_t)stream;
    MI_TRY(h->scratch.ensure(plan.scratch_bytes));
    MI_TRY(h->counts.ensure((size_t)2 * n));
    for (const fast::FastLaunch &k : plan.launches) MI_TRY(run_launch(plan, k, im[k.frame], h->scratch.p, &kps[k.frame], st));
    // degenerate frames have no launch and no count: their slots are never read
    MI_HIP_TRY(hipMemcpyAsync(h->counts.p, h->scratch.p, (size_t)2 * n * sizeof(int), hipMemcpyDeviceToHost, st));
    MI_HIP_TRY(hipStreamSynchronize(st));
    for (int i = 0; i < n; ++i)
        if (!plan.frames[i].degenerate) ns[i] = h->counts.p[2 * i + 1];
    return MI_OK;
}

}  // namespace

extern "C" {

void mi_fast_default_params(mi_fast_params *p)
{
    if (!p) return;
    p->threshold = 10; p->nonmax_suppression = 1; p->max_npoints = 5000;   // FastFeatureDetector::create, cudafeatures2d.hpp:434-437
}

int mi_fast_create(const mi_fast_params *p, mi_fast **out)
{
    MI_REQUIRE(out, MI_ERR_BAD_ARG, "null out");
    *out = nullptr;
    mi_fast_params P;
    if (p) P = *p; else mi_fast_default_params(&P);
    MI_TRY(fast::fast_fail(fast::fast_check_params(P.threshold, P.max_npoints)));
    MI_TRY(require_device());
    mi_fast *h = new mi_fast();
    h->P = P;
    *out = h;
    return MI_OK;
}

int mi_fast_set_params(mi_fast *h, const mi_fast_params *p)
{
    MI_REQUIRE(h && p, MI_ERR_BAD_ARG, "null argument");
    MI_TRY(fast::fast_fail(fast::fast_check_params(p->threshold, p->max_npoints)));
    h->P = *p;
    return MI_OK;
}

int mi_fast_get_params(const mi_fast *h, mi_fast_params *p)
{
    MI_REQUIRE(h && p, MI_ERR_BAD_ARG, "null argument");
    *p = h->P;
    return MI_OK;
}

void mi_fast_destroy(mi_fast *h)
{
    delete h;
}

int mi_fast_scratch_bytes(const mi_fast *h, size_t *bytes)
{
    MI_REQUIRE(h && bytes, MI_ERR_BAD_ARG, "null argument");
    *bytes = h->scratch.n;
    return MI_OK;
}

int mi_fast_detect(mi_fast *h, const mi_mat *img, const mi_mat *mask, mi_mat *keypoints, int *n, void *stream)
{
    return detect_n(h, 1, img, mask, keypoints, n, stream);
}

int mi_fast_detect_batch(mi_fast *h, int n, const mi_mat *imgs, const mi_mat *masks, mi_mat *keypoints, int *ns, void *stream)
{
    return detect_n(h, n, imgs, masks, keypoints, ns, stream);
}

int mi_fast_score(const mi_mat *img, const mi_mat *mask, int threshold, mi_mat *scores, void *stream)
{
    fast::FastImage im;
    MI_TRY(check_frame(img, mask, &im));
    MI_TRY(fast::fast_fail(fast::fast_check_params(threshold, 1)));
    MI_REQUIRE(scores && scores->data, MI_ERR_BAD_ARG, "null scores");
    MI_REQUIRE(scores->type == MI_32SC1, MI_ERR_BAD_TYPE, "scores.type() == CV_32SC1");
    MI_REQUIRE(scores->rows == img->rows && scores->cols == img->cols, MI_ERR_BAD_SIZE, "scores.size() == img.size()");
    MI_REQUIRE(scores->step % 4 == 0 && scores->step >= (size_t)scores->cols * 4, MI_ERR_BAD_ARG, "scores: bad step");
    hipStream_t st = (hipStream_t)stream;
    const int sizes[2] = {img->rows, img->cols};
    const fast::FastPlan plan = fast::fast_make_plan(1, sizes, threshold, 0, 1);
    MI_TRY(fast::fast_fail(plan.err));
    if (plan.frames[0].degenerate) {   // nothing is tested: the plane the reference clears (fast.cpp:140)
        if (img->rows > 0 && img->cols > 0)
            MI_HIP_TRY(hipMemset2DAsync(scores->data, scores->step, 0, (size_t)img->cols * 4, (size_t)img->rows, st));
        return MI_OK;
    }
    DevTmp tmp;
    unsigned char *scratch;
    MI_TRY(tmp.alloc(&scratch, plan.scratch_bytes));
    MI_TRY(fast::score(plan.launches[0], plan.frames[0], im, threshold, frame_scratch(scratch, plan, 0), st));
    MI_TRY(fast::plane_to_scores(plan.frames[0], frame_scratch(scratch, plan, 0).plane, (int *)scores->data, (long long)scores->step, st));
    MI_HIP_TRY(hipStreamSynchronize(st));   // the temporary plane goes with this call
    return MI_OK;
}

int mi_fast_locations_to_points(const mi_mat *keypoints, int n, mi_mat *points, void *stream)
{
    MI_REQUIRE(keypoints && keypoints->data && points && points->data, MI_ERR_BAD_ARG, "null argument");
    MI_REQUIRE(keypoints->rows == fast::FAST_ROWS_COUNT && (keypoints->type == MI_32FC1 || keypoints->type == MI_32SC1), MI_ERR_BAD_TYPE,
               "keypoints.rows == 2 && keypoints.elemSize() == 4");   // fast.cpp:193-194
    MI_REQUIRE(n >= 1 && n <= keypoints->cols, MI_ERR_BAD_SIZE, "1 <= n <= keypoints.cols");
    MI_REQUIRE(points->type == MI_32FC2 && points->rows == 1 && points->cols >= n, MI_ERR_BAD_SIZE, "points must be 1 x (at least n) CV_32FC2");
    return fast::locations_to_points(keypoints->data, n, (float *)points->data, (hipStream_t)stream);
}

}  // extern "C"
