// cv::cuda::SURF_CUDA: handle + C-ABI entry points.  Host-side twin of SURF_CUDA_Invoker
// (modules/xfeatures2d/src/surf.cuda.cpp:134-255): validation, integral(s), octave loop, orientation, descriptors.
// One stream, no host round trip inside the octave loop; the only synchronisation is the final read-back of the
// feature count (the reference's keypoints.cols = featureCounter, :205-209).
#include "surf_dev.h"
#include <cstdlib>
#include "mi_selftest.h"
#include <cmath>
#include <vector>

using namespace mi;

struct mi_surf {
    mi_surf_params P;
    // tables (surf.cpp:544-565 generators; see oracle/surf_ref.c for the correspondence with surf.cu:520-522,685-707)
    DevBuf<float> apt, dw;
    DevBuf<unsigned> counters;                // 64 (DetectBufs::counters): the handle's for life, like the tables
    // what a detect call runs and on which buffers (surf_plan.h): the plan of the last frame's shape, made with the switches as they
    // were when the scratch was allocated (this handle's decision: no process-global state); shape.rows == 0: no scratch
    surf::SurfPlan plan = {};
    surf::SurfKnobs knobs = {};
    // the scratch of the plan, one allocation per region; msum comes with the first masked call
    struct Scratch {
        DevBuf<unsigned> sum, msum, V, BT, poly, rowcnt, segcnt;
        DevBuf<float> det, trace;
        DevBuf<unsigned long long> bits, sbits;
        DevBuf<int4> cand;
        DevBuf<unsigned char> itmp, geo;
        void release()
        {
            sum.release(); msum.release(); V.release(); BT.release(); poly.release(); rowcnt.release(); segcnt.release();
            det.release(); trace.release(); bits.release(); sbits.release(); cand.release(); itmp.release(); geo.release();
        }
    } S;
    surf::DetectBufs B = {};                  // what the kernels are handed: the owners' pointers as of the last ensure()
    int capCand = 0;                          // candidates the lists were allocated for (>= plan.shape.max_candidates)
    std::vector<surf::HaarGeo> geo_host;      // source of the asynchronous upload: outlives the call
    bool geo_dirty = false;
};

using surf::calc_size;

// The Gaussian kernel behind surf.cu's literal weight tables (c_aptW :522, c_DW :685-707): cv::getGaussianKernel(n, sigma, CV_32F) as
// OpenCV 2.4 rounded it -- exp() in double rounded to float, the float terms summed in double, float * (1 / sum) in double rounded to
// float -- for the CPU class's float sigmas promoted to double.  The outer products below reproduce every literal bit for bit
// (tests/test_ref_pin_cuda.py::test_surf_weight_tables_equal_the_literals_of_surf_cu checks the same generator in the oracle against the
// parsed reference file).
static void gauss_tab(int n, float sigma_f, float *k)
{
    const double sigma = (double)sigma_f, scale2 = -0.5 / (sigma * sigma);
    double sum = 0;
    for (int i = 0; i < n; ++i) { const double x = i - (n - 1) * 0.5; k[i] = (float)std::exp(scale2 * x * x); sum += k[i]; }
    sum = 1. / sum;
    for (int i = 0; i < n; ++i) k[i] = (float)(k[i] * sum);
}

extern "C" {

void mi_surf_default_params(mi_surf_params *p)
{
    if (!p) return;
    // SURF_CUDA::create(thr, nOctaves=4, nOctaveLayers=2, extended=false, keypointsRatio=0.01f, upright=false), cuda.hpp:117-118
    p->hessian_threshold = 100; p->n_octaves = 4; p->n_octave_layers = 2; p->extended = 0; p->keypoints_ratio = 0.01f; p->upright = 0;
}

int mi_surf_create(const mi_surf_params *p, mi_surf **out)
{
    MI_REQUIRE(out, MI_ERR_BAD_ARG, "null out");
    *out = nullptr;
    MI_TRY(require_device());
    mi_surf *h = new mi_surf();
    if (p) h->P = *p; else mi_surf_default_params(&h->P);
    // orientation samples: disc of radius 6 (c_aptX / c_aptY, surf.cu:520-521), weights c_aptW (:522) = outer product of the 13-tap
    // kernel for sigma 2.5f; descriptor weights c_DW (:685-707) = outer product of the 20-tap kernel for sigma 3.3f
    float g[13], G[20], apt[3 * 113], dw[400];
    gauss_tab(13, 2.5f, g);
    int k = 0;
    for (int i = -6; i <= 6; i++)
        for (int j = -6; j <= 6; j++)
            if (i * i + j * j <= 36) { apt[k] = (float)i; apt[113 + k] = (float)j; apt[226 + k] = g[i + 6] * g[j + 6]; ++k; }
    gauss_tab(20, 3.3f, G);
    for (int i = 0; i < 20; i++) for (int j = 0; j < 20; j++) dw[i * 20 + j] = G[i] * G[j];
    auto upload = [&]() -> int {
        MI_TRY(h->apt.ensure(3 * 113));
        MI_TRY(h->dw.ensure(400));
        MI_HIP_TRY(hipMemcpy(h->apt.p, apt, sizeof(apt), hipMemcpyHostToDevice));
        MI_HIP_TRY(hipMemcpy(h->dw.p, dw, sizeof(dw), hipMemcpyHostToDevice));
        MI_TRY(h->counters.ensure(64));
        h->B.counters = h->counters.p;
        return MI_OK;
    };
    if (const int rc = upload()) { mi_surf_destroy(h); return rc; }
    *out = h;
    return MI_OK;
}

int mi_surf_set_params(mi_surf *h, const mi_surf_params *p) { MI_REQUIRE(h && p, MI_ERR_BAD_ARG, "null argument"); h->P = *p; return MI_OK; }
int mi_surf_get_params(const mi_surf *h, mi_surf_params *p) { MI_REQUIRE(h && p, MI_ERR_BAD_ARG, "null argument"); *p = h->P; return MI_OK; }

static void free_scratch(mi_surf *h)
{
    h->S.release();
    h->B = surf::DetectBufs();
    h->B.counters = h->counters.p;
    h->plan = surf::SurfPlan();
    h->capCand = 0;
}

void mi_surf_release_memory(mi_surf *h) { if (h) free_scratch(h); }   // SURF_CUDA::releaseMemory, surf.cuda.cpp:434-442

void mi_surf_destroy(mi_surf *h)
{
    delete h;
}

int mi_surf_descriptor_size(const mi_surf *h) { return h && h->P.extended ? 128 : 64; }   // surf.cuda.cpp:277-280

// limits of SURF_CUDA_Invoker's constructor, surf.cuda.cpp:137-156
static int limits(const mi_surf_params &P, int rows, int cols, int *maxFeatures, int *maxCandidates)
{
    MI_REQUIRE(P.n_octaves > 0 && P.n_octave_layers > 0, MI_ERR_BAD_ARG, "nOctaves and nOctaveLayers must be > 0");          // :141
    MI_REQUIRE(P.n_octaves <= 16 && P.n_octave_layers <= 16, MI_ERR_BAD_ARG, "nOctaves / nOctaveLayers too large");
    const int min_size = calc_size(P.n_octaves - 1, 0);
    MI_REQUIRE(rows - min_size >= 0 && cols - min_size >= 0, MI_ERR_BAD_SIZE, "image too small for nOctaves");               // :144-145
    const int lr = rows >> (P.n_octaves - 1), lc = cols >> (P.n_octaves - 1);
    const int min_margin = ((calc_size(P.n_octaves - 1, 2) >> 1) >> (P.n_octaves - 1)) + 1;
    MI_REQUIRE(lr - 2 * min_margin > 0 && lc - 2 * min_margin > 0, MI_ERR_BAD_SIZE, "image too small for nOctaves");         // :150-151
    int mf = (int)((float)(rows * cols) * P.keypoints_ratio);                                                               // :153
    if (mf > 65535) mf = 65535;
    int mc = (int)(1.5 * mf);
    if (mc > 65535) mc = 65535;
    MI_REQUIRE(mf > 0, MI_ERR_BAD_ARG, "maxFeatures <= 0 (keypointsRatio too small)");                                        // :156
    *maxFeatures = mf; *maxCandidates = mc;
    return MI_OK;
}

int mi_surf_max_features(const mi_surf *h, int rows, int cols, int *max_features)
{
    MI_REQUIRE(h && max_features, MI_ERR_BAD_ARG, "null argument");
    int mc;
    return limits(h->P, rows, cols, max_features, &mc);
}

// The switches of the plan, read when a handle (re-)allocates its scratch.  MIFLOW_SURF_FUSED / _LDS exist in the experiments build only;
// MIFLOW_SURF_NMS0=1 is the round 5 experiment kept as a tested opt-in: octave 0's maxima flagged inside the det kernel, no det / trace
// planes for three quarters of the samples.  Bit-identical, but SLOWER on MI355X (r14j, 4K frame: k_det_nms0 180 us against 103 + 65 us
// for the tile kernel + the flag launch -- the 18 % of overlapping samples cost more than the planes' 265 MB -- and the refinement's 27
// re-evaluations per candidate 143 us against 15): 736 against 826 frames/s.  MIFLOW_SURF_POLY=0 keeps the strided gathers of octaves
// >= 1 instead of the polyphase planes of round 5 (bit-identical either way).
static surf::SurfKnobs read_knobs()
{
    static const bool lds_ok = surf::lds_geometry_self_check();   // the LDS path's compile-time geometry against the host's
    const char *f = MI_EXP_ENV("MIFLOW_SURF_FUSED"), *l = MI_EXP_ENV("MIFLOW_SURF_LDS"), *n0 = getenv("MIFLOW_SURF_NMS0"), *pp = getenv("MIFLOW_SURF_POLY");
    surf::SurfKnobs K;
    K.fused = !(f && atoi(f) == 0);
    K.lds = !(l && atoi(l) == 0);
    K.nms0 = n0 && *n0 && atoi(n0) != 0;
    K.poly = !(pp && *pp && atoi(pp) == 0);
    K.lds_ok = lds_ok;
    return K;
}

static int ensure(mi_surf *h, int rows, int cols, int maxCand, bool need_mask, hipStream_t st)
{
    // the plan (launch forms, region sizes, the geometry table) is that of EXACTLY this shape: a handle whose nOctaveLayers was lowered
    // re-plans instead of running on the larger plan's table.  Only candidate lists that are large enough are kept.
    const surf::SurfShape Z = {rows, cols, h->P.n_octaves, h->P.n_octave_layers, maxCand};
    if (!(Z == h->plan.shape)) {
        surf::SurfShape held = h->plan.shape;
        held.max_candidates = maxCand;
        if (held == Z && h->capCand >= maxCand) h->plan = surf::surf_make_plan(Z, h->knobs);
        else {
            free_scratch(h);
            h->knobs = read_knobs();
            const surf::SurfPlan p = surf::surf_make_plan(Z, h->knobs);
            mi_surf::Scratch &S = h->S;   // empty here, so each region gets exactly the plan's size (a count of 0: none)
            MI_TRY(S.sum.ensure(p.sum_words));
            MI_TRY(S.V.ensure(p.v_words));
            MI_TRY(S.BT.ensure(p.bt_words));
            MI_TRY(S.det.ensure(p.plane_floats));
            MI_TRY(S.trace.ensure(p.plane_floats));
            MI_TRY(S.bits.ensure(p.bits_words));
            MI_TRY(S.sbits.ensure(p.sbits_words));
            MI_TRY(S.rowcnt.ensure(p.row_counts));
            MI_TRY(S.segcnt.ensure(p.seg_counts));
            MI_TRY(S.cand.ensure(p.cand_items));
            MI_TRY(S.itmp.ensure(surf::interp_tmp_bytes(p.cand_items)));
            if (p.fused) {
                h->geo_host.resize(p.geo_bytes / sizeof(surf::HaarGeo));
                surf::surf_fill_geometry(p, h->geo_host.data());
                MI_TRY(S.poly.ensure(p.poly_words));
                MI_TRY(S.geo.ensure(p.geo_bytes));
                h->geo_dirty = true;
            }
            h->plan = p;   // (an allocation that failed leaves the handle without a plan)
            h->capCand = maxCand;
        }
    }
    if (need_mask) MI_TRY(h->S.msum.ensure(h->plan.sum_words));
    const mi_surf::Scratch &S = h->S;
    h->B = {S.sum.p, S.msum.p, S.V.p, S.BT.p, S.poly.p, S.det.p, S.trace.p, S.bits.p, S.sbits.p, S.rowcnt.p, S.segcnt.p, S.cand.p, S.itmp.p,
            S.geo.p, h->counters.p};
    if (h->geo_dirty) {   // on the call's stream, not a blocking null-stream copy
        MI_HIP_TRY(hipMemcpyAsync(h->B.geo, h->geo_host.data(), h->plan.geo_bytes, hipMemcpyHostToDevice, st));
        h->geo_dirty = false;
    }
    return MI_OK;
}

static int check_img(const mi_mat *m, const char *name)
{
    MI_REQUIRE(m && m->data, MI_ERR_BAD_ARG, "%s: empty", name);
    MI_REQUIRE(m->type == MI_8UC1, MI_ERR_BAD_TYPE, "%s: must be CV_8UC1", name);   // surf.cuda.cpp:139
    MI_REQUIRE(m->rows > 0 && m->cols > 0 && m->step >= (size_t)m->cols, MI_ERR_BAD_ARG, "%s: bad size/step", name);
    return MI_OK;
}
static int check_kp(const mi_mat *kp, int min_cols)
{
    MI_REQUIRE(kp && kp->data && kp->type == MI_32FC1 && kp->rows == 7 && kp->cols >= min_cols && kp->step % 4 == 0 &&
               kp->step >= (size_t)kp->cols * 4, MI_ERR_BAD_ARG, "keypoints must be CV_32FC1 with ROWS_COUNT = 7 rows and enough columns");
    return MI_OK;
}

// Everything of SURF_CUDA_Invoker's detectKeypoints + findOrientation enqueued on `st`; the feature count stays on the device
// (h->B.counters[0]).  *max_features = the bound the keypoint matrix was checked against.
static int detect_enqueue(mi_surf *h, const mi_mat *img, const mi_mat *mask, mi_mat *keypoints, int *max_features, hipStream_t st)
{
    const mi_surf_params &P = h->P;
    int rc;
    if ((rc = check_img(img, "img"))) return rc;
    const bool use_mask = mask && mask->data;
    if (use_mask) {
        if ((rc = check_img(mask, "mask"))) return rc;
        MI_REQUIRE(mask->rows == img->rows && mask->cols == img->cols, MI_ERR_BAD_SIZE, "mask.size() != img.size()");   // :140
    }
    const int rows = img->rows, cols = img->cols;
    int maxF, maxC;
    if ((rc = limits(P, rows, cols, &maxF, &maxC))) return rc;
    if ((rc = check_kp(keypoints, maxF))) return rc;
    if ((rc = ensure(h, rows, cols, maxC, use_mask, st))) return rc;
    const surf::SurfPlan &Q = h->plan;
    surf::DetectBufs B = h->B;
    if (!use_mask) B.msum = nullptr;
    const int kld = (int)(keypoints->step / 4);
    float *kp = (float *)keypoints->data;

    MI_HIP_TRY(hipMemsetAsync(B.counters, 0, sizeof(unsigned) * 64, st));                                            // :158-159
    if ((rc = surf::integral((const unsigned char *)img->data, (long long)img->step, rows, cols, false, B.V, B.BT, Q.vld, B.sum, Q.sld, st))) return rc;   // :163
    if (use_mask && (rc = surf::integral((const unsigned char *)mask->data, (long long)mask->step, rows, cols, true, B.V, B.BT, Q.vld, B.msum, Q.sld, st)))
        return rc;                                                                                                    // :165-169
    MI_HIP_TRY(hipMemset2DAsync(kp, keypoints->step, 0, (size_t)maxF * 4, 7, st));                                   // keypoints.setTo(0) :180
    if (Q.fused) {                                                                                                   // :182-204, all octaves per launch
        if ((rc = surf::detect_all(Q, B, (float)P.hessian_threshold, kp, kld, maxF, st))) return rc;
    } else
    for (int octave = 0; octave < P.n_octaves; ++octave) {                                                           // :182-204
        unsigned *const ncand = B.counters + 1 + octave;
        if ((rc = surf::det_trace(B.sum, Q.sld, rows, cols, octave, P.n_octave_layers, B.det, B.trace, Q.dld, st))) return rc;
        if ((rc = surf::find_maxima(B.det, B.trace, Q.dld, B.msum, Q.sld, rows, cols, octave, P.n_octave_layers,
                                    (float)P.hessian_threshold, B.bits, B.rowcnt, B.segcnt, B.cand, maxC, ncand, st))) return rc;
        if ((rc = surf::interpolate(B.det, Q.dld, rows, cols, octave, B.cand, ncand, maxC, B.itmp, kp, kld, maxF, B.counters, st))) return rc;
    }
    if ((rc = surf::orientation(B.sum, Q.sld, rows, cols, kp, kld, B.counters, maxF, P.upright != 0, h->apt.p, st))) return rc;   // :211-214
    *max_features = maxF;
    return MI_OK;
}

static int read_count(mi_surf *h, int maxF, int *n_features, hipStream_t st)
{
    unsigned nf = 0;
    MI_HIP_TRY(hipMemcpyAsync(&nf, h->B.counters, sizeof(unsigned), hipMemcpyDeviceToHost, st));                       // :205-207
    MI_HIP_TRY(hipStreamSynchronize(st));
    *n_features = (int)(nf < (unsigned)maxF ? nf : (unsigned)maxF);
    return MI_OK;
}

int mi_surf_detect(mi_surf *h, const mi_mat *img, const mi_mat *mask, mi_mat *keypoints, int *n_features, void *stream)
{
    MI_REQUIRE(h && n_features, MI_ERR_BAD_ARG, "null argument");
    hipStream_t st = (hipStream_t)stream;
    int maxF = 0;
    if (const int rc = detect_enqueue(h, img, mask, keypoints, &maxF, st)) return rc;
    return read_count(h, maxF, n_features, st);
}

// detect + describe with the feature count left on the device between the two (round 5): the reference's operator()(img, mask,
// keypoints, descriptors) reads keypoints.cols back before it launches compute_descriptors (surf.cuda.cpp:205-209, 227-236) -- a host
// round trip in the middle of every frame.  Here the descriptor kernels read the count themselves; the one synchronisation that
// returns it to the caller comes after everything is enqueued.  descriptors: at least max_features rows.
int mi_surf_detect_and_compute(mi_surf *h, const mi_mat *img, const mi_mat *mask, mi_mat *keypoints, mi_mat *descriptors, int *n_features, void *stream)
{
    MI_REQUIRE(h && n_features, MI_ERR_BAD_ARG, "null argument");
    hipStream_t st = (hipStream_t)stream;
    int maxF = 0, rc;
    if ((rc = check_img(img, "img"))) return rc;
    {
        int mc;
        if ((rc = limits(h->P, img->rows, img->cols, &maxF, &mc))) return rc;
    }
    const int dsz = h->P.extended ? 128 : 64;
    MI_REQUIRE(descriptors && descriptors->data && descriptors->type == MI_32FC1 && descriptors->rows >= maxF && descriptors->cols == dsz &&
               descriptors->step % 4 == 0 && descriptors->step >= (size_t)dsz * 4, MI_ERR_BAD_ARG,
               "descriptors must be CV_32FC1 with at least maxFeatures rows and descriptorSize() columns");
    if ((rc = detect_enqueue(h, img, mask, keypoints, &maxF, st))) return rc;
    if ((rc = surf::descriptors((const unsigned char *)img->data, (long long)img->step, img->rows, img->cols, (const float *)keypoints->data,
                                (int)(keypoints->step / 4), maxF, h->P.extended != 0, (float *)descriptors->data,
                                (long long)(descriptors->step / 4), h->dw.p, st, h->B.counters))) return rc;
    return read_count(h, maxF, n_features, st);
}

// n frames through one handle (masks may be NULL, or hold NULL-data entries).  A 4K frame fills the device and the feature
// count of every frame is read back like SURF_CUDA does (surf.cuda.cpp:205-207), so this is a loop sharing the handle's scratch.
int mi_surf_detect_batch(mi_surf *h, int n, const mi_mat *imgs, const mi_mat *masks, mi_mat *keypoints, int *n_features, void *stream)
{
    MI_REQUIRE(h && n > 0 && imgs && keypoints && n_features, MI_ERR_BAD_ARG, "empty batch");
    for (int i = 0; i < n; ++i) {
        const int rc = mi_surf_detect(h, &imgs[i], masks ? &masks[i] : nullptr, &keypoints[i], &n_features[i], stream);
        if (rc) return rc;
    }
    return MI_OK;
}

int mi_surf_compute_orientation(mi_surf *h, const mi_mat *img, mi_mat *keypoints, int n_features, void *stream)
{
    MI_REQUIRE(h, MI_ERR_BAD_ARG, "null handle");
    hipStream_t st = (hipStream_t)stream;
    int rc;
    if ((rc = check_img(img, "img")) || (rc = check_kp(keypoints, n_features))) return rc;
    if (n_features <= 0) return MI_OK;
    const int rows = img->rows, cols = img->cols;
    int maxF, maxC;
    if ((rc = limits(h->P, rows, cols, &maxF, &maxC))) return rc;
    if ((rc = ensure(h, rows, cols, maxC, false, st))) return rc;
    if ((rc = surf::integral((const unsigned char *)img->data, (long long)img->step, rows, cols, false, h->B.V, h->B.BT, h->plan.vld, h->B.sum, h->plan.sld, st))) return rc;
    return surf::orientation(h->B.sum, h->plan.sld, rows, cols, (float *)keypoints->data, (int)(keypoints->step / 4), nullptr, n_features,
                             h->P.upright != 0, h->apt.p, st);
}

int mi_surf_compute_descriptors(mi_surf *h, const mi_mat *img, const mi_mat *keypoints, int n_features, mi_mat *descriptors, void *stream)
{
    MI_REQUIRE(h, MI_ERR_BAD_ARG, "null handle");
    int rc;
    if ((rc = check_img(img, "img")) || (rc = check_kp(keypoints, n_features))) return rc;
    if (n_features <= 0) return MI_OK;
    const int dsz = h->P.extended ? 128 : 64;
    MI_REQUIRE(descriptors && descriptors->data && descriptors->type == MI_32FC1 && descriptors->rows >= n_features && descriptors->cols == dsz &&
               descriptors->step % 4 == 0, MI_ERR_BAD_ARG, "descriptors must be CV_32FC1, nFeatures x descriptorSize()");   // :232
    return surf::descriptors((const unsigned char *)img->data, (long long)img->step, img->rows, img->cols, (const float *)keypoints->data,
                             (int)(keypoints->step / 4), n_features, h->P.extended != 0, (float *)descriptors->data,
                             (long long)(descriptors->step / 4), h->dw.p, (hipStream_t)stream);
}

// ---- stage-level entry points (parity tests)
int mi_surf_integral(mi_surf *h, const mi_mat *img, int clamp_to_one, mi_mat *sum, void *stream)
{
    MI_REQUIRE(h, MI_ERR_BAD_ARG, "null handle");
    hipStream_t st = (hipStream_t)stream;
    int rc;
    if ((rc = check_img(img, "img"))) return rc;
    MI_REQUIRE(sum && sum->data && sum->type == MI_32SC1 && sum->rows == img->rows + 1 && sum->cols == img->cols + 1 && sum->step % 4 == 0,
               MI_ERR_BAD_ARG, "sum must be CV_32SC1 (rows+1) x (cols+1)");   // cuda::integral, cudaarithm/src/cuda/integral.cu:62-83
    const int vld = align_up(img->cols, 64);
    unsigned *V = nullptr, *BT = nullptr;
    DevTmp tmp;
    MI_TRY(tmp.alloc(&V, (size_t)vld * img->rows));
    MI_TRY(tmp.alloc(&BT, (size_t)vld * surf::integral_bands(img->rows)));
    rc = surf::integral((const unsigned char *)img->data, (long long)img->step, img->rows, img->cols, clamp_to_one != 0, V, BT, vld,
                        (unsigned *)sum->data, (int)(sum->step / 4), st);
    if (rc) return rc;
    MI_HIP_TRY(hipStreamSynchronize(st));   // the temporaries are freed on return: the kernels must be done (and their faults seen)
    return MI_OK;
}

int mi_surf_det_trace(mi_surf *h, const mi_mat *sum, int octave, int n_octave_layers, mi_mat *det, mi_mat *trace, void *stream)
{
    MI_REQUIRE(h, MI_ERR_BAD_ARG, "null handle");
    MI_REQUIRE(sum && sum->data && sum->type == MI_32SC1 && sum->step % 4 == 0 && sum->rows > 1 && sum->cols > 1, MI_ERR_BAD_ARG, "bad sum");
    const int rows = sum->rows - 1, cols = sum->cols - 1, lr = rows >> octave;
    MI_REQUIRE(octave >= 0 && octave < 16 && n_octave_layers > 0 && lr > 0, MI_ERR_BAD_ARG, "bad octave / layers");
    // the class's limits for this octave being its last (surf.cuda.cpp:144-151)
    const int min_size = calc_size(octave, 0), min_margin = ((calc_size(octave, 2) >> 1) >> octave) + 1;
    MI_REQUIRE(rows - min_size >= 0 && cols - min_size >= 0 && lr - 2 * min_margin > 0 && (cols >> octave) - 2 * min_margin > 0, MI_ERR_BAD_SIZE,
               "image too small for this octave");
    MI_REQUIRE(det && trace && det->data && trace->data && det->type == MI_32FC1 && trace->type == MI_32FC1 &&
               det->rows == (n_octave_layers + 2) * lr && trace->rows == det->rows && det->cols == cols && trace->cols == cols &&
               det->step == trace->step && det->step % 4 == 0, MI_ERR_BAD_ARG, "det/trace must be CV_32FC1 ((layers+2)*layer_rows) x cols, same step");
    return surf::det_trace((const unsigned *)sum->data, (int)(sum->step / 4), rows, cols, octave, n_octave_layers, (float *)det->data,
                           (float *)trace->data, (int)(det->step / 4), (hipStream_t)stream);
}

int miflow_selftest_wave_scan(const unsigned *in_host, unsigned *out_host)
{
    MI_REQUIRE(in_host && out_host, MI_ERR_BAD_ARG, "null argument");
    unsigned *d = nullptr;
    DevTmp tmp;
    MI_TRY(tmp.alloc(&d, 128));
    MI_HIP_TRY(hipMemcpy(d, in_host, sizeof(unsigned) * 64, hipMemcpyHostToDevice));
    int rc = surf::dbg_scan(d, d + 64, nullptr);
    if (!rc) { MI_HIP_TRY(hipDeviceSynchronize()); MI_HIP_TRY(hipMemcpy(out_host, d + 64, sizeof(unsigned) * 64, hipMemcpyDeviceToHost)); }
    return rc;
}

int miflow_selftest_surf_libm(const float *a_host, const float *b_host, int n, float *atan2_host, float *sin_host, float *cos_host)
{
    MI_REQUIRE(a_host && b_host && atan2_host && sin_host && cos_host, MI_ERR_BAD_ARG, "null argument");
    MI_REQUIRE(n > 0 && n <= (1 << 22), MI_ERR_BAD_ARG, "n must be in 1 .. 2^22");
    float *d = nullptr;
    DevTmp tmp;
    const size_t N = (size_t)n;
    MI_TRY(tmp.alloc(&d, 5 * N));
    MI_HIP_TRY(hipMemcpy(d, a_host, sizeof(float) * N, hipMemcpyHostToDevice));
    MI_HIP_TRY(hipMemcpy(d + N, b_host, sizeof(float) * N, hipMemcpyHostToDevice));
    MI_TRY(surf::dbg_libm(d, d + N, n, d + 2 * N, d + 3 * N, d + 4 * N, nullptr));
    MI_HIP_TRY(hipDeviceSynchronize());
    MI_HIP_TRY(hipMemcpy(atan2_host, d + 2 * N, sizeof(float) * N, hipMemcpyDeviceToHost));
    MI_HIP_TRY(hipMemcpy(sin_host, d + 3 * N, sizeof(float) * N, hipMemcpyDeviceToHost));
    MI_HIP_TRY(hipMemcpy(cos_host, d + 4 * N, sizeof(float) * N, hipMemcpyDeviceToHost));
    return MI_OK;
}

}  // extern "C"
