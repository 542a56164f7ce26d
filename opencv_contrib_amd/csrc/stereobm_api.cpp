// cv::cuda::StereoBM: handle + C-ABI entry points.  Host-side twin of StereoBMImpl
// (modules/cudastereo/src/stereobm.cpp:67-197): validation, optional prefilter of both images,
// block matching, textureness post-filter -- all stream-ordered on the caller's stream.
#include "stereobm_dev.h"
#include <vector>
#include <algorithm>
#include "mi_selftest.h"

using namespace mi;

struct mi_stereobm {
    mi_stereobm_params P;
    // scratch owned by the handle (stereobm.cpp:126: minSSD_, leBuf_, riBuf_)
    DevBuf<unsigned> minssd;
    DevBuf<unsigned char> lebuf, ribuf;
    DevBuf<int> tex;      // |Sobel| plane of the textureness filter (extended domain)
    int cap_rows = 0, cap_cols = 0, cap_pairs = 0;   // the per-pair stride of the three above: grown together, never shrunk
    long long step = 0;   // bytes per row of lebuf/ribuf; minssd uses step elements
    // batch: per-pair pointer table (device) and the host copy the asynchronous upload reads
    DevBuf<sbm::BmPair> tab_dev;
    std::vector<sbm::BmPair> tab_host;
};

extern "C" {

void mi_stereobm_default_params(mi_stereobm_params *p)
{
    if (!p) return;
    // createStereoBM(64, 19) cudastereo.hpp:90; StereoBMImpl ctor stereobm.cpp:129-132
    p->num_disparities = 64; p->block_size = 19; p->prefilter_type = MI_PREFILTER_NONE; p->prefilter_cap = 31;
    p->prefilter_size = 9; p->texture_threshold = 3.0f; p->uniqueness_ratio = 0; p->emulate_cuda_edge = 1;
}

int mi_stereobm_create(const mi_stereobm_params *p, mi_stereobm **out)
{
    MI_REQUIRE(out, MI_ERR_BAD_ARG, "null out");
    *out = nullptr;
    MI_TRY(require_device());
    mi_stereobm *h = new mi_stereobm();
    if (p) h->P = *p; else mi_stereobm_default_params(&h->P);
    *out = h;
    return MI_OK;
}

int mi_stereobm_set_params(mi_stereobm *h, const mi_stereobm_params *p)
{
    MI_REQUIRE(h && p, MI_ERR_BAD_ARG, "null argument");
    h->P = *p;   // like the reference's setters: validated at compute() (stereobm.cpp:143-146)
    return MI_OK;
}

int mi_stereobm_get_params(const mi_stereobm *h, mi_stereobm_params *p)
{
    MI_REQUIRE(h && p, MI_ERR_BAD_ARG, "null argument");
    *p = h->P;
    return MI_OK;
}

void mi_stereobm_destroy(mi_stereobm *h)
{
    delete h;
}

static int check_u8(const mi_mat *m, const char *name)
{
    MI_REQUIRE(m && m->data, MI_ERR_BAD_ARG, "%s: null matrix", name);
    MI_REQUIRE(m->type == MI_8UC1, MI_ERR_BAD_TYPE, "%s: must be CV_8UC1", name);   // stereobm.cpp:151
    MI_REQUIRE(m->rows > 0 && m->cols > 0, MI_ERR_BAD_SIZE, "%s: empty", name);
    MI_REQUIRE(m->step >= (size_t)m->cols, MI_ERR_BAD_ARG, "%s: step < cols", name);
    return MI_OK;
}

// two matrices of one size
static int check_same(const mi_mat *a, const char *an, const mi_mat *b, const char *bn, const char *msg = "size mismatch")
{
    MI_TRY(check_u8(a, an)); MI_TRY(check_u8(b, bn));
    MI_REQUIRE(a->rows == b->rows && a->cols == b->cols, MI_ERR_BAD_SIZE, "%s", msg);
    return MI_OK;
}
static int check_pair(const mi_mat *left, const mi_mat *right, const mi_mat *disp)
{
    MI_TRY(check_same(left, "left", right, "right", "left.size() != right.size()"));   // CV_Assert( left.size() == right.size() && left.type() == right.type() )  stereobm.cpp:152
    return check_same(disp, "disparity", left, "left", "disparity.size() != left.size()");
}

static int ensure_scratch(mi_stereobm *h, int rows, int cols, bool need_bufs, int pairs = 1)
{
    if (h->cap_rows < rows || h->cap_cols < cols || h->cap_pairs < pairs) {
        // the stride changes: everything laid out by the old one goes before anything of the new one comes
        h->minssd.release(); h->lebuf.release(); h->ribuf.release(); h->tex.release();
        h->cap_rows = std::max(h->cap_rows, rows); h->cap_cols = std::max(h->cap_cols, cols); h->cap_pairs = std::max(h->cap_pairs, pairs);
        h->step = align_up(h->cap_cols, 256);
    }
    const size_t all_pairs = (size_t)h->step * h->cap_rows * h->cap_pairs;
    MI_TRY(h->minssd.ensure(all_pairs));
    if (need_bufs) {
        MI_TRY(h->lebuf.ensure(all_pairs));
        MI_TRY(h->ribuf.ensure(all_pairs));
    }
    return MI_OK;
}

// stereobm.cpp:164-185: the handle's prefilter (MI_PREFILTER_XSOBEL or _NORMALIZED_RESPONSE) of one image into its scratch plane
static int prefilter(const mi_stereobm *h, const unsigned char *src, long long sstep, unsigned char *dst, int rows, int cols, hipStream_t st)
{
    return h->P.prefilter_type == MI_PREFILTER_XSOBEL ? sbm::prefilter_xsobel(src, sstep, dst, h->step, rows, cols, h->P.prefilter_cap, st)
                                                      : sbm::prefilter_norm(src, sstep, dst, h->step, rows, cols, h->P.prefilter_cap, h->P.prefilter_size, st);
}

// THE pipeline, for n pairs of one size through one handle: checks, scratch, prefilters pair by pair (small, bandwidth-bound kernels),
// zero fill, block matching, textureness post-filter -- all stream-ordered.  One pair goes by its pointers; a batch through a device
// table of the pairs' pointers, so that the zero fill, the block matching -- where the time goes -- and the fused post-filter are ONE
// launch each with blockIdx.z = pair.  A single 1080p pair needs ~16-row bands to put enough waves on the device, and every band
// spends 2R rows building its first window (47 % of the rows at block size 15); the batch supplies the waves, so its bands are up to
// 48 rows tall (23 %; sbm_plan.h bm_band_rows: the cap holds for single pairs and batches alike).
static int run_pairs(mi_stereobm *h, int n, const mi_mat *lefts, const mi_mat *rights, mi_mat *disps, hipStream_t st)
{
    const mi_stereobm_params &P = h->P;
    for (int i = 0; i < n; ++i) {
        MI_TRY(check_pair(&lefts[i], &rights[i], &disps[i]));
        MI_REQUIRE(lefts[i].rows == lefts[0].rows && lefts[i].cols == lefts[0].cols, MI_ERR_BAD_SIZE, "the pairs of a batch must have one size");
    }
    const int rows = lefts[0].rows, cols = lefts[0].cols;
    const sbm::BmPlan plan = sbm::sbm_make_plan(rows, cols, P.num_disparities, P.block_size, P.uniqueness_ratio, n, sbm::bm_switches());
    MI_TRY(sbm::sbm_fail(plan.err));
    const bool pre = P.prefilter_type == MI_PREFILTER_XSOBEL || P.prefilter_type == MI_PREFILTER_NORMALIZED_RESPONSE;
    MI_TRY(ensure_scratch(h, rows, cols, pre, n));
    const long long pp = h->step * h->cap_rows;   // bytes (lebuf / ribuf) = elements (minssd) per pair
    h->tab_host.resize(n);
    for (int i = 0; i < n; ++i) {
        sbm::BmPair &p = h->tab_host[i];
        p = {(const unsigned char *)lefts[i].data, (const unsigned char *)rights[i].data, (unsigned char *)disps[i].data,
             (long long)lefts[i].step, (long long)rights[i].step, (long long)disps[i].step};
        if (pre) {
            unsigned char *lb = h->lebuf.p + i * pp, *rb = h->ribuf.p + i * pp;
            MI_TRY(prefilter(h, p.left, p.lstep, lb, rows, cols, st));
            MI_TRY(prefilter(h, p.right, p.rstep, rb, rows, cols, st));
            p.left = lb; p.right = rb; p.lstep = p.rstep = h->step;
        }
    }
    // the winners' SSDs are the uniqueness pass's input only: without that test nothing reads them and the kernel does not store them
    // (8.3 of the 11.8 MB a 1080p pair's launch wrote, profiles/r10 StereoBM traffic)
    sbm::BmImages img = {h->tab_host[0], nullptr, P.uniqueness_ratio > 0 ? h->minssd.p : nullptr, h->step, pp, P.emulate_cuda_edge};
    const sbm::BmPair &one = img.one;
    // the form: disp := 0 (stereobm.cu:506; the 0xFF fill of minSSD, :507, is not needed -- the kernel writes every element it later reads)
    if (n > 1) {
        MI_TRY(h->tab_dev.ensure(n));
        MI_HIP_TRY(hipMemcpyAsync(h->tab_dev.p, h->tab_host.data(), sizeof(sbm::BmPair) * n, hipMemcpyHostToDevice, st));
        img.tab = h->tab_dev.p;
        MI_TRY(sbm::zero_disp_batch(img.tab, n, rows, cols, st));
    } else
        MI_HIP_TRY(hipMemset2DAsync(one.disp, (size_t)one.dstep, 0, (size_t)cols, (size_t)rows, st));
    MI_TRY(sbm::block_match(img, plan, st));
    if (!(P.texture_threshold > 0)) return MI_OK;                       // stereobm.cpp:189-190
    if (tuning().sbm_texfuse != 0)                                      // one launch (k_textureness_fused)
        return img.tab ? sbm::textureness_fused(nullptr, 0, nullptr, 0, img.tab, n, rows, cols, P.block_size, P.texture_threshold, st)
                       : sbm::textureness_fused(one.left, one.lstep, one.disp, one.dstep, nullptr, 1, rows, cols, P.block_size, P.texture_threshold, st);
    int sld, sh;
    sbm::textureness_scratch_dims(h->cap_rows, h->cap_cols, &sld, &sh);   // the two-pass filter's plane, for the capacity the other scratch has
    MI_TRY(h->tex.ensure((size_t)sld * sh));
    for (const sbm::BmPair &p : h->tab_host)
        MI_TRY(sbm::textureness(p.left, p.lstep, p.disp, p.dstep, rows, cols, P.block_size, P.texture_threshold, h->tex.p, st));
    return MI_OK;
}

int mi_stereobm_compute(mi_stereobm *h, const mi_mat *left, const mi_mat *right, mi_mat *disp, void *stream)
{
    MI_REQUIRE(h, MI_ERR_BAD_ARG, "null handle");
    return run_pairs(h, 1, left, right, disp, (hipStream_t)stream);
}

int mi_stereobm_compute_batch(mi_stereobm *h, int n, const mi_mat *lefts, const mi_mat *rights, mi_mat *disps, void *stream)
{
    MI_REQUIRE(h, MI_ERR_BAD_ARG, "null handle");
    MI_REQUIRE(n > 0 && lefts && rights && disps, MI_ERR_BAD_ARG, "empty batch");
    return run_pairs(h, n, lefts, rights, disps, (hipStream_t)stream);
}

// ---- stage-level entry points (the reference's device-layer functions, stereobm.cpp:54-63)
int mi_stereobm_prefilter_xsobel(const mi_mat *src, mi_mat *dst, int prefilter_cap, void *stream)
{
    MI_TRY(check_same(src, "input", dst, "output"));
    return sbm::prefilter_xsobel((const unsigned char *)src->data, (long long)src->step, (unsigned char *)dst->data,
                                 (long long)dst->step, src->rows, src->cols, prefilter_cap, (hipStream_t)stream);
}

int mi_stereobm_prefilter_norm(const mi_mat *src, mi_mat *dst, int prefilter_cap, int winsize, void *stream)
{
    MI_TRY(check_same(src, "input", dst, "output"));
    return sbm::prefilter_norm((const unsigned char *)src->data, (long long)src->step, (unsigned char *)dst->data,
                               (long long)dst->step, src->rows, src->cols, prefilter_cap, winsize, (hipStream_t)stream);
}

int mi_stereobm_block_match(const mi_mat *left, const mi_mat *right, mi_mat *disp, mi_mat *min_ssd, int ndisp, int winsz,
                            int uniqueness_ratio, int emulate_cuda_edge, void *stream)
{
    MI_TRY(check_pair(left, right, disp));
    MI_REQUIRE(min_ssd && min_ssd->data && min_ssd->type == MI_32SC1 && min_ssd->rows == left->rows && min_ssd->cols == left->cols &&
               min_ssd->step % 4 == 0 && min_ssd->step >= (size_t)left->cols * 4, MI_ERR_BAD_ARG, "min_ssd must be CV_32SC1 of the image size");
    const sbm::BmPlan plan = sbm::sbm_make_plan(left->rows, left->cols, ndisp, winsz, uniqueness_ratio, 1, sbm::bm_switches());
    MI_TRY(sbm::sbm_fail(plan.err));
    hipStream_t st = (hipStream_t)stream;
    MI_HIP_TRY(hipMemset2DAsync(disp->data, disp->step, 0, (size_t)left->cols, (size_t)left->rows, st));
    MI_HIP_TRY(hipMemset2DAsync(min_ssd->data, min_ssd->step, 0xFF, (size_t)left->cols * 4, (size_t)left->rows, st));  // stereobm.cu:507
    const sbm::BmPair one = {(const unsigned char *)left->data, (const unsigned char *)right->data, (unsigned char *)disp->data,
                             (long long)left->step, (long long)right->step, (long long)disp->step};
    return sbm::block_match({one, nullptr, (unsigned *)min_ssd->data, (long long)(min_ssd->step / 4), 0, emulate_cuda_edge}, plan, st);
}

int mi_stereobm_textureness(const mi_mat *img, mi_mat *disp, int winsz, float avg_texture_threshold, void *stream)
{
    MI_TRY(check_same(img, "input", disp, "disparity"));
    MI_TRY(sbm::sbm_fail(sbm::sbm_check_window(winsz, 0)));
    if (tuning().sbm_texfuse != 0)
        return sbm::textureness_fused((const unsigned char *)img->data, (long long)img->step, (unsigned char *)disp->data, (long long)disp->step,
                                      nullptr, 1, img->rows, img->cols, winsz, avg_texture_threshold, (hipStream_t)stream);
    int sld, sh, *S = nullptr;
    sbm::textureness_scratch_dims(img->rows, img->cols, &sld, &sh);
    DevTmp tmp;
    MI_TRY(tmp.alloc(&S, (size_t)sld * sh));
    MI_TRY(sbm::textureness((const unsigned char *)img->data, (long long)img->step, (unsigned char *)disp->data,
                            (long long)disp->step, img->rows, img->cols, winsz, avg_texture_threshold, S, (hipStream_t)stream));
    MI_HIP_TRY(hipStreamSynchronize((hipStream_t)stream));   // S is freed on return
    return MI_OK;
}

// one wave of a debug kernel: nin input words, nout output words behind them
static int selftest(int (*launch)(const unsigned *, unsigned *, hipStream_t), const unsigned *in_host, size_t nin, unsigned *out_host, size_t nout)
{
    MI_REQUIRE(in_host && out_host, MI_ERR_BAD_ARG, "null argument");
    unsigned *d = nullptr;
    DevTmp tmp;
    MI_TRY(tmp.alloc(&d, nin + nout));
    MI_HIP_TRY(hipMemcpy(d, in_host, sizeof(unsigned) * nin, hipMemcpyHostToDevice));
    MI_TRY(launch(d, d + nin, nullptr));
    MI_HIP_TRY(hipDeviceSynchronize());
    MI_HIP_TRY(hipMemcpy(out_host, d + nin, sizeof(unsigned) * nout, hipMemcpyDeviceToHost));
    return MI_OK;
}
int miflow_selftest_tmax16(const unsigned *in_host, unsigned *out_host) { return selftest(sbm::dbg_tmax16, in_host, 1024, out_host, 64); }
int miflow_selftest_wave_min(const unsigned *in_host, unsigned *out_host) { return selftest(sbm::dbg_wave_min, in_host, 64, out_host, 65); }

}  // extern "C"
