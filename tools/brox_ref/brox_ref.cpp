/* tools/brox_ref/brox_ref.cpp -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.
 * C entry points over the reference's own code for cv::cuda::BroxOpticalFlow, compiled for the host by tools/make_golden_brox.py.  Every
 * file #included below with a name ending in .gen.cpp or .gen.inc is a build intermediate that cu2host.py writes from the reference
 * tree (never committed):
 *   brox_npp.gen.cpp   slices of cudalegacy/src/cuda/NPP_staging.cu: the mirror filters with their two host wrappers (:1433-1633) and
 *                      processLine .. nppiStResize_32f_C1R (:2073-2282), launches rewritten;
 *   brox_ncv.gen.cpp   cudalegacy/src/cuda/NCVBroxOpticalFlow.cu, whole, launches rewritten.  NCVBroxOpticalFlow() compiles whole
 *                      against tools/brox_ref/cu, so the class fixtures are what the reference's host function computed;
 *   brox_s_*.gen.inc   for the STAGE fixtures, slices of the same host function, launches rewritten: the supersample call (:763-764),
 *                      the prolongation with its scaling (:952-955), the seven filter calls (:842-868), the grids (:889-893), the
 *                      launches of the two prepare stages (:901-902, :906) and the solver loop (:912-924).
 * Written here and not by the reference: only the objects those slices name (planes with a ptr(), sizes, rectangles, strides) and the
 * closing brace of the solver loop, which the slice ends before. */
#include <vector>
#include "brox_ncv_standin.hpp"
#include "opencv2/cudev/ptr2d/texture.hpp"
#include "brox_npp.gen.cpp"
#include "brox_ncv.gen.cpp"

static std::vector<int> g_linear;   /* rows, cols of every linearly filtered texture made: NCVBroxOpticalFlow makes nine per level (:829-876) */
extern "C" void brox_ref_texture_made(int rows, int cols, int linear)
{
    if (!linear) return;
    g_linear.push_back(rows);
    g_linear.push_back(cols);
}

namespace {
struct Plane { float *p; float *ptr() { return p; } };   /* what the slices call FloatVector: something with a ptr() */
}

extern "C" {

/* strides in floats; the two resizes as NCVBroxOpticalFlow calls them */
int brox_ref_resize_down(float *src, int sw, int sh, int sstride, float *dst, int dw, int dh, int dstride, float scale_factor)
{
    Plane in = {src}, out = {dst}, *I0 = &in, *level_frame0 = &out;
    NcvSize32u srcSize(sw, sh), dstSize(dw, dh);
    NcvRect32u srcROI(0, 0, sw, sh), dstROI(0, 0, dw, dh);
    const Ncv32u prev_level_pitch = sstride * sizeof(float), level_width_aligned = dstride;
#include "brox_s_down.gen.inc"
    return NCV_SUCCESS;
}

int brox_ref_resize_up(float *src, int sw, int sh, int sstride, float *dst, int dw, int dh, int dstride, float scale_factor)
{
    Plane in = {src}, out = {dst}, *ptrU = &in, *ptrUNew = &out;
    NcvSize32u inner_srcSize(sw, sh), dstSize(dw, dh);
    NcvRect32u srcROI(0, 0, sw, sh), dstROI(0, 0, dw, dh);
    const Ncv32u kLevelStride = sstride, ns = dstride, nh = dh;
    cudaStream_t stream = 0;
    if (dstride != dw) return NCV_INCONSISTENT_INPUT;   /* ScaleVector runs over ns * nh floats */
#include "brox_s_up.gen.inc"
    return NCV_SUCCESS;
}

/* out: Ix0, Iy0, Ix, Iy, Ixx, Iyy, Ixy, each h x stride */
int brox_ref_derivatives(float *i0, float *i1, int w, int h, int stride, float **out)
{
    float taps[5] = {1.0f, -8.0f, 0.0f, 8.0f, -1.0f};   /* derivativeFilterHost, :689: data */
    const int kDFilterSize = 5;
    Plane derivativeFilter = {taps}, a = {i0}, b = {i1}, *I0 = &a, *I1 = &b;
    Plane Ix0 = {out[0]}, Iy0 = {out[1]}, Ix = {out[2]}, Iy = {out[3]}, Ixx = {out[4]}, Iyy = {out[5]}, Ixy = {out[6]};
    NcvSize32u srcSize(w, h);
    Ncv32u nSrcStep = stride * sizeof(float);
    NcvRect32u oROI(0, 0, w, h);
#include "brox_s_filters.gen.inc"
    return NCV_SUCCESS;
}

/* flows: u, v, du, dv; images: I0, I1, Ix, Ixx, Ix0, Iy, Iyy, Iy0, Ixy; coeffs: diffusivity_x, diffusivity_y, denominator_u,
 * denominator_v, numerator_dudv, numerator_u, numerator_v.  stage: 1 = prepare_sor_stage_1_tex, 2 = prepare_sor_stage_2 on the same planes */
int brox_ref_prepare(int stage, float **flows, float **images, float **coeffs, int w, int h, int stride, float alpha, float gamma)
{
    const Ncv32u kLevelWidth = w, kLevelHeight = h, kLevelStride = stride;
    const int kLevelSizeInBytes = stride * h * sizeof(float), kPitchTex = stride * sizeof(float);
    cudaStream_t stream = 0;
    Plane diffusivity_x = {coeffs[0]}, diffusivity_y = {coeffs[1]}, denom_u = {coeffs[2]}, denom_v = {coeffs[3]}, num_dudv = {coeffs[4]},
          num_u = {coeffs[5]}, num_v = {coeffs[6]};
    Texture texU(kLevelSizeInBytes, flows[0]), texV(kLevelSizeInBytes, flows[1]), texDu(kLevelSizeInBytes, flows[2]), texDv(kLevelSizeInBytes, flows[3]);
    Texture texDiffX(kLevelSizeInBytes, diffusivity_x.ptr()), texDiffY(kLevelSizeInBytes, diffusivity_y.ptr());
#define BROX_TEX(i) Texture(kLevelHeight, kLevelWidth, images[i], kPitchTex, true, cudaFilterModeLinear, cudaAddressModeMirror)
    Texture texI0 = BROX_TEX(0), texI1 = BROX_TEX(1), texIx = BROX_TEX(2), texIxx = BROX_TEX(3), texIx0 = BROX_TEX(4), texIy = BROX_TEX(5),
            texIyy = BROX_TEX(6), texIy0 = BROX_TEX(7), texIxy = BROX_TEX(8);
#undef BROX_TEX
#include "brox_s_grids.gen.inc"
    (void)sor_blocks; (void)sor_threads;
    if (stage == 1) {
#include "brox_s_stage1.gen.inc"
    } else {
#include "brox_s_stage2.gen.inc"
    }
    return NCV_SUCCESS;
}

/* flows: u, v, du, dv (du, dv updated), tmp: du_new, dv_new; coeffs after stage 2 */
int brox_ref_sor(float **flows, float **tmp, float **coeffs, int w, int h, int stride, int solver_iterations)
{
    const Ncv32u kLevelWidth = w, kLevelHeight = h, kLevelStride = stride;
    const int kLevelSizeInBytes = stride * h * sizeof(float);
    cudaStream_t stream = 0;
    NCVBroxOpticalFlowDescriptor desc = {};
    desc.number_of_solver_iterations = solver_iterations;
    Plane diffusivity_x = {coeffs[0]}, diffusivity_y = {coeffs[1]}, denom_u = {coeffs[2]}, denom_v = {coeffs[3]}, num_dudv = {coeffs[4]},
          num_u = {coeffs[5]}, num_v = {coeffs[6]}, du = {flows[2]}, dv = {flows[3]}, du_new = {tmp[0]}, dv_new = {tmp[1]};
    Texture texU(kLevelSizeInBytes, flows[0]), texV(kLevelSizeInBytes, flows[1]), texDu(kLevelSizeInBytes, du.ptr()), texDv(kLevelSizeInBytes, dv.ptr()),
            texDuNew(kLevelSizeInBytes, du_new.ptr()), texDvNew(kLevelSizeInBytes, dv_new.ptr());
    Texture texDiffX(kLevelSizeInBytes, diffusivity_x.ptr()), texDiffY(kLevelSizeInBytes, diffusivity_y.ptr());
#include "brox_s_grids.gen.inc"
    (void)psor_blocks; (void)psor_threads;
#include "brox_s_solver.gen.inc"
    }   /* the slice ends before the loop's closing brace */
    return NCV_SUCCESS;
}

/* NCVBroxOpticalFlow, whole.  levels: room for 2 * max_levels ints (rows, cols; coarsest first); returns the status, *n_levels the count */
int brox_ref_calc(float alpha, float gamma, float scale_factor, int inner, int outer, int solver, float *f0, float *f1, int w, int h, int pitch_bytes,
                  float *u, float *v, int out_pitch_bytes, int alignment, int *levels, int max_levels, int *n_levels)
{
    NCVBroxOpticalFlowDescriptor desc = {alpha, gamma, scale_factor, (Ncv32u)inner, (Ncv32u)outer, (Ncv32u)solver};
    INCVMemAllocator alloc(alignment);
    NCVMatrix<Ncv32f> m0(f0, w, h, pitch_bytes), m1(f1, w, h, pitch_bytes), mu(u, w, h, out_pitch_bytes), mv(v, w, h, out_pitch_bytes);
    g_linear.clear();
    const NCVStatus s = NCVBroxOpticalFlow(desc, alloc, m0, m1, mu, mv, 0);
    *n_levels = (int)(g_linear.size() / 18);
    for (int i = 0; i < *n_levels && i < max_levels; ++i) { levels[2 * i] = g_linear[18 * i]; levels[2 * i + 1] = g_linear[18 * i + 1]; }
    return s;
}

}  /* extern "C" */
