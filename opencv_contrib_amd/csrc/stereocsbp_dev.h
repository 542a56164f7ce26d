// Internal launch API of the StereoConstantSpaceBP HIP kernels (stereocsbp_kernels.hip).  Not part of the C-ABI.
// Every plane set (costs, candidates, one message) is planar as in the reference: plane k of pixel (y, x) of a rows x cols level at
// element (k * rows + y) * step + x; steps in ELEMENTS of T (short for CV_16S, float for CV_32F messages).  Image steps in bytes.
#pragma once
#include "mi_common.h"
#include "scsbp_plan.h"

namespace mi {
namespace scsbp {

inline int csbp_fail(const CsbpErr &e) { MI_REQUIRE(e.code == MI_OK, e.code, "%s", e.msg); return MI_OK; }

struct CsbpImages { const unsigned char *left, *right; long long lstep, rstep; int rows, cols, cn; };
// what the reference passes by value at every launch; max_disc_term is the int the host truncates the float to (stereocsbp.cu:720)
struct CsbpConst { float max_data_term, data_weight; int min_disp; int max_disc_term; float disc_single_jump; };
// u, d, l, r and the selected disparities of one level, one step
struct CsbpSet { void *u, *d, *l, *r, *disp; long long step; };

// init_data_cost / compute_data_cost + their reduce forms, stereocsbp.cu:178-267, :356-447.  sel == null: candidate k is disparity k
// (n = ndisp); else candidate k of pixel (y, x) is sel[(k * h2 + y / 2) * sel_step + x / 2] (n = the parent's planes).
int data_cost(int msg_type, const CsbpImages &im, const void *sel, long long sel_step, int h2, void *out, long long ostep, int h, int w,
              int level, int n, const CsbpConst &c, hipStream_t s);
// get_first_k_initial_local / _global, stereocsbp.cu:86-176.  Up to CSBP_FIRST_K_WAVE_MAX disparities a wave selects for one pixel from
// a copy of its costs in LDS (2 x ndisp x sizeof(T) <= 32 KiB); beyond, a lane selects for one pixel in global memory as the reference
// does, and cost (ndisp planes) is consumed.
constexpr int CSBP_FIRST_K_WAVE_MAX = 4096;
int first_k(int msg_type, int local, void *cost, void *sel_cost, void *sel_disp, long long step, int h, int w, int nr_plane, int ndisp,
            hipStream_t s);
// init_message, stereocsbp.cu:525-607: data_cost, sel_cost, temp and the new set share the new set's step
int init_message(int msg_type, void *temp, const CsbpSet &nw, const CsbpSet &cur, void *sel_cost, const void *data_cost, int h, int w,
                 int nr_plane, int h2, int w2, int nr_plane2, hipStream_t s);
// compute_message, stereocsbp.cu:656-716, half-sweep t, in the given form; temp is touched by the general form only
int iterate(int msg_type, int form, int cap, const CsbpSet &m, const void *sel_cost, void *temp, int h, int w, int nr_plane, int t,
            const CsbpConst &c, hipStream_t s);
// compute_disp, stereocsbp.cu:752-804, + out.setTo(0) and convertTo (stereocsbp.cpp:303-328); ostep in BYTES
int compute_disp(int msg_type, const CsbpSet &m, const void *sel_cost, int rows, int cols, int nr_plane, void *disp, long long ostep,
                 int out_type, hipStream_t s);

}  // namespace scsbp
}  // namespace mi
