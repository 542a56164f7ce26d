// Internal launch API of the StereoBeliefPropagation HIP kernels (stereobp_kernels.hip).  Not part of the C-ABI.
// Every plane set (data cost, one message) is planar as in the reference: disparity k of pixel (y, x) of a rows x cols level at
// element (k * rows + y) * step + x; steps in ELEMENTS of T (short for CV_16S, float for CV_32F messages).
#pragma once
#include "mi_common.h"
#include "sbp_plan.h"

namespace mi {
namespace sbp {

// the reference's __constant__ state (stereobp.cu:57-61) as kernel arguments: two handles on two streams do not share it
struct BpConst { int ndisp; float max_data_term, data_weight, max_disc_term, disc_single_jump; };
inline int sbp_fail(const SbpErr &e) { MI_REQUIRE(e.code == MI_OK, e.code, "%s", e.msg); return MI_OK; }

// comp_data<cn, T>, stereobp.cu:132-161: interior pixels only
int comp_data(int msg_type, int cn, const unsigned char *left, long long lstep, const unsigned char *right, long long rstep,
              void *data, long long dstep, int rows, int cols, const BpConst &c, hipStream_t s);
// data_step_down<T>, stereobp.cu:257-280
int data_step_down(int msg_type, const void *src, long long sstep, int src_rows, int src_cols, void *dst, long long dstep,
                   int dst_rows, int dst_cols, int ndisp, hipStream_t s);
// level_up_message<T> x 4, stereobp.cu:305-349: msgs u, d, l, r in one launch
struct BpMsgs { void *u, *d, *l, *r; long long step; };
int level_up(int msg_type, const BpMsgs &src, int src_rows, const BpMsgs &dst, int dst_rows, int dst_cols, int ndisp, hipStream_t s);
// one_iteration<T>, stereobp.cu:429-450, in the plan's form (cap: the register form's capacity)
int iterate(int msg_type, int form, int cap, const BpMsgs &m, const void *data, long long dstep, int rows, int cols, int t,
            const BpConst &c, hipStream_t s);
// output<T>, stereobp.cu:481-517, + out.setTo(0) and convertTo of calcBP (stereobp.cpp:342-358): disp of out_type MI_16SC1 / MI_8UC1 /
// MI_32SC1 / MI_32FC1, dstep in BYTES
int output(int msg_type, const BpMsgs &m, const void *data, long long dstep, int rows, int cols, int ndisp, void *disp, long long ostep,
           int out_type, hipStream_t s);

}  // namespace sbp
}  // namespace mi
