/* tools/gftt_ref/cu: stand-in for <thrust/version.h> while the reference's cudaimgproc/src/cuda/gftt.cu is compiled for the host.
 * TEST INFRASTRUCTURE.  At 100802 and above gftt.cu takes the call with an execution policy and the allocator (gftt.cu:128-132). */
#ifndef GFTT_REF_THRUST_VERSION_H
#define GFTT_REF_THRUST_VERSION_H
#define THRUST_VERSION 100802
#endif
