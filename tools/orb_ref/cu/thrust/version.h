/* tools/orb_ref/cu: stand-in for <thrust/version.h> while the reference's cudafeatures2d/src/cuda/orb.cu is compiled for the host.
 * TEST INFRASTRUCTURE.  Below 100800 orb.cu takes its plain sort_by_key call (orb.cu:86), with no allocator and no execution policy. */
#ifndef ORB_REF_THRUST_VERSION_H
#define ORB_REF_THRUST_VERSION_H
#define THRUST_VERSION 100700
#endif
