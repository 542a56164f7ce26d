/* tools/sgm_ref/cu/cuda.h -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.
 * <cuda.h> while the reference's modules/cudastereo/src/cuda/stereosgm.cu is compiled for the host: the toolkit version its shuffle
 * wrappers ask for (>= 9000: the *_sync forms of oracle/refshim/cudashim/cudashim.h) and the device intrinsics the file calls that the
 * shim lacks.  Their definitions are those of the CUDA Math API / C++ Programming Guide; none of them is reference arithmetic. */
#ifndef SGM_REF_CUDA_H
#define SGM_REF_CUDA_H
#include <cstdint>
#define CUDA_VERSION 12000

static inline int __popc(unsigned x) { return __builtin_popcount(x); }
template <typename T> static inline T __ldg(const T *p) { return *p; }   // a load through the read-only cache

/* per-halfword / per-byte unsigned SIMD-in-a-word: compare greater-than (all ones where a > b), minimum, maximum */
namespace sgm_ref_simd {
template <int BITS, typename F> inline uint32_t lanes(uint32_t a, uint32_t b, F f)
{
    const uint32_t m = BITS == 16 ? 0xffffu : 0xffu;
    uint32_t r = 0;
    for (int s = 0; s < 32; s += BITS) r |= (f((a >> s) & m, (b >> s) & m) & m) << s;
    return r;
}
inline uint32_t gt(uint32_t a, uint32_t b) { return a > b ? 0xffffffffu : 0u; }
inline uint32_t mn(uint32_t a, uint32_t b) { return a < b ? a : b; }
inline uint32_t mx(uint32_t a, uint32_t b) { return a > b ? a : b; }
}
static inline uint32_t __vcmpgtu2(uint32_t a, uint32_t b) { return sgm_ref_simd::lanes<16>(a, b, sgm_ref_simd::gt); }
static inline uint32_t __vcmpgtu4(uint32_t a, uint32_t b) { return sgm_ref_simd::lanes<8>(a, b, sgm_ref_simd::gt); }
static inline uint32_t __vminu2(uint32_t a, uint32_t b) { return sgm_ref_simd::lanes<16>(a, b, sgm_ref_simd::mn); }
static inline uint32_t __vminu4(uint32_t a, uint32_t b) { return sgm_ref_simd::lanes<8>(a, b, sgm_ref_simd::mn); }
static inline uint32_t __vmaxu2(uint32_t a, uint32_t b) { return sgm_ref_simd::lanes<16>(a, b, sgm_ref_simd::mx); }
static inline uint32_t __vmaxu4(uint32_t a, uint32_t b) { return sgm_ref_simd::lanes<8>(a, b, sgm_ref_simd::mx); }
#endif
