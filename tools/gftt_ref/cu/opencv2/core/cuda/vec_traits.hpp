/* tools/gftt_ref/cu: in front of oracle/refshim/cudavec on the include path while the reference's 8-bit row filter is compiled for the
 * host.  TEST INFRASTRUCTURE.  Adds the single-channel uchar case of VecTraits / TypeVec (main-repo vec_traits.hpp), which the shim
 * has for float only.  No arithmetic of the filters. */
#ifndef GFTT_REF_VEC_TRAITS_HPP
#define GFTT_REF_VEC_TRAITS_HPP
#include_next "opencv2/core/cuda/vec_traits.hpp"
namespace cv { namespace cuda { namespace device {
template <> struct VecTraits<unsigned char> {
    typedef unsigned char elem_type; enum { cn = 1 };
    static unsigned char all(unsigned char v) { return v; }
    static unsigned char make(unsigned char x) { return x; }
    static unsigned char make(const unsigned char *v) { return *v; }
};
template <> struct TypeVec<unsigned char, 1> { typedef unsigned char vec_type; };
}}}
#endif
