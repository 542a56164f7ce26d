/* tools/orb_ref/cu: in front of oracle/refshim/cudashim on the include path while orb.cu is compiled for the host.  TEST INFRASTRUCTURE.
 * Adds the three-component tuple form of reduce that HarrisResponses uses (orb.cu:134-135), per component like the shim's two-component
 * one, and short2.  No arithmetic of ORB. */
#ifndef ORB_REF_REDUCE_HPP
#define ORB_REF_REDUCE_HPP
#include_next "opencv2/core/cuda/reduce.hpp"

struct short2 { short x, y; };

namespace cv { namespace cuda { namespace device {
template <typename P0, typename P1, typename P2> struct SmemTuple3 { P0 p0; P1 p1; P2 p2; };
template <typename T0, typename T1, typename T2> inline SmemTuple3<volatile T0 *, volatile T1 *, volatile T2 *> smem_tuple(T0 *a, T1 *b, T2 *c)
{
    SmemTuple3<volatile T0 *, volatile T1 *, volatile T2 *> r = {a, b, c};
    return r;
}
}}}
namespace thrust {
template <typename A, typename B, typename C> struct RefTriple { A &a; B &b; C &c; };
template <typename A, typename B, typename C> inline RefTriple<A, B, C> tie(A &a, B &b, C &c) { RefTriple<A, B, C> r = {a, b, c}; return r; }
template <typename A, typename B, typename C> struct ValTriple { A a; B b; C c; };
template <typename A, typename B, typename C> inline ValTriple<A, B, C> make_tuple(A a, B b, C c) { ValTriple<A, B, C> r = {a, b, c}; return r; }
}
namespace cv { namespace cuda { namespace device {
template <unsigned N, typename P0, typename P1, typename P2, typename R0, typename R1, typename R2, class Op0, class Op1, class Op2>
inline void reduce(const SmemTuple3<P0, P1, P2> &smem, const thrust::RefTriple<R0, R1, R2> &val, unsigned tid, const thrust::ValTriple<Op0, Op1, Op2> &op)
{
    reduce_shim::run<N, R0, Op0>(smem.p0, val.a, tid, op.a);
    reduce_shim::run<N, R1, Op1>(smem.p1, val.b, tid, op.b);
    reduce_shim::run<N, R2, Op2>(smem.p2, val.c, tid, op.c);
}
}}}
#endif
