/* tools/gftt_ref/cu: stand-in for <thrust/execution_policy.h>: thrust::cuda::par(allocator) and its .on(stream), which say where the
 * sort runs and where its temporary storage comes from.  On the host both say nothing.  TEST INFRASTRUCTURE. */
#ifndef GFTT_REF_THRUST_EXECUTION_POLICY_H
#define GFTT_REF_THRUST_EXECUTION_POLICY_H
namespace thrust { namespace cuda {
struct host_policy {
    template <class Stream> host_policy on(Stream) const { return *this; }
};
struct par_t {
    template <class Allocator> host_policy operator()(Allocator &) const { return host_policy(); }
};
static const par_t par = par_t();
}}
#endif
