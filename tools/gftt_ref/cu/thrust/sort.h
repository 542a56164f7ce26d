/* tools/gftt_ref/cu: stand-in for <thrust/sort.h>: sort(policy, first, last, cmp) as std::stable_sort.  thrust's comparison sort is
 * not stable, so the order among elements that compare equal is open in the reference; the strict fixtures are recorded where no two
 * candidates have equal responses, and the `ties` fixture is compared as a set.  TEST INFRASTRUCTURE. */
#ifndef GFTT_REF_THRUST_SORT_H
#define GFTT_REF_THRUST_SORT_H
#include <algorithm>
#include <thrust/device_ptr.h>
#include <thrust/execution_policy.h>
namespace thrust {
template <typename T, class Cmp> inline void sort(device_ptr<T> first, device_ptr<T> last, Cmp cmp) { std::stable_sort(first.p, last.p, cmp); }
template <class Policy, typename T, class Cmp> inline void sort(const Policy &, device_ptr<T> first, device_ptr<T> last, Cmp cmp)
{
    std::stable_sort(first.p, last.p, cmp);
}
}
#endif
