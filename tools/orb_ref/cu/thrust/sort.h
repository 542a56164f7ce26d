/* tools/orb_ref/cu: stand-in for <thrust/sort.h>: sort_by_key as a std::stable_sort of a permutation (thrust's radix path for float keys is
 * stable too; the fixtures are recorded where no tie straddles a cut, so stability decides nothing in them).  TEST INFRASTRUCTURE. */
#ifndef ORB_REF_THRUST_SORT_H
#define ORB_REF_THRUST_SORT_H
#include <algorithm>
#include <numeric>
#include <vector>
#include <thrust/device_ptr.h>
namespace thrust {
template <typename T> struct greater { bool operator()(const T &a, const T &b) const { return a > b; } };
template <typename K, typename V, class Cmp> inline void sort_by_key(device_ptr<K> first, device_ptr<K> last, device_ptr<V> values, Cmp cmp)
{
    const size_t n = (size_t)(last - first);
    std::vector<size_t> order(n);
    std::iota(order.begin(), order.end(), (size_t)0);
    std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return cmp(first.p[a], first.p[b]); });
    std::vector<K> k(n);
    std::vector<V> v(n);
    for (size_t i = 0; i < n; ++i) { k[i] = first.p[order[i]]; v[i] = values.p[order[i]]; }
    for (size_t i = 0; i < n; ++i) { first.p[i] = k[i]; values.p[i] = v[i]; }
}
}
#endif
