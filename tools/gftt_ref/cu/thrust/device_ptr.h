/* tools/gftt_ref/cu: stand-in for <thrust/device_ptr.h>: on the host a device pointer is a pointer.  TEST INFRASTRUCTURE. */
#ifndef GFTT_REF_THRUST_DEVICE_PTR_H
#define GFTT_REF_THRUST_DEVICE_PTR_H
#include <cstddef>
#include <thrust/version.h>
namespace thrust {
template <typename T> struct device_ptr {
    T *p;
    explicit device_ptr(T *q) : p(q) {}
    device_ptr operator+(ptrdiff_t n) const { return device_ptr(p + n); }
    ptrdiff_t operator-(const device_ptr &o) const { return p - o.p; }
};
}
#endif
