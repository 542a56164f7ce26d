// The one owner of a handle's scratch memory.  No HIP in here: the allocator is a policy (mi_common.h has the device and the
// pinned-host one), so tests/cpp/grow_buf_test.cpp runs the same code on the host with an allocator that counts and fails.
// Its sibling mi_own.h owns what is not a buffer: streams, events and the cached TV-L1 arenas.  Together they make every
// mi_*_destroy a `delete h`.
#pragma once
#include <cstddef>
#include "miflow/c_api.h"

namespace mi {

void set_error(const char *fmt, ...);

// n elements of T: grown on demand, never shrunk, freed with its owner.  Alloc supplies
//   static int alloc(void **p, size_t bytes)   MI_OK or the error code (and the error text)
//   static void free(void *p)
// A growth RELEASES FIRST and allocates then: the peak footprint stays one block, and the device policy's free synchronises
// the device, which is what makes a re-grow safe against work of an earlier call still in flight on another stream.
template <class T, class Alloc>
struct GrowBuf {
    T *p = nullptr;
    size_t n = 0;   // elements held
    GrowBuf() = default;
    GrowBuf(const GrowBuf &) = delete;
    GrowBuf &operator=(const GrowBuf &) = delete;
    ~GrowBuf() { release(); }
    // at least `want` elements; on failure the buffer is empty and the allocator's code comes back
    int ensure(size_t want)
    {
        if (n >= want) return MI_OK;
        release();
        if (want > (size_t)-1 / sizeof(T)) {
            set_error("scratch buffer of %zu x %zu bytes exceeds the address space", want, sizeof(T));
            return MI_ERR_OOM;
        }
        void *q = nullptr;
        if (const int rc = Alloc::alloc(&q, sizeof(T) * want)) return rc;
        p = (T *)q; n = want;
        return MI_OK;
    }
    void release()
    {
        if (p) Alloc::free(p);
        p = nullptr; n = 0;
    }
};

}  // namespace mi
