// Owners of everything a handle holds besides its scratch buffers (mi_buf.h): one opaque handle (a stream, an event), the process-wide
// cache of large device blocks, and a TV-L1 lane's block out of that cache.  No HIP in here: what creates and destroys a handle is a
// policy, what the cache does to the device a backend (mi_common.h has the HIP ones), so tests/cpp/own_test.cpp runs the same code on
// the host against a fake that counts, fails on request and knows every live object.
#pragma once
#include <cstddef>
#include <mutex>
#include <utility>
#include <vector>
#include "mi_buf.h"

namespace mi {

// One handle, created on demand, destroyed with its owner; move-only.  Policy supplies
//   using handle = ...;                  a pointer type
//   static int create(handle *h)         MI_OK or the error code (and the error text)
//   static void destroy(handle h)        errors ignored
template <class Policy>
class Owned {
public:
    using handle = typename Policy::handle;
    Owned() = default;
    explicit Owned(handle h) : h_(h) {}   // adopts h
    Owned(Owned &&o) noexcept : h_(o.release()) {}
    Owned &operator=(Owned &&o) noexcept { if (this != &o) { reset(); h_ = o.release(); } return *this; }
    Owned(const Owned &) = delete;
    Owned &operator=(const Owned &) = delete;
    ~Owned() { reset(); }
    // the handle exists afterwards; on failure the owner stays empty and the policy's code comes back
    int ensure()
    {
        if (h_) return MI_OK;
        handle q = nullptr;
        if (const int rc = Policy::create(&q)) return rc;
        h_ = q;
        return MI_OK;
    }
    handle get() const { return h_; }
    handle release() { handle q = h_; h_ = nullptr; return q; }   // gives the handle up: the caller owns it now
    void reset() { if (h_) Policy::destroy(h_); h_ = nullptr; }
private:
    handle h_ = nullptr;
};

// Events of a cache backend B as an Owned policy
template <class B>
struct BackendEvent {
    using handle = void *;
    static int create(handle *e) { return B::event_create(e); }
    static void destroy(handle e) { B::event_destroy(e); }
};

// The cache of large device blocks (the per-lane TV-L1 arenas; why it exists: mi_common.h).  A block given back is kept -- with the
// event its previous owner recorded behind its last work, which the next taker waits for -- and handed to the next request of a
// similar size on the same device.  B supplies, each returning 0 or the device runtime's error number:
//   dev_malloc(void **, size_t)  dev_free(void *)  get_device(int *)  pointer_device(const void *, int *)  set_device(int)
//   device_sync()  event_sync(void *)  event_create(void **)  event_record(void *event, void *stream)
//   stream_capturing(void *stream, bool *)
// and  void event_destroy(void *),  void clear_error()  (the thread's sticky error),  const char *error_string(int).
template <class B>
class ArenaCache {
public:
    using Event = Owned<BackendEvent<B>>;
    // at most max_blocks blocks and dev_bytes bytes per device, total_bytes bytes over all devices (0 bytes: nothing is kept)
    ArenaCache(size_t max_blocks, size_t dev_bytes, size_t total_bytes) : max_blocks_(max_blocks), dev_bytes_(dev_bytes), total_bytes_(total_bytes) {}
    ArenaCache(const ArenaCache &) = delete;
    ArenaCache &operator=(const ArenaCache &) = delete;
    ~ArenaCache() { trim(); }

    // a block of at least `bytes` on the current device: the smallest cached one of bytes <= cap <= bytes + bytes / 2 + 64 MB, else a new one
    int alloc(void **p, size_t bytes, size_t *capacity)
    {
        *p = nullptr;
        int dev = 0;
        if (const int e = B::get_device(&dev)) { set_error("no current device: %s", B::error_string(e)); return MI_ERR_HIP; }
        Block hit;
        {
            std::lock_guard<std::mutex> lk(mu_);
            int best = -1;
            for (size_t i = 0; i < blocks_.size(); ++i)
                if (blocks_[i].dev == dev && blocks_[i].cap >= bytes && blocks_[i].cap <= bytes + bytes / 2 + ((size_t)64 << 20) &&
                    (best < 0 || blocks_[i].cap < blocks_[best].cap))
                    best = (int)i;
            if (best >= 0) {
                hit = std::move(blocks_[best]);
                blocks_.erase(blocks_.begin() + best);
            }
        }
        // nothing the block's previous owner enqueued may still touch it: wait for ITS last work only (the event that came with the
        // block) -- no device-wide synchronisation, other handles' streams keep running
        if (hit.p && hit.ready.get()) {
            const int we = B::event_sync(hit.ready.get());
            hit.ready.reset();
            if (we) {
                // The event could not be waited for.  Seen on ROCm 7.2 when the stream it was recorded on has since been destroyed
                // (hipErrorCapturedEvent: the runtime looks at the dead stream).  Clear the thread's sticky error -- it would surface
                // at the next look after an unrelated launch -- and fall back to what vouches for the block without the event: the
                // whole device idle.  If even that fails the block is dropped for a fresh one.
                B::clear_error();
                if (B::device_sync()) { B::clear_error(); (void)B::dev_free(hit.p); hit.p = nullptr; }
            }
        }
        if (hit.p) { *p = hit.p; *capacity = hit.cap; return MI_OK; }
        int e = B::dev_malloc(p, bytes);
        if (e) {   // make room and retry once
            trim();
            e = B::dev_malloc(p, bytes);
        }
        if (e) { *p = nullptr; set_error("device allocation of %zu bytes failed: %s", bytes, B::error_string(e)); return MI_ERR_OOM; }
        *capacity = bytes;
        return MI_OK;
    }

    // `ready`: an event the owner recorded behind its last work on the block WHILE ITS STREAM WAS ALIVE (it passes to the cache; the next
    // taker waits for it and destroys it).  No event and `busy`: the owner cannot vouch for the block (e.g. its last calc was enqueued
    // under stream capture) -- the block's device is synchronised instead.  Nothing here touches a caller's stream: at destroy time it
    // may no longer exist.  A block the cache does not keep (not idle, or a bound would be passed) goes back to the driver.
    void free(void *p, size_t capacity, Event ready, bool busy)
    {
        if (!p) return;   // (an event that came along dies with `ready`)
        int dev = 0;
        if (B::get_device(&dev) == 0) {
            const int cur = dev;
            if (B::pointer_device(p, &dev) != 0) dev = cur;
            if (dev != cur) (void)B::set_device(dev);
            bool idle = true;
            if (!ready.get() && busy) idle = B::device_sync() == 0;
            if (dev != cur) (void)B::set_device(cur);
            std::lock_guard<std::mutex> lk(mu_);
            size_t total = capacity, all = capacity, blocks = 0;
            for (const Block &b : blocks_) {
                all += b.cap;
                if (b.dev == dev) { total += b.cap; ++blocks; }
            }
            if (idle && blocks < max_blocks_ && total <= dev_bytes_ && all <= total_bytes_) {
                blocks_.push_back(Block{p, capacity, dev, std::move(ready)});
                return;
            }
            if (ready.get()) (void)B::event_sync(ready.get());
        }
        ready.reset();   // the cache does not take the block: its event goes with it
        if (const int fe = B::dev_free(p)) set_error("freeing a %zu-byte arena failed: %s", capacity, B::error_string(fe));
    }

    // everything back to the driver; the current device stays
    void trim()
    {
        std::vector<Block> all;
        {
            std::lock_guard<std::mutex> lk(mu_);
            all.swap(blocks_);
        }
        int cur = 0;
        const bool have = B::get_device(&cur) == 0;
        for (Block &b : all) {
            if (b.ready.get()) { (void)B::event_sync(b.ready.get()); b.ready.reset(); }
            (void)B::dev_free(b.p);   // (pointers of any device)
        }
        if (have) (void)B::set_device(cur);
    }

    size_t cached_blocks() { std::lock_guard<std::mutex> lk(mu_); return blocks_.size(); }

private:
    struct Block { void *p = nullptr; size_t cap = 0; int dev = 0; Event ready; };   // ready: the previous owner's last work on the block (may be empty)
    const size_t max_blocks_, dev_bytes_, total_bytes_;
    std::mutex mu_;
    std::vector<Block> blocks_;
};

// A TV-L1 lane's block out of the cache, and what the cache needs to know when it comes back: the event behind the lane's last calc.
template <class B>
class CachedArena {
public:
    explicit CachedArena(ArenaCache<B> *cache) : cache_(cache) {}
    CachedArena(const CachedArena &) = delete;
    CachedArena &operator=(const CachedArena &) = delete;
    ~CachedArena() { release(); }
    void *get() const { return p_; }
    size_t capacity() const { return cap_; }
    bool used() const { return used_; }               // a calc has been enqueued on the block
    bool idle_valid() const { return idle_valid_; }   // the idle event stands behind the last of them
    bool holds_event() const { return idle_.get() != nullptr; }
    // another block of at least `bytes` (the one held goes back first); empty on failure
    int acquire(size_t bytes)
    {
        release();
        return cache_->alloc(&p_, bytes, &cap_);
    }
    // Behind everything a call enqueued for the block on `stream` (also on an error return: part of it may be in flight).  No event under
    // stream capture, or when the event cannot be created or recorded: the block then counts as busy with nobody to vouch for it.
    void mark(void *stream)
    {
        if (!p_) return;
        used_ = true; idle_valid_ = false;
        bool capturing = false;
        if (B::stream_capturing(stream, &capturing) || capturing) { B::clear_error(); return; }
        if (idle_.ensure()) { B::clear_error(); return; }
        if (B::event_record(idle_.get(), stream) == 0) idle_valid_ = true; else B::clear_error();
    }
    // The block goes back to the cache with the idle event, where that is valid: whoever takes the block next waits for that event
    // only -- destroying one handle does not stall the other handles' streams.  An event that is not valid stays here for the next block.
    void release()
    {
        if (p_) cache_->free(p_, cap_, idle_valid_ ? std::move(idle_) : typename ArenaCache<B>::Event(), used_);
        idle_valid_ = used_ = false;
        p_ = nullptr; cap_ = 0;
    }
    // release(), and the idle event goes too where the cache did not take it: as constructed
    void reset() { release(); idle_.reset(); }
private:
    ArenaCache<B> *cache_;
    void *p_ = nullptr;
    size_t cap_ = 0;
    typename ArenaCache<B>::Event idle_;   // recorded behind the lane's last calc on the stream it ran on
    bool idle_valid_ = false, used_ = false;
};

}  // namespace mi
