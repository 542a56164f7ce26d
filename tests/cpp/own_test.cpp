// The owners of csrc/mi_own.h on the host: Owned over a policy that counts, ArenaCache and CachedArena over a fake device whose events
// and blocks are malloc'd tokens (a leak or a second destroy is a sanitizer error, and the fake's own live sets fail the plain build),
// whose calls are logged and can be made to fail by kind and number.  Plain C++, no device.  Run by tests/test_own.py, plain and under
// the address / undefined-behaviour sanitizers; -fsanitize=thread -pthread builds it too (two_threads is there for that).
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <set>
#include <string>
#include <thread>
#include <vector>
#include "mi_own.h"

namespace mi {
static thread_local char g_err[256];
void set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
}  // namespace mi

namespace {

int g_checks = 0;
#define CHECK(c) do { ++g_checks; if (!(c)) { printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); exit(1); } } while (0)

const int kFailCode = 77;   // what a failing fake call returns: the owners hand it on, they make up none of their own
const size_t MB = (size_t)1 << 20;

enum Kind { MALLOC, FREE, GET_DEVICE, PTR_DEVICE, SET_DEVICE, DEV_SYNC, EV_SYNC, EV_CREATE, EV_RECORD, EV_DESTROY, CAPTURING, CLEAR, NKINDS };

// The fake device.  Currency is per thread, like HIP's; everything else is shared and locked.
struct Fake {
    static std::mutex mu;
    static int calls[NKINDS], fail_at[NKINDS], fail_n[NKINDS];   // calls fail_at .. fail_at + fail_n - 1 of a kind fail (1-based; 0: none)
    static std::map<void *, int> blocks;                          // live block -> device
    static std::set<void *> events;                               // live events
    static std::set<void *> recorded, capturing;                  // events recorded at least once; streams under capture
    static std::vector<std::string> log;
    static bool logging;
    static thread_local int dev;

    static void reset()
    {
        for (int k = 0; k < NKINDS; ++k) calls[k] = fail_at[k] = fail_n[k] = 0;
        log.clear(); recorded.clear(); capturing.clear();
        logging = true;
        dev = 0;
    }
    static void fail(Kind k, int nth_from_now, int n = 1) { fail_at[k] = calls[k] + nth_from_now; fail_n[k] = n; }
    static bool clean() { return blocks.empty() && events.empty(); }
    // counts the call, logs it; true = this one fails
    static bool enter(Kind k, const std::string &what)
    {
        ++calls[k];
        if (logging) log.push_back(what);
        return fail_at[k] && calls[k] >= fail_at[k] && calls[k] < fail_at[k] + fail_n[k];
    }

    static int dev_malloc(void **p, size_t)
    {
        std::lock_guard<std::mutex> lk(mu);
        if (enter(MALLOC, "malloc")) return kFailCode;
        *p = malloc(1);
        blocks[*p] = dev;
        return 0;
    }
    static int dev_free(void *p)
    {
        std::lock_guard<std::mutex> lk(mu);
        const bool f = enter(FREE, "free");
        if (!blocks.erase(p)) { printf("FAIL: free of a block that is not live\n"); exit(1); }
        ::free(p);
        return f ? kFailCode : 0;   // (a failing free has freed: only its report differs)
    }
    static int get_device(int *d)
    {
        std::lock_guard<std::mutex> lk(mu);
        if (enter(GET_DEVICE, "get_device")) return kFailCode;
        *d = dev;
        return 0;
    }
    static int pointer_device(const void *p, int *d)
    {
        std::lock_guard<std::mutex> lk(mu);
        if (enter(PTR_DEVICE, "pointer_device")) return kFailCode;
        const auto it = blocks.find(const_cast<void *>(p));
        if (it == blocks.end()) { printf("FAIL: attributes of a block that is not live\n"); exit(1); }
        *d = it->second;
        return 0;
    }
    static int set_device(int d)
    {
        std::lock_guard<std::mutex> lk(mu);
        const bool f = enter(SET_DEVICE, "set_device:" + std::to_string(d));
        dev = d;
        return f ? kFailCode : 0;
    }
    static int device_sync()
    {
        std::lock_guard<std::mutex> lk(mu);
        return enter(DEV_SYNC, "device_sync@" + std::to_string(dev)) ? kFailCode : 0;
    }
    static void need_event(void *e, const char *what)
    {
        if (!events.count(e)) { printf("FAIL: %s of an event that is not live\n", what); exit(1); }
    }
    static int event_sync(void *e)
    {
        std::lock_guard<std::mutex> lk(mu);
        need_event(e, "wait");
        return enter(EV_SYNC, "event_sync") ? kFailCode : 0;
    }
    static int event_create(void **e)
    {
        std::lock_guard<std::mutex> lk(mu);
        if (enter(EV_CREATE, "event_create")) return kFailCode;
        *e = malloc(1);
        events.insert(*e);
        return 0;
    }
    static void event_destroy(void *e)
    {
        std::lock_guard<std::mutex> lk(mu);
        (void)enter(EV_DESTROY, "event_destroy");
        need_event(e, "destroy");
        events.erase(e);
        recorded.erase(e);
        ::free(e);
    }
    static int event_record(void *e, void *)
    {
        std::lock_guard<std::mutex> lk(mu);
        need_event(e, "record");
        if (enter(EV_RECORD, "event_record")) return kFailCode;
        recorded.insert(e);
        return 0;
    }
    static int stream_capturing(void *s, bool *c)
    {
        std::lock_guard<std::mutex> lk(mu);
        if (enter(CAPTURING, "capturing")) return kFailCode;
        *c = capturing.count(s) != 0;
        return 0;
    }
    static void clear_error() { std::lock_guard<std::mutex> lk(mu); (void)enter(CLEAR, "clear"); }
    static const char *error_string(int e) { return e == kFailCode ? "injected failure" : "?"; }
};
std::mutex Fake::mu;
int Fake::calls[NKINDS], Fake::fail_at[NKINDS], Fake::fail_n[NKINDS];
std::map<void *, int> Fake::blocks;
std::set<void *> Fake::events, Fake::recorded, Fake::capturing;
std::vector<std::string> Fake::log;
bool Fake::logging = true;
thread_local int Fake::dev = 0;

using Cache = mi::ArenaCache<Fake>;
using Event = Cache::Event;
using Arena = mi::CachedArena<Fake>;

std::string joined(size_t from = 0)
{
    std::string s;
    for (size_t i = from; i < Fake::log.size(); ++i) s += (i > from ? " " : "") + Fake::log[i];
    return s;
}
Event new_event()
{
    Event e;
    CHECK(e.ensure() == MI_OK && e.get());
    return e;
}
// a block of `bytes` put into the cache from device `dev` (idle, optionally with an event); returns its pointer
void *seed(Cache &c, size_t bytes, int dev = 0, bool with_event = false)
{
    const int before = Fake::dev;
    Fake::dev = dev;
    void *p = nullptr;
    size_t cap = 0;
    const size_t n = c.cached_blocks();
    CHECK(c.alloc(&p, bytes, &cap) == MI_OK && p && cap == bytes);
    c.free(p, cap, with_event ? new_event() : Event(), false);
    CHECK(c.cached_blocks() == n + 1);   // (callers seed in an order that cannot hit)
    Fake::dev = before;
    return p;
}

// ---------------------------------------------------------------- Owned
struct Tok {
    using handle = int *;
    static int created, destroyed, fail_next;
    static std::set<int *> live;
    static int create(handle *h)
    {
        if (fail_next) { --fail_next; mi::set_error("token policy: create fails"); return kFailCode; }
        *h = (int *)malloc(sizeof(int));
        live.insert(*h);
        ++created;
        return MI_OK;
    }
    static void destroy(handle h)
    {
        if (!live.erase(h)) { printf("FAIL: destroy of a token that is not live\n"); exit(1); }
        ::free(h);
        ++destroyed;
    }
};
int Tok::created, Tok::destroyed, Tok::fail_next;
std::set<int *> Tok::live;
using Owner = mi::Owned<Tok>;

void owned_handle()
{
    {
        Owner o;
        CHECK(o.get() == nullptr && Tok::created == 0);            // lazy: nothing before the first ensure
        CHECK(o.ensure() == MI_OK && o.get());
        int *const first = o.get();
        CHECK(o.ensure() == MI_OK && o.get() == first && Tok::created == 1);   // ... and once
    }
    CHECK(Tok::created == 1 && Tok::destroyed == 1 && Tok::live.empty());
    {
        Owner o;
        Tok::fail_next = 1;
        CHECK(o.ensure() == kFailCode && o.get() == nullptr);     // the policy's code; empty
        CHECK(o.ensure() == MI_OK && o.get());                    // usable
        o.reset();
        CHECK(o.get() == nullptr && Tok::destroyed == 2);
        o.reset();
        CHECK(Tok::destroyed == 2);
    }
    CHECK(Tok::destroyed == 2);
    int *raw = nullptr;
    {
        Owner o;
        CHECK(o.ensure() == MI_OK);
        raw = o.release();
        CHECK(raw && o.get() == nullptr);
    }
    CHECK(Tok::destroyed == 2 && Tok::live.count(raw));           // given up: the destructor destroyed nothing
    {
        Owner adopted(raw);
        Owner moved(std::move(adopted));
        CHECK(adopted.get() == nullptr && moved.get() == raw);    // move leaves the source empty
        Owner other;
        CHECK(other.ensure() == MI_OK);
        other = std::move(moved);                                  // ... and the target's old handle is destroyed
        CHECK(moved.get() == nullptr && other.get() == raw && Tok::destroyed == 3);
    }
    CHECK(Tok::destroyed == 4 && Tok::live.empty());
    const int before = Tok::created;
    {
        std::vector<Owner> pool;                                   // a pool of profiling events: grows, i.e. moves its owners
        for (int i = 0; i < 9; ++i) { pool.emplace_back(); CHECK(pool.back().ensure() == MI_OK); }
        CHECK(Tok::live.size() == 9 && Tok::destroyed == 4);
    }
    CHECK(Tok::created == before + 9 && Tok::destroyed == 4 + 9 && Tok::live.empty());   // each exactly once
}

// ---------------------------------------------------------------- ArenaCache
void hit_window()
{
    Fake::reset();
    const size_t C = 200 * MB;
    // the smallest request a block of C still serves: bytes + bytes / 2 + 64 MB >= C
    const size_t lo = 95070891;
    static_assert(95070891 + 95070891 / 2 + 64 * ((size_t)1 << 20) == 200 * ((size_t)1 << 20), "lower end of the window");
    static_assert(95070890 + 95070890 / 2 + 64 * ((size_t)1 << 20) < 200 * ((size_t)1 << 20), "one below it");
    for (const size_t bytes : {C, C + 1, lo, lo - 1}) {
        Cache c(4, 4096 * MB, 4096 * MB);
        void *const blk = seed(c, C);
        const bool want_hit = bytes == C || bytes == lo;
        const int mallocs = Fake::calls[MALLOC];
        void *p = nullptr;
        size_t cap = 0;
        CHECK(c.alloc(&p, bytes, &cap) == MI_OK && p);
        CHECK((p == blk) == want_hit && cap == (want_hit ? C : bytes));
        CHECK(Fake::calls[MALLOC] == mallocs + (want_hit ? 0 : 1));            // a miss allocates, a hit does not
        CHECK(c.cached_blocks() == (want_hit ? 0u : 1u));
        c.free(p, cap, Event(), false);
    }
    CHECK(Fake::clean());
}

void smallest_fitting_and_devices()
{
    Fake::reset();
    {
        Cache c(4, 4096 * MB, 4096 * MB);
        void *const b200 = seed(c, 200 * MB);
        void *const b250 = seed(c, 250 * MB);
        seed(c, 300 * MB);
        void *p = nullptr, *q = nullptr;
        size_t cap = 0, capq = 0;
        CHECK(c.alloc(&p, 190 * MB, &cap) == MI_OK && p == b200 && cap == 200 * MB);   // all three fit: the smallest
        CHECK(c.alloc(&q, 190 * MB, &capq) == MI_OK && q == b250 && capq == 250 * MB);
        c.free(p, cap, Event(), false);
        c.free(q, capq, Event(), false);
    }
    CHECK(Fake::clean());
    {
        Cache c(4, 4096 * MB, 4096 * MB);
        void *const other = seed(c, 200 * MB, 1);
        void *p = nullptr, *q = nullptr;
        size_t cap = 0, capq = 0;
        CHECK(c.alloc(&p, 200 * MB, &cap) == MI_OK && p != other && Fake::blocks[p] == 0);   // device 0 never gets device 1's block
        CHECK(c.cached_blocks() == 1);
        Fake::dev = 1;
        CHECK(c.alloc(&q, 200 * MB, &capq) == MI_OK && q == other);
        Fake::dev = 0;
        c.free(q, capq, Event(), false);                            // given back from ANOTHER current device: filed under its own
        Fake::dev = 1;
        CHECK(c.alloc(&q, 200 * MB, &capq) == MI_OK && q == other);
        Fake::dev = 0;
        c.free(p, cap, Event(), false);
        c.free(q, capq, Event(), false);
    }
    CHECK(Fake::clean());
}

void alloc_failures()
{
    Fake::reset();
    Cache c(4, 4096 * MB, 4096 * MB);
    seed(c, 100 * MB, 0, true);
    seed(c, 400 * MB, 1, true);
    void *p = nullptr;
    size_t cap = 0;
    Fake::fail(MALLOC, 1);
    const int mallocs = Fake::calls[MALLOC];
    CHECK(c.alloc(&p, 1000 * MB, &cap) == MI_OK && p && cap == 1000 * MB);      // trimmed, retried
    CHECK(Fake::calls[MALLOC] == mallocs + 2 && c.cached_blocks() == 0 && Fake::blocks.size() == 1 && Fake::events.empty());
    c.free(p, cap, Event(), false);
    seed(c, 100 * MB);
    Fake::fail(MALLOC, 1, 2);
    mi::g_err[0] = 0;
    p = (void *)&cap;
    CHECK(c.alloc(&p, 5000 * MB, &cap) == MI_ERR_OOM && p == nullptr && mi::g_err[0] != 0);   // retried ONCE
    CHECK(Fake::calls[MALLOC] == mallocs + 2 + 1 + 2 && c.cached_blocks() == 0 && Fake::clean());
    Fake::fail(GET_DEVICE, 1);
    CHECK(c.alloc(&p, MB, &cap) == MI_ERR_HIP && p == nullptr);
}

// how many blocks a cache of the given limits holds after the listed (bytes, device) blocks came back idle
size_t kept(size_t max_blocks, size_t dev_bytes, size_t total_bytes, const std::vector<std::pair<size_t, int>> &blocks, bool events = true)
{
    size_t n = 0;
    {
        Cache c(max_blocks, dev_bytes, total_bytes);
        std::vector<std::pair<void *, size_t>> held;
        for (const auto &b : blocks) {
            Fake::dev = b.second;
            void *p = nullptr;
            size_t cap = 0;
            CHECK(c.alloc(&p, b.first, &cap) == MI_OK && cap == b.first);
            held.push_back({p, cap});
        }
        Fake::dev = 0;
        for (const auto &h : held) c.free(h.first, h.second, events ? new_event() : Event(), true);
        n = c.cached_blocks();
        CHECK(Fake::blocks.size() == n && Fake::events.size() == (events ? n : 0));   // what was not taken is freed, its event destroyed
    }
    CHECK(Fake::clean());
    return n;
}

void take_back_rule()
{
    Fake::reset();
    const size_t big = 1 << 20;   // (in MB)
    CHECK(kept(4, big * MB, big * MB, {{10 * MB, 0}, {20 * MB, 0}, {30 * MB, 0}, {40 * MB, 0}}) == 4);                // blocks per device
    CHECK(kept(4, big * MB, big * MB, {{10 * MB, 0}, {20 * MB, 0}, {30 * MB, 0}, {40 * MB, 0}, {50 * MB, 0}}) == 4);
    CHECK(kept(4, big * MB, big * MB, {{10 * MB, 0}, {20 * MB, 0}, {30 * MB, 0}, {40 * MB, 0}, {50 * MB, 1}}) == 5);  // ... PER device
    CHECK(kept(4, 500 * MB, big * MB, {{200 * MB, 0}, {300 * MB, 0}}) == 2);                                          // bytes per device
    CHECK(kept(4, 500 * MB, big * MB, {{200 * MB, 0}, {300 * MB + 1, 0}}) == 1);
    CHECK(kept(4, 500 * MB, big * MB, {{200 * MB, 0}, {300 * MB + 1, 1}}) == 2);
    CHECK(kept(4, 500 * MB, 500 * MB, {{200 * MB, 0}, {300 * MB, 1}}) == 2);                                          // bytes per process
    CHECK(kept(4, 500 * MB, 500 * MB, {{200 * MB, 0}, {300 * MB + 1, 1}}) == 1);
    CHECK(kept(4, 0, big * MB, {{MB, 0}}) == 0 && kept(4, big * MB, 0, {{MB, 0}}) == 0);                              // a limit of 0 caches nothing
    CHECK(kept(4, 0, 0, {{MB, 0}, {MB, 1}}, false) == 0);
    // not idle: no event vouches for the block and the device cannot be synchronised
    Fake::reset();
    Fake::fail(DEV_SYNC, 1);
    CHECK(kept(4, big * MB, big * MB, {{MB, 0}}, false) == 0);
    CHECK(kept(4, big * MB, big * MB, {{MB, 0}}, false) == 1);
    // a block that is not kept although it came with an event: the event is waited for, destroyed, then the block freed
    Fake::reset();
    const size_t from = Fake::log.size();
    CHECK(kept(4, 0, 0, {{MB, 0}}) == 0);
    CHECK(joined(from) == "get_device malloc event_create get_device pointer_device event_sync event_destroy free get_device set_device:0");
}

void events_on_every_path()
{
    Fake::reset();
    {
        Cache c(4, 4096 * MB, 4096 * MB);
        c.free(nullptr, 0, new_event(), true);                     // no block: the event is destroyed, nothing else happens
        CHECK(Fake::events.empty() && Fake::calls[EV_DESTROY] == 1 && Fake::calls[GET_DEVICE] == 0);
        void *const blk = seed(c, 100 * MB, 0, true);
        CHECK(Fake::events.size() == 1);
        void *p = nullptr;
        size_t cap = 0;
        size_t from = Fake::log.size();
        CHECK(c.alloc(&p, 100 * MB, &cap) == MI_OK && p == blk);   // hit: waited for, destroyed, no device synchronisation
        CHECK(joined(from) == "get_device event_sync event_destroy" && Fake::events.empty());
        // the wait fails: sticky error cleared, the device synchronised instead, the block is used
        c.free(p, cap, new_event(), true);
        Fake::fail(EV_SYNC, 1);
        from = Fake::log.size();
        CHECK(c.alloc(&p, 100 * MB, &cap) == MI_OK && p == blk && cap == 100 * MB);
        CHECK(joined(from) == "get_device event_sync event_destroy clear device_sync@0" && Fake::events.empty());
        // ... and when that fails too: the block is freed, a fresh one allocated
        c.free(p, cap, new_event(), true);
        Fake::fail(EV_SYNC, 1);
        Fake::fail(DEV_SYNC, 1);
        from = Fake::log.size();
        CHECK(c.alloc(&p, 100 * MB, &cap) == MI_OK && p && cap == 100 * MB);
        CHECK(joined(from) == "get_device event_sync event_destroy clear device_sync@0 clear free malloc");
        CHECK(Fake::events.empty() && Fake::blocks.size() == 1);
        // the thread has no current device: nothing is cached, block and event go
        Fake::fail(GET_DEVICE, 1);
        c.free(p, cap, new_event(), true);
        CHECK(Fake::clean() && c.cached_blocks() == 0);
        // trim: every event waited for and destroyed, every block freed, the current device restored
        seed(c, 100 * MB, 0, true);
        seed(c, 300 * MB, 1, true);
        seed(c, 700 * MB, 1, false);
        Fake::dev = 1;
        from = Fake::log.size();
        c.trim();
        CHECK(joined(from) == "get_device event_sync event_destroy free event_sync event_destroy free free set_device:1");
        CHECK(Fake::clean() && Fake::dev == 1);
        Fake::dev = 0;
        seed(c, 100 * MB, 0, true);                                // left to the cache's destructor
    }
    CHECK(Fake::clean() && Fake::calls[EV_CREATE] == Fake::calls[EV_DESTROY]);
}

void busy_without_event()
{
    Fake::reset();
    Cache c(4, 4096 * MB, 4096 * MB);
    Fake::dev = 1;
    void *p = nullptr;
    size_t cap = 0;
    CHECK(c.alloc(&p, 100 * MB, &cap) == MI_OK);
    Fake::dev = 0;
    size_t from = Fake::log.size();
    c.free(p, cap, Event(), true);                                 // the BLOCK's device is synchronised, the current one restored
    CHECK(joined(from) == "get_device pointer_device set_device:1 device_sync@1 set_device:0" && Fake::dev == 0 && c.cached_blocks() == 1);
    Fake::dev = 1;
    CHECK(c.alloc(&p, 100 * MB, &cap) == MI_OK);
    from = Fake::log.size();
    c.free(p, cap, Event(), true);                                 // on its own device: no switch
    CHECK(joined(from) == "get_device pointer_device device_sync@1");
    CHECK(c.alloc(&p, 100 * MB, &cap) == MI_OK);
    from = Fake::log.size();
    c.free(p, cap, Event(), false);                                // never used: nothing to wait for
    CHECK(joined(from) == "get_device pointer_device");
    CHECK(c.alloc(&p, 100 * MB, &cap) == MI_OK);
    from = Fake::log.size();
    c.free(p, cap, new_event(), true);                             // an event vouches: no synchronisation
    CHECK(joined(from) == "event_create get_device pointer_device");
    Fake::dev = 0;
}

// ---------------------------------------------------------------- CachedArena
void arena_owner()
{
    Fake::reset();
    int stream_a = 0, stream_cap = 0;
    Fake::capturing.insert(&stream_cap);
    {
        Cache c(4, 4096 * MB, 4096 * MB);
        {
            Arena a(&c);
            size_t from = Fake::log.size();
            a.mark(&stream_a);                                     // no block: nothing at all
            a.release();
            CHECK(Fake::log.size() == from && !a.used() && !a.idle_valid() && !a.holds_event());

            // a valid mark, then release: the event goes to the cache with the block, none is kept
            CHECK(a.acquire(100 * MB) == MI_OK && a.get() && a.capacity() == 100 * MB && !a.used());
            void *const blk = a.get();
            from = Fake::log.size();
            a.mark(&stream_a);
            CHECK(joined(from) == "capturing event_create event_record" && a.used() && a.idle_valid() && a.holds_event());
            a.mark(&stream_a);                                     // every calc marks: the one event is recorded again
            CHECK(Fake::calls[EV_CREATE] == 1 && Fake::calls[EV_RECORD] == 2 && a.idle_valid());
            from = Fake::log.size();
            a.release();
            CHECK(joined(from) == "get_device pointer_device");     // (no synchronisation: the event vouches)
            CHECK(!a.get() && a.capacity() == 0 && !a.used() && !a.idle_valid() && !a.holds_event());
            CHECK(c.cached_blocks() == 1 && Fake::events.size() == 1);
            from = Fake::log.size();
            a.release();                                           // idempotent
            CHECK(Fake::log.size() == from && c.cached_blocks() == 1);
            from = Fake::log.size();
            CHECK(a.acquire(100 * MB) == MI_OK && a.get() == blk); // the next taker waits for that event
            CHECK(joined(from) == "get_device event_sync event_destroy" && Fake::events.empty());

            // under capture: used, no valid event, sticky error cleared, no event created
            from = Fake::log.size();
            a.mark(&stream_cap);
            CHECK(joined(from) == "capturing clear" && a.used() && !a.idle_valid() && !a.holds_event());
            // the capture query itself fails: the same
            Fake::fail(CAPTURING, 1);
            from = Fake::log.size();
            a.mark(&stream_a);
            CHECK(joined(from) == "capturing clear" && a.used() && !a.idle_valid() && !a.holds_event());
            // the event cannot be created
            Fake::fail(EV_CREATE, 1);
            from = Fake::log.size();
            a.mark(&stream_a);
            CHECK(joined(from) == "capturing event_create clear" && a.used() && !a.idle_valid() && !a.holds_event());
            // ... or not recorded: it exists, but does not count
            Fake::fail(EV_RECORD, 1);
            from = Fake::log.size();
            a.mark(&stream_a);
            CHECK(joined(from) == "capturing event_create event_record clear" && a.used() && !a.idle_valid() && a.holds_event());
            // such a block comes back busy with no event: the device is synchronised, the unused event stays with the arena
            from = Fake::log.size();
            a.release();
            CHECK(joined(from) == "get_device pointer_device device_sync@0" && a.holds_event() && Fake::events.size() == 1);
            a.reset();                                             // ... until the arena is reset: as constructed
            CHECK(!a.holds_event() && Fake::events.empty() && c.cached_blocks() == 1);
            // a mark that works after one that did not: valid again, with the event kept from before
            CHECK(a.acquire(100 * MB) == MI_OK && a.get() == blk);
            Fake::fail(EV_RECORD, 1);
            a.mark(&stream_a);
            CHECK(!a.idle_valid() && a.holds_event());
            a.mark(&stream_a);
            CHECK(a.idle_valid() && Fake::events.size() == 1 && Fake::calls[EV_CREATE] == 4);
            a.mark(&stream_cap);                                   // ... and a captured calc behind a valid mark takes the validity away
            CHECK(!a.idle_valid() && a.used() && a.holds_event());
            a.mark(&stream_a);
            CHECK(a.idle_valid());
            // acquire while holding: the old block goes back first (and, out of the window, is not the one handed out)
            CHECK(a.acquire(900 * MB) == MI_OK && a.get() != blk && a.capacity() == 900 * MB && !a.used() && c.cached_blocks() == 1);
            // a failed acquire leaves the arena empty
            Fake::fail(MALLOC, 1, 2);
            CHECK(a.acquire(5000 * MB) == MI_ERR_OOM && !a.get() && a.capacity() == 0);
            CHECK(Fake::clean());
            CHECK(a.acquire(100 * MB) == MI_OK);
            a.mark(&stream_a);
        }                                                          // the destructor releases, once
        CHECK(c.cached_blocks() == 1 && Fake::calls[FREE] == 2 && Fake::blocks.size() == 1 && Fake::events.size() == 1);
        {
            Arena b(&c);                                           // never marked: comes back unused, without an event or a synchronisation
            CHECK(b.acquire(300 * MB) == MI_OK);
            Arena never(&c);
        }
        CHECK(c.cached_blocks() == 2 && Fake::calls[DEV_SYNC] == 1);
    }
    CHECK(Fake::clean() && Fake::calls[EV_CREATE] == Fake::calls[EV_DESTROY] + 1);   // (one create was made to fail)
}

// three threads against one cache: what the mutex is for
void two_threads()
{
    Fake::reset();
    Fake::logging = false;
    {
        Cache c(4, 4096 * MB, 4096 * MB);
        auto work = [&c](int dev) {
            Fake::dev = dev;
            int stream = 0;
            for (int i = 0; i < 300; ++i) {
                Arena a(&c);
                if (a.acquire((size_t)(100 + 50 * (i % 3)) * MB) != MI_OK) { printf("FAIL: acquire in a thread\n"); exit(1); }
                if (i % 4) a.mark(&stream);
                if (i % 50 == 49) c.trim();
                if (i % 7 == 0) a.release();
            }
        };
        std::thread t0(work, 0), t1(work, 1), t2(work, 0);
        t0.join(); t1.join(); t2.join();
        CHECK(c.cached_blocks() <= 8 && Fake::blocks.size() == c.cached_blocks());
    }
    CHECK(Fake::clean());
}

}  // namespace

int main()
{
    owned_handle();
    hit_window();
    smallest_fitting_and_devices();
    alloc_failures();
    take_back_rule();
    events_on_every_path();
    busy_without_event();
    arena_owner();
    two_threads();
    CHECK(Fake::clean() && Tok::live.empty());                     // at exit: nothing left
    printf("own_test: ok (%d checks)\n", g_checks);
    return 0;
}
