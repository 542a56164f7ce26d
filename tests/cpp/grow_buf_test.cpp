// GrowBuf (csrc/mi_buf.h) on the host: an allocator that counts its calls, can fail the k-th of them and knows every live block.
// Plain C++, no device.  Run by tests/test_grow_buf.py, plain and under the address / undefined-behaviour sanitizers.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <set>
#include <string>
#include <vector>
#include "mi_buf.h"

namespace mi {
static char g_err[256];
void set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
}  // namespace mi

namespace {

const int kFailCode = MI_ERR_HIP;   // not MI_ERR_OOM: a buffer has to hand on the allocator's code, not one of its own

struct Counting {
    static int calls, fail_at, frees;          // fail_at: the 1-based alloc call that fails (0: none)
    static std::set<void *> live;
    static std::vector<std::string> log;       // "a" per successful alloc, "f" per free, "x" per failed alloc
    static void reset(int fail = 0) { calls = 0; fail_at = fail; frees = 0; log.clear(); }
    static int alloc(void **p, size_t bytes)
    {
        if (++calls == fail_at) { log.push_back("x"); mi::set_error("counting allocator: call %d fails", calls); return kFailCode; }
        *p = malloc(bytes ? bytes : 1);
        live.insert(*p);
        log.push_back("a");
        return MI_OK;
    }
    static void free(void *p)
    {
        if (!live.erase(p)) { printf("FAIL: free of a block that is not live\n"); exit(1); }
        ::free(p);
        ++frees;
        log.push_back("f");
    }
};
int Counting::calls, Counting::fail_at, Counting::frees;
std::set<void *> Counting::live;
std::vector<std::string> Counting::log;

template <class T> using Buf = mi::GrowBuf<T, Counting>;

int g_checks = 0;
#define CHECK(c) do { ++g_checks; if (!(c)) { printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); exit(1); } } while (0)

std::string joined() { std::string s; for (const auto &e : Counting::log) s += e; return s; }

void grow_only()
{
    Counting::reset();
    Buf<int> b;
    CHECK(b.p == nullptr && b.n == 0);
    CHECK(b.ensure(10) == MI_OK && b.p && b.n == 10);
    int *const first = b.p;
    for (int i = 0; i < 10; ++i) b.p[i] = i;   // (the sanitizer run sees an allocation shorter than n elements)
    CHECK(b.ensure(4) == MI_OK && b.p == first && b.n == 10);    // a smaller request keeps the block
    CHECK(b.ensure(10) == MI_OK && b.p == first && b.n == 10);
    CHECK(Counting::calls == 1 && Counting::frees == 0);
    CHECK(b.ensure(11) == MI_OK && b.n == 11);
    for (int i = 0; i < 11; ++i) b.p[i] = i;
    CHECK(joined() == "afa");                                     // release BEFORE allocate: never two blocks live
    CHECK(Counting::live.size() == 1);
}

void failed_growth()
{
    Counting::reset(2);
    {
        Buf<double> b;
        CHECK(b.ensure(8) == MI_OK);
        CHECK(b.ensure(16) == kFailCode);                         // the allocator's code
        CHECK(b.p == nullptr && b.n == 0);                        // empty, not the old block and not a dangling pointer
        CHECK(joined() == "afx" && Counting::frees == 1 && Counting::live.empty());   // old block freed exactly once
        CHECK(b.ensure(4) == MI_OK && b.p && b.n == 4);           // usable again
        b.p[3] = 1.0;
    }
    CHECK(joined() == "afxaf" && Counting::live.empty());
}

void zero_and_overflow()
{
    Counting::reset();
    Buf<long long> b;
    CHECK(b.ensure(0) == MI_OK && b.p == nullptr && b.n == 0 && Counting::calls == 0);   // nothing wanted, nothing allocated
    mi::g_err[0] = 0;
    CHECK(b.ensure((size_t)-1 / sizeof(long long) + 1) == MI_ERR_OOM);                   // byte count wraps: refused before the allocator
    CHECK(Counting::calls == 0 && b.p == nullptr && b.n == 0 && mi::g_err[0] != 0);
    CHECK(b.ensure((size_t)-1) == MI_ERR_OOM && Counting::calls == 0);
    CHECK(b.ensure(3) == MI_OK && b.n == 3);
    CHECK(b.ensure((size_t)-1) == MI_ERR_OOM && b.p == nullptr && b.n == 0 && Counting::live.empty());   // empty after ANY failed growth
    Buf<char> c;
    CHECK(c.ensure(5) == MI_OK && c.ensure(0) == MI_OK && c.n == 5);
}

void release_and_destructor()
{
    Counting::reset();
    {
        Buf<float> b;
        b.release();                                              // on an empty buffer: nothing
        CHECK(Counting::frees == 0);
        CHECK(b.ensure(7) == MI_OK);
        b.release();
        CHECK(b.p == nullptr && b.n == 0 && Counting::frees == 1);
        b.release();
        CHECK(Counting::frees == 1);                              // idempotent
        CHECK(b.ensure(2) == MI_OK);
    }
    CHECK(Counting::frees == 2 && Counting::live.empty());        // the destructor frees, once
    { Buf<float> never; }
    CHECK(Counting::frees == 2);
}

// Two buffers a call ensures one after the other (StereoBM's lebuf / ribuf), for every choice of the failing allocator call: a call that
// reports MI_OK has both, and the retry after a failure ends with both -- never "MI_OK with one of them null".
int ensure_pair(Buf<unsigned char> &le, Buf<unsigned char> &ri, size_t n)
{
    if (const int rc = le.ensure(n)) return rc;
    return ri.ensure(n);
}

void pair_with_failures()
{
    for (int fail = 0; fail <= 6; ++fail) {
        Counting::reset(fail);
        {
            Buf<unsigned char> le, ri;
            int failures = 0;
            for (const size_t n : {(size_t)100, (size_t)100, (size_t)300, (size_t)50}) {
                int rc = ensure_pair(le, ri, n);
                if (rc) {
                    ++failures;
                    CHECK(rc == kFailCode);
                    CHECK((le.p == nullptr) == (le.n == 0) && (ri.p == nullptr) == (ri.n == 0));   // each is empty or whole
                    CHECK(le.p == nullptr || ri.p == nullptr);    // ... and the one that failed is empty
                    rc = ensure_pair(le, ri, n);                  // the next call: the same request again
                }
                CHECK(rc == MI_OK && le.p && ri.p && le.n >= n && ri.n >= n);
                le.p[n - 1] = ri.p[n - 1] = 1;
                CHECK(Counting::live.size() == 2);
            }
            CHECK(failures == (fail >= 1 && fail <= 4 ? 1 : 0));  // the sequence makes four allocator calls when none fails
        }
        CHECK(Counting::live.empty());
    }
}

}  // namespace

int main()
{
    grow_only();
    CHECK(Counting::live.empty());
    failed_growth();
    zero_and_overflow();
    CHECK(Counting::live.empty());
    release_and_destructor();
    pair_with_failures();
    CHECK(Counting::live.empty());                                // at exit: no block left
    printf("grow_buf_test: ok (%d checks)\n", g_checks);
    return 0;
}
