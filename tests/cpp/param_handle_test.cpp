// cv::cuda::miflow_detail::ParamHandle (include/opencv2/core/cuda.hpp) over a fake C library: a toy params struct, handles that are
// malloc'd tokens (a leak or a second destroy is a sanitizer error, and the fake's own counters fail the plain build), a create and a
// set_params that reject on request.  Plain C++, no device, no libmiflow.  Run by tests/test_param_handle.py, plain and under the
// address / undefined-behaviour sanitizers.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "opencv2/core/cuda.hpp"

extern "C" const char *mi_last_error(void) { return "fake: rejected"; }   // all of libmiflow that miCheck asks for

namespace {

int g_checks = 0;
#define CHECK(c) do { ++g_checks; if (!(c)) { printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); exit(1); } } while (0)

struct toy_params { double rate; int level; char tag[4]; };   // no padding: the tests compare whole structs bit for bit
static_assert(sizeof(toy_params) == 16, "toy_params has padding");
struct toy { toy_params p; };

int g_creates = 0, g_sets = 0, g_destroys = 0, g_live = 0;
bool g_fail_create = false;

// level must lie in [1, 8], as a validating set_params of the library would ask
int check_params(const toy_params *p) { return p->level >= 1 && p->level <= 8 ? MI_OK : MI_ERR_BAD_ARG; }

int toy_create(const toy_params *p, toy **out)
{
    ++g_creates;
    if (g_fail_create || check_params(p) != MI_OK) return MI_ERR_BAD_ARG;
    *out = (toy *)malloc(sizeof(toy));
    (*out)->p = *p;
    ++g_live;
    return MI_OK;
}
int toy_create_extra(const toy_params *p, int extra, toy **out)
{
    const int rc = toy_create(p, out);
    if (rc == MI_OK) (*out)->p.level += extra;
    return rc;
}
int toy_set_params(toy *h, const toy_params *p)
{
    ++g_sets;
    if (check_params(p) != MI_OK) return MI_ERR_BAD_ARG;
    h->p = *p;
    return MI_OK;
}
int toy_get_params(const toy *h, toy_params *p) { *p = h->p; return MI_OK; }
void toy_destroy(toy *h)
{
    ++g_destroys;
    --g_live;
    free(h);
}

using Handle = cv::cuda::miflow_detail::ParamHandle<toy, toy_params, toy_create, toy_set_params, toy_destroy>;
using HandleExtra = cv::cuda::miflow_detail::ParamHandle<toy, toy_params, nullptr, toy_set_params, toy_destroy>;

toy_params make(int level, double rate)
{
    toy_params p;
    memset(&p, 0, sizeof(p));
    p.level = level; p.rate = rate; strcpy(p.tag, "toy");
    return p;
}
bool same(const toy_params &a, const toy_params &b) { return memcmp(&a, &b, sizeof(a)) == 0; }

template <class F> int thrown_code(F f)
{
    try { f(); } catch (const cv::Exception &e) { return e.code; }
    return 0;
}

void create_failure_throws_and_destroys_nothing()
{
    g_fail_create = true;
    CHECK(thrown_code([] { Handle h(make(3, 0.5)); }) == cv::Error::StsBadArg);
    g_fail_create = false;
    CHECK(thrown_code([] { Handle h(make(0, 0.5)); }) == cv::Error::StsBadArg);   // rejected by validation
    CHECK(thrown_code([] { HandleExtra h(make(0, 0.5), [](const toy_params *p, toy **o) { return toy_create_extra(p, 1, o); }); }) ==
          cv::Error::StsBadArg);
    CHECK(g_creates == 3 && g_destroys == 0 && g_live == 0);
}

void set_commits_on_acceptance_only()
{
    const int destroys0 = g_destroys;
    {
        Handle h(make(3, 0.5));
        CHECK(h.get() != nullptr && g_live == 1);
        CHECK(same(h.params(), make(3, 0.5)));

        h.set([](toy_params &q) { q.level = 5; q.rate = 0.25; });   // accepted: committed, and the library has it
        CHECK(same(h.params(), make(5, 0.25)) && same(h.get()->p, make(5, 0.25)));

        const toy_params before = h.params();
        const int sets0 = g_sets;
        CHECK(thrown_code([&] { h.set([](toy_params &q) { q.level = 9; q.rate = 7.0; }); }) == cv::Error::StsBadArg);
        CHECK(g_sets == sets0 + 1);                                        // the library was asked
        CHECK(same(h.params(), before) && same(h.get()->p, before));       // and nothing of the edit stays, the valid field neither

        h.set([](toy_params &q) { q.rate = 1.5; });                        // the object is not stuck: a valid setter succeeds
        CHECK(same(h.params(), make(5, 1.5)) && same(h.get()->p, make(5, 1.5)));
        CHECK(g_destroys == destroys0);
    }
    CHECK(g_destroys == destroys0 + 1 && g_live == 0);   // destroyed exactly once
}

void refresh_overwrites_the_kept_struct()
{
    Handle h(make(4, 0.5));
    h.get()->p.level = 2;   // a calc of the library shrinks a value on its side
    CHECK(h.params().level == 4);
    h.refresh(toy_get_params);
    CHECK(same(h.params(), make(2, 0.5)));
    h.set([](toy_params &q) { q.rate = 2.0; });   // the next setter starts from the refreshed struct
    CHECK(same(h.get()->p, make(2, 2.0)));
}

void create_with_a_further_argument()
{
    const int destroys0 = g_destroys;
    {
        HandleExtra h(make(3, 0.5), [](const toy_params *p, toy **o) { return toy_create_extra(p, 2, o); });
        CHECK(h.get()->p.level == 5 && h.params().level == 3);   // the kept struct is what was asked for
        h.set([](toy_params &q) { q.level = 6; });
        CHECK(h.get()->p.level == 6 && h.params().level == 6);
    }
    CHECK(g_destroys == destroys0 + 1 && g_live == 0);
}

}  // namespace

int main()
{
    create_failure_throws_and_destroys_nothing();
    set_commits_on_acceptance_only();
    refresh_overwrites_the_kept_struct();
    create_with_a_further_argument();
    CHECK(g_live == 0 && g_destroys == g_creates - 3);   // every handle that was created was destroyed, the three failures never
    printf("param_handle_test: ok (%d checks)\n", g_checks);
    return 0;
}
