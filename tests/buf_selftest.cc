// buf_selftest.cc -- the worker's owning buffer types (inferflow_amd/csrc/ifa_buf.h) over malloc-backed spaces with a failure
// switch and a live counter.  A plain program: tests/test_buf_cpu.py builds it with the address + undefined sanitizers and runs it.
#include <cstdio>
#include <cstdlib>
#include <utility>
#include "ifa_buf.h"

static long g_live = 0, g_allocs = 0, g_frees = 0, g_fail_at = 0;      // g_fail_at: the n-th alloc from now fails once (0: off)

template <int Tag> struct FakeSpace {
    static int alloc(void **p, size_t bytes)
    {
        if (g_fail_at > 0 && --g_fail_at == 0) { *p = nullptr; return -7; }
        *p = malloc(bytes ? bytes : 1);
        if (!*p) return -2;
        g_live++; g_allocs++;
        return 0;
    }
    static void free(void *p) { ::free(p); g_live--; g_frees++; }
};
using Dev = FakeSpace<0>;
using Pin = FakeSpace<1>;
using IntBuf = ifa::Buf<int, Dev>;
using Pair = ifa::Staged<int, Dev, Pin>;

static int g_failed = 0;
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); g_failed++; } } while (0)

static void test_alloc_and_scope()
{
    {
        IntBuf b;
        CHECK(!b && b.cap() == 0);
        CHECK(b.alloc(10) == 0 && b && b.cap() == 10 && g_live == 1);
        b[9] = 5; *(b + 3) = 4;                     // reads as an int *
        int *raw = b;
        CHECK(raw[9] == 5 && raw[3] == 4);
        const long frees = g_frees;
        CHECK(b.alloc(20) == 0 && b.cap() == 20);   // alloc over a held block frees it
        CHECK(g_frees == frees + 1 && g_live == 1);
        b[19] = 1;
        b.reset();
        CHECK(!b && b.cap() == 0 && g_live == 0);
        CHECK(b.alloc(3) == 0);
    }
    CHECK(g_live == 0);
    {
        ifa::Buf<void, Dev> bytes;                  // capacity in bytes
        CHECK(bytes.alloc(33) == 0 && bytes.cap() == 33);
        static_cast<char *>(static_cast<void *>(bytes))[32] = 1;
    }
    CHECK(g_live == 0);
}

static void test_failed_alloc()
{
    {
        IntBuf b;
        CHECK(b.alloc(4) == 0);
        g_fail_at = 1;
        CHECK(b.alloc(8) == -7);                    // the space's code comes back
        CHECK(!b && b.cap() == 0 && g_live == 0);   // empty, and the old block is gone (not leaked, not dangling)
        CHECK(b.alloc(8) == 0 && b.cap() == 8);     // usable afterwards
    }
    CHECK(g_live == 0);
}

static void test_moves()
{
    {
        IntBuf a;
        CHECK(a.alloc(4) == 0);
        int *pa = a;
        IntBuf b(std::move(a));                     // move construction
        CHECK(!a && a.cap() == 0 && (int *)b == pa && b.cap() == 4 && g_live == 1);
        IntBuf c;
        CHECK(c.alloc(6) == 0 && g_live == 2);
        const long frees = g_frees;
        c = std::move(b);                           // move assignment: c's old block freed exactly once
        CHECK(g_frees == frees + 1 && g_live == 1);
        CHECK(!b && b.cap() == 0 && (int *)c == pa && c.cap() == 4);
        IntBuf &self = c;
        c = std::move(self);                        // self-move keeps the block
        CHECK((int *)c == pa && c.cap() == 4 && g_live == 1);
        c[3] = 7;
    }
    CHECK(g_live == 0);
}

static void test_staged()
{
    {
        Pair p;
        CHECK(p.cap() == 0 && !p.dev && !p.pin);
        CHECK(p.reserve(16) == 0 && p.cap() == 16 && p.dev && p.pin && g_live == 2);
        int *d = p.dev, *h = p.pin;
        CHECK(p.reserve(8) == 0 && (int *)p.dev == d && (int *)p.pin == h);      // no shrink, no move
        p.dev[15] = 1; p.pin[15] = 1;
        g_fail_at = 2;                              // growth whose SECOND allocation fails: holds nothing
        CHECK(p.reserve(32) == -7);
        CHECK(p.cap() == 0 && !p.dev && !p.pin && g_live == 0);
        g_fail_at = 1;                              // ... and whose first fails
        CHECK(p.reserve(32) == -7 && p.cap() == 0 && !p.dev && !p.pin && g_live == 0);
        CHECK(p.reserve(4) == 0 && p.cap() == 4 && g_live == 2);                 // the next call allocates again
        Pair q(std::move(p));
        CHECK(p.cap() == 0 && !p.dev && !p.pin && q.cap() == 4 && g_live == 2);
        Pair r;
        CHECK(r.reserve(2) == 0 && g_live == 4);
        r = std::move(q);
        CHECK(g_live == 2 && r.cap() == 4 && q.cap() == 0);
    }
    CHECK(g_live == 0);
}

int main()
{
    test_alloc_and_scope();
    test_failed_alloc();
    test_moves();
    test_staged();
    CHECK(g_live == 0 && g_allocs == g_frees && g_fail_at == 0);
    if (g_failed) { fprintf(stderr, "buf_selftest: %d checks failed\n", g_failed); return 1; }
    printf("buf_selftest ok (%ld allocations)\n", g_allocs);
    return 0;
}
