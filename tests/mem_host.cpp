// mem_host.cpp -- csrc/q3_mem.h on the host: DevMem / PinMem over an allocator that counts, logs and can fail the k-th request.
// A stand-alone program (tests/test_host_and_abi.py builds it with -fsanitize=address,undefined and runs it): no HIP, no GPU.
// Sizes are the smallest that can go wrong: capacities 0 and 1, need == n, need == n + 1.
#define Q3_MEM_NO_HIP
#include "q3_mem.h"

#include <cstdio>
#include <cstdlib>
#include <set>
#include <string>

#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
            exit(1);                                                         \
        }                                                                    \
    } while (0)

namespace {

struct Fake {
    typedef int Stream;
    static std::set<void*> live;
    static std::string log;          // 'a' allocate, 'f' release, 'w' wait, in call order
    static long requests, fail_at;   // fail_at: the request, counted from 1, that is refused (0: none)
    static int allocate(void** p, size_t bytes) {
        if (++requests == fail_at) return -4;
        *p = malloc(bytes ? bytes : 1);
        CHECK(*p && live.insert(*p).second);
        log += 'a';
        return 0;
    }
    static void release(void* p) {
        CHECK(live.erase(p) == 1);   // freed exactly once
        free(p);
        log += 'f';
    }
    static int wait(Stream st) {
        CHECK(st == 7);
        log += 'w';
        return 0;
    }
    static void start(long fail = 0) {
        CHECK(live.empty());
        log.clear();
        requests = 0;
        fail_at = fail;
    }
};
std::set<void*> Fake::live;
std::string Fake::log;
long Fake::requests = 0, Fake::fail_at = 0;

typedef DevMem<int, Fake> Dev;
typedef PinMem<int, Fake> Pin;

template <class M> auto has_grow(int) -> decltype(&M::grow, true) { return true; }
template <class M> bool has_grow(...) { return false; }

void move_and_swap() {
    Fake::start();
    {
        Dev a;
        CHECK(!a && a.n == 0);
        CHECK(a.alloc(3) == 0 && a && a.n == 3);
        a[2] = 5;
        Dev b(std::move(a));
        CHECK(!a && a.n == 0 && b.n == 3 && b[2] == 5);
        Dev c;
        CHECK(c.alloc(1) == 0 && Fake::live.size() == 2);
        c = std::move(b);                        // frees what c held
        CHECK(!b && c.n == 3 && c[2] == 5 && Fake::live.size() == 1);
        c.swap(a);
        CHECK(!c && c.n == 0 && a.n == 3 && a[2] == 5);
        CHECK(a.alloc(1) == 0 && a.n == 1 && Fake::live.size() == 1);   // a fresh allocation frees the old one
        CHECK(c.alloc(0) == 0 && c.n == 0);      // zero elements: whatever the allocator returns is owned and freed
        a.reset();
        a.reset();
        CHECK(!a && a.n == 0 && Fake::live.size() == 1);
        Pin h;
        CHECK(h.alloc(2) == 0 && h.n == 2);
        h[1] = 9;
        Pin g = std::move(h);
        CHECK(!h && g[1] == 9 && Fake::live.size() == 2);
    }
    CHECK(Fake::live.empty() && Fake::log.size() == 10);      // five allocations, each freed once (release() checks the once)
    CHECK(has_grow<Dev>(0) && !has_grow<Pin>(0));
}

void grow() {
    Fake::start();
    {
        Dev a;
        CHECK(a.grow(0, 7) == 0 && !a && a.n == 0 && Fake::log.empty());         // capacity 0, need 0
        CHECK(a.grow(1, 7) == 0 && a && a.n == 1 && Fake::log == "wa");
        Fake::log.clear();
        int* const p = a;
        CHECK(a.grow(1, 7) == 0 && a.grow(0, 7) == 0 && a == p && a.n == 1);     // need == n, need < n: neither allocation nor wait
        CHECK(Fake::log.empty());
        CHECK(a.grow(2, 7) == 0 && a.n == 2 && Fake::live.size() == 1);          // need == n + 1
        CHECK(Fake::log == "wfa");                                               // one wait, in front of the free
        a[1] = 1;
    }
    CHECK(Fake::live.empty());
}

void failed_grow() {
    Fake::start(2);
    {
        Dev a;
        CHECK(a.alloc(1) == 0);
        CHECK(a.grow(2, 7) != 0 && !a && a.n == 0 && Fake::live.empty() && Fake::log == "awf");
        CHECK(a.grow(2, 7) == 0 && a.n == 2 && Fake::log == "awfwa");
        a[1] = 1;
    }
    CHECK(Fake::live.empty());
    Fake::start(1);
    Dev b;
    CHECK(b.alloc(1) != 0 && !b && b.n == 0 && Fake::live.empty());
}

// An all-or-nothing group as the library writes it (q3_sampler_set): four buffers into locals, committed together.
struct Ctx {
    Dev a;
    DevMem<double, Fake> b;
    Dev c;
    Pin d;
};
int group_get(Ctx& x) {
    if (x.a) return 0;               // the first buffer stands for the group
    Dev a, c;
    DevMem<double, Fake> b;
    Pin d;
    int rc;
    if ((rc = a.alloc(1)) || (rc = b.alloc(2)) || (rc = c.alloc(1)) || (rc = d.alloc(1))) return rc;
    x.a = std::move(a);
    x.b = std::move(b);
    x.c = std::move(c);
    x.d = std::move(d);
    return 0;
}
void group() {
    for (long k = 1; k <= 4; ++k) {
        Fake::start(k);
        {
            Ctx x;
            CHECK(group_get(x) != 0);
            CHECK(!x.a && !x.b && !x.c && !x.d && Fake::live.empty());           // the context holds nothing, nothing is left behind
            CHECK(group_get(x) == 0);                                            // the retry starts from the first buffer
            CHECK(x.a && x.b && x.c && x.d && x.b.n == 2 && Fake::live.size() == 4);
            x.b[1] = 1.0;
            const long before = Fake::requests;
            CHECK(group_get(x) == 0 && Fake::requests == before);
        }
        CHECK(Fake::live.empty());
    }
}

}  // namespace

int main() {
    move_and_swap();
    grow();
    failed_grow();
    group();
    puts("mem_host ok");
    return 0;
}
