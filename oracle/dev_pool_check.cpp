// dev_pool_check — drives csrc/dev_pool.h on the CPU with a counting backend that fails the k-th
// request, for every k from 1 to the number of requests of the script below (and once with no
// failure).  Built with -fsanitize=address,undefined (oracle/Makefile) and run as a child process
// by tests/test_dev_pool.py.  Exit status 0 and one line of counts, or the first broken rule.
#include "dev_pool.h"
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <set>
#include <vector>

using namespace vo;

static struct Backend {
    long requests = 0, fail_at = 0, failures = 0, made = 0, dropped = 0, bad_drops = 0;
    uintptr_t next = 0;
    std::set<void*> live;
    std::vector<PoolKind> drop_order;
} g;

static int fake_make(PoolKind kind, size_t bytes, void** out)
{
    if (++g.requests == g.fail_at) { g.failures += 1; return 2; }   // the runtime's "out of memory"
    if ((kind == POOL_EVENT || kind == POOL_STREAM) != (bytes == 0)) return 1;
    *out = (void*)(++g.next * 64);
    g.live.insert(*out);
    g.made += 1;
    return 0;
}

static void fake_drop(PoolKind kind, void* h)
{
    if (g.live.erase(h) != 1) g.bad_drops += 1;                      // released twice, or never made
    g.dropped += 1;
    g.drop_order.push_back(kind);
}

#define CHECK(cond)                                                                               \
    do {                                                                                          \
        if (!(cond)) {                                                                            \
            printf("dev_pool_check: fail_at=%ld line %d: %s\n", g.fail_at, __LINE__, #cond);      \
            exit(1);                                                                              \
        }                                                                                         \
    } while (0)

struct Event;      // the runtime's handles are pointers to opaque types
struct Stream;

// The script: single allocations of each kind, a group of four, a grow-and-retire sequence, the
// releases that must do nothing, destruction.  Every step tolerates the injected failure and
// checks what the header promises about it.
static void script()
{
    std::vector<void*> retired;
    {
        DevPool pool(PoolBackend{fake_make, fake_drop});
        float* dev = nullptr; int* pin = nullptr; Event* ev = nullptr; Stream* st = nullptr;
        size_t live = 0;
        int rc = 0;
        auto single = [&](const void* p) {
            CHECK((rc == 0) == (p != nullptr));
            live += rc == 0;
            CHECK(pool.live() == live && g.live.size() == live);
        };
        rc = pool.alloc(dev, 100); single(dev);
        rc = pool.pinned(pin, 7); single(pin);
        rc = pool.event(ev); single(ev);
        rc = pool.stream(st); single(st);
        Stream* st2 = nullptr;                              // a second stream, made before the next event
        rc = pool.stream(st2); single(st2);
        Event* ev2 = nullptr;
        rc = pool.event(ev2); single(ev2);

        // group of four: all or nothing
        double* a = nullptr; uint8_t* b = nullptr; int* c = nullptr; float* d = nullptr;
        rc = pool.group({DevPool::req(a, 3), DevPool::req(b, 5), DevPool::req(c, 1), DevPool::req(d, 9)});
        if (rc) CHECK(!a && !b && !c && !d);
        else { CHECK(a && b && c && d); live += 4; }
        CHECK(pool.live() == live && g.live.size() == live);

        // grow and retire: from nothing; to a larger pair with the old one retired (still owned);
        // to a larger one with the old one released at once.  A failure leaves the old pair.
        float* X = nullptr; uint8_t* keep = nullptr;
        rc = pool.grow({DevPool::req(X, 3 * 16), DevPool::req(keep, 16)}, &retired);
        if (rc) CHECK(!X && !keep);
        else { CHECK(X && keep); live += 2; }
        CHECK(retired.empty() && pool.live() == live);
        float* oX = X; uint8_t* ok = keep;
        rc = pool.grow({DevPool::req(X, 3 * 32), DevPool::req(keep, 32)}, &retired);
        if (rc) CHECK(X == oX && keep == ok && retired.empty());
        else {
            CHECK(X && keep && X != oX && keep != ok);
            CHECK(retired.size() == (oX ? 2u : 0u));
            for (void* p : retired) CHECK(g.live.count(p) == 1);
            live += 2;
        }
        CHECK(pool.live() == live && g.live.size() == live);
        oX = X; ok = keep;
        rc = pool.grow({DevPool::req(X, 3 * 64), DevPool::req(keep, 64)});
        if (rc) CHECK(X == oX && keep == ok);
        else {
            CHECK(X && keep);
            if (oX) CHECK(X != oX && g.live.count(oX) == 0 && g.live.count(ok) == 0);
            else live += 2;
        }
        CHECK(pool.live() == live && g.live.size() == live);
        for (void*& p : retired) {
            pool.release(p);
            CHECK(!p);
            live -= 1;
        }
        CHECK(pool.live() == live && g.live.size() == live);

        // releases that do nothing: null, a pointer the pool never made, one released already
        int* none = nullptr;
        pool.release(none);
        int local = 0;
        int* unknown = &local;
        pool.release(unknown);
        CHECK(unknown == &local);
        float* stale = dev;
        pool.release(dev);
        CHECK(!dev);
        live -= stale != nullptr;
        pool.release(stale);
        CHECK(pool.live() == live && g.live.size() == live && g.bad_drops == 0);
        g.drop_order.clear();
    }
    // destruction: everything released once, memory before events before streams
    CHECK(g.live.empty() && g.made == g.dropped && g.bad_drops == 0);
    int rank = 0;
    for (PoolKind k : g.drop_order) {
        const int r = k == POOL_STREAM ? 2 : k == POOL_EVENT ? 1 : 0;
        CHECK(r >= rank);
        rank = r;
    }
}

int main()
{
    script();
    const long n = g.requests;
    CHECK(n > 0 && g.failures == 0);
    long injected = 0, handles = g.made, twice = g.bad_drops, leaked = (long)g.live.size();
    for (long k = 1; k <= n; ++k) {
        g = Backend();
        g.fail_at = k;
        script();
        CHECK(g.failures == 1);
        injected += g.failures;
        handles += g.made;
        twice += g.bad_drops;
        leaked += (long)g.live.size();
    }
    printf("dev_pool_check ok: requests=%ld runs=%ld failures_injected=%ld handles=%ld double_releases=%ld leaked=%ld\n", n,
           n + 1, injected, handles, twice, leaked);
    return 0;
}
