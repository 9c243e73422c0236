// Host check of csrc/ctg_pool.h and csrc/ctg_buffers.h for tests/test_pool.py:
// the caching allocator and the self-owning buffers over a fake back end --
// malloc / free with a ledger of live blocks and a switch that refuses chosen
// allocations or frees, and a stream_wait that logs into the same event list
// as dev_free (the order of a StreamWait and the buffers of its scope).  Prints "class BYTES ROUNDED" lines (the size-class
// table at its edges) and one "ok NAME" line per case that held; the first
// broken expectation ends the run with its line number.
//
// g++ -std=c++17 -fsanitize=address,undefined tools/pool_check.cpp -o pool_check
#include <cstdio>
#include <cstdlib>
#include <map>
#include <set>
#include <utility>
#include <vector>

#include "../cluster_tools_amd/csrc/ctg_buffers.h"
#include "../cluster_tools_amd/csrc/ctg_pool.h"

using namespace ctg;

#define EXPECT(c)                                                              \
    do {                                                                       \
        if (!(c)) {                                                            \
            fprintf(stderr, "pool_check:%d: %s does not hold\n", __LINE__, #c); \
            exit(1);                                                           \
        }                                                                      \
    } while (0)

// ---------------------------------------------------------------------------
// the fake back end
// ---------------------------------------------------------------------------
struct Ledger {
    std::map<void*, size_t> live;   // blocks handed out and not yet freed
    long n_alloc = 0, n_free = 0;   // calls so far
    long refuse_alloc = -1, refuse_allocs = 0;   // allocations [refuse_alloc, refuse_alloc + refuse_allocs) fail
    long refuse_free = -1;                       // this free fails
    int bad_frees = 0;                           // frees of a block that is not live (double or foreign)
    std::vector<std::pair<char, void*>> events;  // ('f', block) of every dev_free, ('w', stream) of every stream_wait
    void refuse_next_allocs(long n) { refuse_alloc = n_alloc, refuse_allocs = n; }
};
static Ledger g_led;

static int fake_alloc(void** p, size_t bytes) {
    const long i = g_led.n_alloc++;
    if (i >= g_led.refuse_alloc && i < g_led.refuse_alloc + g_led.refuse_allocs) return 2;
    *p = malloc(bytes);
    g_led.live[*p] = bytes;
    return 0;
}

static int fake_free(void* p) {
    if (g_led.n_free++ == g_led.refuse_free) return 1;
    auto it = g_led.live.find(p);
    if (it == g_led.live.end()) {
        ++g_led.bad_frees;
        return 0;
    }
    free(p);
    g_led.live.erase(it);
    return 0;
}

// dev_alloc / dev_free as ctg_workspace.hip defines them, over the pool of the running case
static DevicePool* g_pool = nullptr;
static int g_device = 0;   // the "current device"
void* ctg::dev_alloc(size_t bytes) { return g_pool->alloc(g_device, bytes); }
void ctg::dev_free(void* p) {
    if (p) g_led.events.emplace_back('f', p);
    g_pool->free(p);
}
void ctg::stream_wait(void* stream) { g_led.events.emplace_back('w', stream); }
using Events = std::vector<std::pair<char, void*>>;

static std::set<void*> cached(DevicePool& pool, int device) {
    std::set<void*> s;
    pool.for_each_cached(device, [&](size_t, void* p) { EXPECT(s.insert(p).second); });
    return s;
}

// every cached block is live at the back end
static void expect_cache_live(DevicePool& pool, int device) {
    for (void* p : cached(pool, device)) EXPECT(g_led.live.count(p) == 1);
}

// One case: a fresh ledger and pool; when the body is done every device is
// purged, and nothing may be left at the back end or have been freed twice.
template <class F>
static void run_case(const char* name, F&& body) {
    g_led = Ledger{};
    g_device = 0;
    DevicePool pool(fake_alloc, fake_free);
    g_pool = &pool;
    body(pool);
    for (int d = 0; d < DevicePool::MAX_DEVICES; ++d) EXPECT(pool.purge(d) == 0);
    EXPECT(g_led.live.empty());
    EXPECT(g_led.bad_frees == 0);
    g_pool = nullptr;
    printf("ok %s\n", name);
}

int main() {
    // the size classes at their edges (compared in tests/test_pool.py), idempotent
    const size_t Mi = 1u << 20;
    const size_t edges[] = {0, 1, 255, 256, 257, 511, 512, 513, Mi - 1, Mi, Mi + 1, Mi + Mi / 4, Mi + Mi / 4 + 1,
                            1638400, 1638401, (size_t)1 << 31, ((size_t)1 << 32) + 1, (size_t)1 << 36};
    for (size_t b : edges) {
        const size_t r = pool_round_up(b);
        EXPECT(r >= b && pool_round_up(r) == r);
        printf("class %zu %zu\n", b, r);
    }

    run_case("reuse_bound", [](DevicePool& pool) {
        void* a = pool.alloc(0, 1000);   // class 1024
        EXPECT(a && g_led.live[a] == 1024 + DevicePool::SLACK);
        pool.free(a);
        EXPECT(pool.alloc(0, 512) == a);   // exactly twice the request: reused
        pool.free(a);
        void* z = pool.alloc(0, 0);        // class 256, four times: a raw allocation
        EXPECT(z && z != a && g_led.n_alloc == 2);
        void* b = pool.alloc(0, 2048);
        pool.free(b);
        EXPECT(pool.alloc(0, 512) == a);   // the smallest fitting block is looked at, not 2048
        // past 1 MiB the classes step by 1.25: three steps up (1.95x) are reused, four (2.44x) are not
        void* c = pool.alloc(0, 2560000);
        void* d = pool.alloc(0, 3200000);
        EXPECT(g_led.live[c] == 2560000 + DevicePool::SLACK && g_led.live[d] == 3200000 + DevicePool::SLACK);
        pool.free(d);
        const long before = g_led.n_alloc;
        void* e = pool.alloc(0, 1310720);
        EXPECT(e != d && g_led.n_alloc == before + 1);
        pool.free(c);
        EXPECT(pool.alloc(0, 1310720) == c && g_led.n_alloc == before + 1);
        pool.free(nullptr);
        int not_ours = 0;
        pool.free(&not_ours);   // ignored
        EXPECT(cached(pool, 0) == (std::set<void*>{b, d}));
        for (void* p : {a, c, e, z}) pool.free(p);
    });

    run_case("purge_and_retry", [](DevicePool& pool) {
        void* a = pool.alloc(0, 4096);
        pool.free(a);
        g_led.refuse_next_allocs(1);
        void* b = pool.alloc(0, 1 << 16);   // refused, the cache purged, retried
        EXPECT(b && g_led.n_alloc == 3 && g_led.n_free == 1);
        EXPECT(cached(pool, 0).empty() && g_led.live.size() == 1 && g_led.live.count(b));
        pool.free(b);
    });

    run_case("purge_and_retry_refused", [](DevicePool& pool) {
        void* a = pool.alloc(0, 4096);
        void* held = pool.alloc(0, 4096);
        pool.free(a);
        g_led.refuse_next_allocs(2);
        EXPECT(pool.alloc(0, 1 << 16) == nullptr);
        // the cache went to the back end, the block in use did not
        EXPECT(cached(pool, 0).empty() && g_led.live.size() == 1 && g_led.live.count(held));
        void* b = pool.alloc(0, 1 << 16);   // the back end has recovered
        EXPECT(b && b != held);
        pool.free(b);
        pool.free(held);
        EXPECT(cached(pool, 0).size() == 2);
    });

    run_case("freed_to_allocating_device", [](DevicePool& pool) {
        g_device = 1;
        void* a = dev_alloc(1000);
        g_device = 0;   // another device is current when the block comes back
        dev_free(a);
        EXPECT(cached(pool, 0).empty() && cached(pool, 1) == std::set<void*>{a});
        void* b = dev_alloc(1000);   // device 0 does not get device 1's block
        EXPECT(b && b != a);
        g_device = 1;
        EXPECT(dev_alloc(1000) == a);
        dev_free(a);
        dev_free(b);
        EXPECT(cached(pool, 0) == std::set<void*>{b} && cached(pool, 1) == std::set<void*>{a});
    });

    run_case("purge_with_refused_free", [](DevicePool& pool) {
        void* p[3] = {pool.alloc(0, 256), pool.alloc(0, 4096), pool.alloc(0, 1 << 16)};
        for (void* q : p) pool.free(q);
        g_led.refuse_free = g_led.n_free + 1;   // the second of the three
        EXPECT(pool.purge(0) == 1);             // reported
        // the two freed blocks left the pool; the one whose free failed is still a live block
        EXPECT(cached(pool, 0) == std::set<void*>{p[1]} && g_led.live.size() == 1);
        expect_cache_live(pool, 0);
        EXPECT(pool.alloc(0, 4096) == p[1]);
        pool.free(p[1]);
    });

    run_case("dev_buf", [](DevicePool& pool) {
        void* first = nullptr;
        {
            DevBuf<char> a(100);
            first = a.p;
            DevBuf<char> b(std::move(a));
            EXPECT(!a.p && b.p == first);
            EXPECT(b.alloc(100) != first);   // the new block is taken before the old one goes back
        }
        EXPECT(cached(pool, 0).size() == 2);
        DevBuf<char> c(100);
        char* kept = c.release();
        EXPECT(!c.p && cached(pool, 0).size() == 1);
        dev_free(kept);
    });

    // a StreamWait below the buffers of its scope: the wait, then the frees in reverse order of declaration
    run_case("wait_before_frees", [](DevicePool&) {
        int stream = 0;
        void *pa = nullptr, *pb = nullptr;
        {
            DevBuf<char> a(100), b(100);
            StreamWait wait{&stream};
            pa = a.p, pb = b.p;
            EXPECT(pa && pb && g_led.events.empty());
        }
        EXPECT(g_led.events == (Events{{'w', &stream}, {'f', pb}, {'f', pa}}));
    });

    // the same on an early return, and as the last member of a struct
    run_case("wait_on_early_return", [](DevicePool&) {
        struct Scratch {
            DevBuf<char> a, b;
            StreamWait wait;
        };
        int stream = 0;
        void* pa = nullptr;
        const auto call = [&](bool fail) {
            Scratch s{{}, {}, StreamWait{&stream}};
            pa = s.a.alloc(100);
            if (fail) return 1;
            s.b.alloc(100);
            return 0;
        };
        EXPECT(call(true) == 1);
        EXPECT(g_led.events == (Events{{'w', &stream}, {'f', pa}}));
    });

    run_case("wait_disarmed", [](DevicePool&) {
        int stream = 0;
        void *pa = nullptr, *pb = nullptr;
        {
            DevBuf<char> a(100), b(100);
            StreamWait wait{&stream};
            pa = a.p, pb = b.p;
            wait.disarm();   // (the success path has just waited itself)
        }
        EXPECT(g_led.events == (Events{{'f', pb}, {'f', pa}}));
    });

    // armed from construction: the wait does not depend on the buffers (nothing is freed here)
    run_case("wait_without_buffers", [](DevicePool&) {
        int stream = 0;
        {
            DevBuf<char> a, b;
            StreamWait wait{&stream};
        }
        EXPECT(g_led.events == (Events{{'w', &stream}}));
    });

    // on = false: no wait until arm()
    run_case("wait_armed_later", [](DevicePool&) {
        int stream = 0;
        void* pa = nullptr;
        {
            DevBuf<char> a;
            StreamWait wait{&stream, false};
        }
        EXPECT(g_led.events.empty());
        {
            DevBuf<char> a;
            StreamWait wait{&stream, false};
            pa = a.alloc(100);
            wait.arm();
        }
        EXPECT(g_led.events == (Events{{'w', &stream}, {'f', pa}}));
    });

    run_case("grow_buf", [](DevicePool& pool) {
        GrowBuf g;
        EXPECT(g.reserve(1000) && g.bytes == 1000);
        void* p = g.p;
        EXPECT(g.reserve(10) == p && g.bytes == 1000);   // never shrinks
        EXPECT(g.reserve(1001) && g.bytes == 1500);      // max(need, have + have / 2)
        g_led.refuse_next_allocs(2);
        EXPECT(g.reserve(100000) == nullptr && g.p == nullptr && g.bytes == 0);
        EXPECT(cached(pool, 0).empty() && g_led.live.empty());   // (the old block was purged for the retry)
        EXPECT(g.reserve(500) && g.p && g.bytes == 500);
        g.free();
        EXPECT(!g.p && g.bytes == 0 && cached(pool, 0).size() == 1);
        g.free();   // twice is harmless
    });

    run_case("sort_scratch_growth", [](DevicePool& pool) {
        SortScratch s;
        EXPECT(s.reserve(1000) && s.cap == 1000);
        uint64_t* was = s.sk_in;
        EXPECT(s.reserve(999) && s.sk_in == was && s.cap == 1000);
        EXPECT(s.reserve(1001) && s.cap == 1500);   // max(n, cap + cap / 2)
        EXPECT(g_led.live[s.sk_in] == pool_round_up(1500 * 8) + DevicePool::SLACK);
        EXPECT(g_led.live[s.pos] == pool_round_up(1500 * 4) + DevicePool::SLACK);
        s.free();
        EXPECT(s.cap == 0 && !s.sk_in && !s.pos);
    });

    // a refusal at each of the nine allocations of a growth
    for (int k = 0; k < 9; ++k) {
        char name[64];
        snprintf(name, sizeof(name), "sort_scratch_refused_%d", k);
        run_case(name, [k](DevicePool& pool) {
            SortScratch s;
            EXPECT(s.reserve(1000));
            // (5000 elements: classes the cached blocks of 1000 cannot serve, so each array is a raw allocation)
            g_led.refuse_alloc = g_led.n_alloc + k;
            g_led.refuse_allocs = 2;   // the allocation and its retry
            EXPECT(!s.reserve(5000));
            EXPECT(g_led.n_alloc == 9 + k + 2);
            void* arrays[9] = {s.sk_in, s.sk_out, s.idx_in, s.idx_out, s.uniq, s.runs, s.offs, s.keep, s.pos};
            for (void* a : arrays) EXPECT(a == nullptr);
            EXPECT(s.cap == 0);
            // all released: whatever the back end still holds lies in the pool
            EXPECT(cached(pool, 0).size() == g_led.live.size() && g_led.live.size() == (size_t)k);
            expect_cache_live(pool, 0);
            const long before = g_led.n_alloc;
            EXPECT(s.reserve(100) && s.cap == 100);   // smaller than before the failure: allocated afresh
            EXPECT(g_led.n_alloc == before + 9);
            void* fresh[9] = {s.sk_in, s.sk_out, s.idx_in, s.idx_out, s.uniq, s.runs, s.offs, s.keep, s.pos};
            EXPECT(std::set<void*>(fresh, fresh + 9).size() == 9 && !std::set<void*>(fresh, fresh + 9).count(nullptr));
            s.free();
        });
    }
    return 0;
}
