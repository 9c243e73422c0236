// Device memory of libctg.so: the caching allocator, the per-device workspace
// with its lock, ctg_trim and the page-locked host arenas.
#include <hip/hip_runtime.h>
#include <cstdlib>
#include <cstring>
#include <sys/mman.h>

#include <algorithm>
#include <map>
#include <mutex>

#include "ctg_internal.h"

namespace ctg {

// ---------------------------------------------------------------------------
// caching device allocator: results and scratch are recycled between calls so
// steady-state calls do no hipMalloc/hipFree
// ---------------------------------------------------------------------------
static std::mutex g_mu;
static std::multimap<size_t, void*> g_pool[64];

int current_device() {
    int d = 0;
    hipGetDevice(&d);
    return d;
}

static size_t round_up(size_t b) {
    size_t r = 256;
    while (r < b) r = r < (1u << 20) ? r * 2 : r + (r >> 2);
    return r;
}

static void* dmalloc(size_t bytes) {
    if (bytes == 0) bytes = 256;
    bytes = round_up(bytes);
    const int d = current_device();
    {
        std::lock_guard<std::mutex> g(g_mu);
        auto& pool = g_pool[d & 63];
        auto it = pool.lower_bound(bytes);
        if (it != pool.end() && it->first <= bytes * 2) {
            void* p = it->second;
            pool.erase(it);
            return p;
        }
    }
    void* p = nullptr;
    if (hipMalloc(&p, bytes + 64) != hipSuccess) {
        // release cached blocks and retry once
        std::lock_guard<std::mutex> g(g_mu);
        for (auto& kv : g_pool[d & 63]) hipFree(kv.second);
        g_pool[d & 63].clear();
        if (hipMalloc(&p, bytes + 64) != hipSuccess) return nullptr;
    }
    return p;
}

static std::map<void*, size_t> g_sizes;
void* dev_alloc(size_t bytes) {
    bytes = round_up(bytes == 0 ? 256 : bytes);
    void* p = dmalloc(bytes);
    if (p) {
        std::lock_guard<std::mutex> g(g_mu);
        g_sizes[p] = bytes;
    }
    return p;
}
void dev_free(void* p) {
    if (!p) return;
    const int d = current_device();
    std::lock_guard<std::mutex> g(g_mu);
    auto it = g_sizes.find(p);
    size_t b = it == g_sizes.end() ? 256 : it->second;
    g_pool[d & 63].emplace(b, p);
}

void ensure(void** p, size_t& have, size_t need) {
    if (need <= have && *p) return;
    if (*p) dev_free(*p);
    size_t n = std::max(need, have + have / 2);
    *p = dev_alloc(n);
    have = *p ? n : 0;
}

static Workspace g_ws[64];
Workspace& ws(int device) { return g_ws[device & 63]; }

static std::recursive_mutex g_dev_mu[64];
std::recursive_mutex& device_mutex(int device) { return g_dev_mu[device & 63]; }

hipError_t ws_init(Workspace& w) {
    if (w.counters) return hipSuccess;
    CTG_TRY(hipMalloc(&w.counters, sizeof(Counters)));
    CTG_TRY(hipHostMalloc(&w.counters_host, sizeof(Counters), hipHostMallocDefault));
    CTG_TRY(hipMalloc(&w.small, 64 * sizeof(unsigned int)));
    CTG_TRY(hipMalloc(&w.bsort, BK_SMALL_WORDS * sizeof(uint32_t)));   // bucket sort scratch
    CTG_TRY(hipMalloc(&w.gsort, GS_SMALL_WORDS * sizeof(uint32_t)));   // group sort scratch
    // the splitters stay in workspace memory: k_mgpu_bounds still reads them
    // after ctg_mgpu_split returns (a pool block freed there could be handed
    // to a call on another stream while that kernel runs)
    CTG_TRY(hipMalloc(&w.mgpu_spl, CTG_MGPU_MAX_WORLD * sizeof(uint64_t)));
    CTG_TRY(hipHostMalloc(&w.small_host, 64 * sizeof(unsigned int), hipHostMallocDefault));
    for (int i = 0; i < 10; ++i) hipEventCreate(&w.ev[i]);
    w.events = true;
    return hipSuccess;
}

void free_records(Workspace& w) {
    ++w.gen;   // a CTG_DEFER_STATS handle must not read the freed records (ctg_trim, fresh sizing)
    dev_free(w.rec.key);
    dev_free(w.rec.sums);
    dev_free(w.rec.hist);
    w.rec = RecordBuf{};
}

hipError_t ensure_records(Workspace& w, int64_t need, int wide) {
    ++w.gen;   // a scan is about to overwrite the records
    if (need <= w.rec.cap && w.rec.key) return hipSuccess;
    free_records(w);
    const int words = wide ? WREC_WORDS : NREC_STRIDE;
    w.rec.key = (uint64_t*)dev_alloc((size_t)need * 8);
    w.rec.sums = wide ? (double2*)dev_alloc((size_t)need * 16) : nullptr;
    w.rec.hist = (uint32_t*)dev_alloc((size_t)need * words * 4);
    if (!w.rec.key || (wide && !w.rec.sums) || !w.rec.hist) return hipErrorOutOfMemory;
    w.rec.cap = need;
    w.rec.rcap = need / NREG;
    return hipSuccess;
}

}  // namespace ctg

using namespace ctg;

extern "C" {

int ctg_trim(void) {
    DevLock dev_lock;
    // hand every cached device block of the current device back to HIP: the
    // workspace (records, sort scratch, staging) and the allocator's pool
    const int d = current_device();
    Workspace& w = ws(d);
    CTG_CHECK(hipDeviceSynchronize());
    free_records(w);   // bumps w.gen: deferred handles made before the trim are refused (CTG_ERR_STALE)
    dev_free(w.sk_in); dev_free(w.sk_out); dev_free(w.idx_in); dev_free(w.idx_out);
    dev_free(w.uniq); dev_free(w.runs); dev_free(w.offs); dev_free(w.keep); dev_free(w.pos);
    w.sk_in = w.sk_out = w.uniq = nullptr;
    w.idx_in = w.idx_out = w.runs = w.offs = w.keep = w.pos = nullptr;
    w.sort_cap = 0;
    dev_free(w.temp);
    w.temp = nullptr;
    w.temp_bytes = 0;
    for (int i = 0; i < 2; ++i) {
        dev_free(w.stage[i]);
        w.stage[i] = nullptr;
        w.stage_bytes[i] = 0;
    }
    std::lock_guard<std::mutex> g(g_mu);
    for (auto& kv : g_pool[d & 63]) {
        g_sizes.erase(kv.second);
        CTG_CHECK(hipFree(kv.second));
    }
    g_pool[d & 63].clear();
    return CTG_OK;
}

// Page-locked staging arenas.  Default: 2 MB-aligned memory marked for
// transparent huge pages, touched and registered with HIP (hipHostRegister),
// so pinning and unpinning walk 2 MB pages instead of 4 KB ones -- a drop-in
// job process pins ~1 GB of arenas and paid ~0.2 s to pin and as much again
// to unpin at exit.  CTG_HOST_ALLOC=hip: hipHostMalloc.
static std::mutex g_host_mu;
static std::map<void*, size_t>& g_host_reg = *new std::map<void*, size_t>;   // registered arenas (never destroyed)

static bool host_alloc_hip() {
    static const bool hip = [] { const char* e = getenv("CTG_HOST_ALLOC"); return e && !strcmp(e, "hip"); }();
    return hip;
}

void* ctg_host_alloc(int64_t bytes) {
    void* p = nullptr;
    if (bytes <= 0) bytes = 64;
    if (!host_alloc_hip() && bytes >= (1 << 20)) {   // (small buffers: hipHostMalloc)
        constexpr size_t HUGE = 2u << 20;
        const size_t cap = ((size_t)bytes + HUGE - 1) / HUGE * HUGE;
        p = aligned_alloc(HUGE, cap);
        if (p) {
            madvise(p, cap, MADV_HUGEPAGE);
            for (size_t o = 0; o < cap; o += 4096) static_cast<volatile char*>(p)[o] = 0;   // fault in as huge pages
            if (hipHostRegister(p, cap, hipHostRegisterDefault) == hipSuccess) {
                std::lock_guard<std::mutex> g(g_host_mu);
                g_host_reg[p] = cap;
                return p;
            }
            free(p);   // registration refused: hipHostMalloc below
            p = nullptr;
        }
    }
    if (hipHostMalloc(&p, (size_t)bytes, hipHostMallocDefault) != hipSuccess) {
        set_error("ctg_host_alloc: hipHostMalloc failed");
        return nullptr;
    }
    return p;
}

void ctg_host_free(void* p) {
    if (!p) return;
    {
        std::lock_guard<std::mutex> g(g_host_mu);
        auto it = g_host_reg.find(p);
        if (it != g_host_reg.end()) {
            g_host_reg.erase(it);
            hipHostUnregister(p);
            free(p);
            return;
        }
    }
    hipHostFree(p);
}

}  // extern "C"
