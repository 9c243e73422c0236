// Device memory of libctg.so: the caching allocator, the per-device workspace
// with its lock, ctg_trim and the page-locked host arenas.
#include <hip/hip_runtime.h>
#include <cstdlib>
#include <cstring>
#include <sys/mman.h>

#include <map>
#include <mutex>

#include "ctg_internal.h"
#include "ctg_pool.h"

namespace ctg {

// ---------------------------------------------------------------------------
// the caching device allocator (ctg_pool.h) over hipMalloc / hipFree
// ---------------------------------------------------------------------------
static DevicePool g_pool([](void** p, size_t bytes) -> int { return hipMalloc(p, bytes); },
                         [](void* p) -> int { return hipFree(p); });

int current_device() {
    int d = 0;
    hipGetDevice(&d);
    return d;
}

void* dev_alloc(size_t bytes) { return g_pool.alloc(current_device(), bytes); }
void dev_free(void* p) { g_pool.free(p); }
void stream_wait(void* stream) { hipStreamSynchronize((hipStream_t)stream); }

static Workspace g_ws[64];
Workspace& ws(int device) { return g_ws[device & 63]; }

static std::recursive_mutex g_dev_mu[64];
std::recursive_mutex& device_mutex(int device) { return g_dev_mu[device & 63]; }

static hipError_t ws_create(Workspace& w) {
    CTG_TRY(hipMalloc(&w.counters, sizeof(Counters)));
    CTG_TRY(hipHostMalloc(&w.counters_host, sizeof(Counters), hipHostMallocDefault));
    CTG_TRY(hipMalloc(&w.small, SMALL_WORDS * sizeof(unsigned int)));
    CTG_TRY(hipMalloc(&w.bsort, BK_SMALL_WORDS * sizeof(uint32_t)));   // bucket sort scratch
    CTG_TRY(hipMalloc(&w.gsort, GS_SMALL_WORDS * sizeof(uint32_t)));   // group sort scratch
    // the splitters stay in workspace memory: k_mgpu_bounds still reads them
    // after ctg_mgpu_split returns (a pool block freed there could be handed
    // to a call on another stream while that kernel runs)
    CTG_TRY(hipMalloc(&w.mgpu_spl, CTG_MGPU_MAX_WORLD * sizeof(uint64_t)));
    CTG_TRY(hipHostMalloc(&w.small_host, SMALL_WORDS * sizeof(unsigned int), hipHostMallocDefault));
    for (hipEvent_t& ev : w.ev) CTG_TRY(hipEventCreate(&ev));
    CTG_TRY(hipStreamCreateWithFlags(&w.copy_stream, hipStreamNonBlocking));
    return hipSuccess;
}

// All or nothing: ready only once every member exists; a failed attempt
// releases what it made, so the next call starts over.
hipError_t ws_init(Workspace& w) {
    if (w.ready) return hipSuccess;
    const hipError_t e = ws_create(w);
    w.ready = e == hipSuccess;
    if (w.ready) return e;
    auto drop = [](auto*& p, auto release) {
        if (p) release(p);
        p = nullptr;
    };
    drop(w.counters, hipFree);
    drop(w.counters_host, hipHostFree);
    drop(w.small, hipFree);
    drop(w.bsort, hipFree);
    drop(w.gsort, hipFree);
    drop(w.mgpu_spl, hipFree);
    drop(w.small_host, hipHostFree);
    for (hipEvent_t& ev : w.ev) drop(ev, hipEventDestroy);
    drop(w.copy_stream, hipStreamDestroy);
    return e;
}

void free_records(Workspace& w) {
    ++w.gen;   // a CTG_DEFER_STATS handle must not read the freed records (ctg_trim, fresh sizing)
    dev_free(w.rec.key);
    dev_free(w.rec.sums);
    dev_free(w.rec.hist);
    w.rec = RecordBuf{};
}

// all or nothing, like the sort scratch: cap > 0 exactly when the buffers exist
hipError_t ensure_records(Workspace& w, int64_t need, int wide) {
    ++w.gen;   // a scan is about to overwrite the records
    if (need <= w.rec.cap && w.rec.key) return hipSuccess;
    free_records(w);
    const int words = wide ? WREC_WORDS : NREC_STRIDE;
    w.rec.key = (uint64_t*)dev_alloc((size_t)need * 8);
    w.rec.sums = wide ? (double2*)dev_alloc((size_t)need * 16) : nullptr;
    w.rec.hist = (uint32_t*)dev_alloc((size_t)need * words * 4);
    if (!w.rec.key || (wide && !w.rec.sums) || !w.rec.hist) {
        free_records(w);
        return hipErrorOutOfMemory;
    }
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
    w.sort.free();
    w.temp.free();
    for (GrowBuf& st : w.stage) st.free();
    CTG_CHECK((hipError_t)g_pool.purge(d));   // hipFree of every cached block; the first failure is reported
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
