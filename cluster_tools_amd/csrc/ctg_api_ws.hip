// C ABI of the seeded watershed (include/ctg.h: ctg_seeded_watershed) over the
// kernels of ctg_ws.hip.  The host decisions -- the buffers and the grid, the
// round cap, the chase launches -- are ctg_plan.h's (ws_plan, ws_round_cap,
// WS_CHASE_LAUNCHES).  The size filter counts with the morphology's tile-table
// scan (ctg_morphology on the flood's own output), one table per domain.
#include <hip/hip_runtime.h>

#include <vector>

#include "ctg_api.h"
#include "ctg_ws.h"

using namespace ctg;

namespace {

// the call's scratch
struct WsScratch {
    DevBuf<uint32_t> parent, key, pick;
    DevBuf<unsigned long long> best, words;
    bool alloc(const WsPlan& P) {
        return parent.alloc((size_t)P.parent_bytes) && key.alloc((size_t)P.key_bytes) &&
               pick.alloc((size_t)P.pick_bytes) && best.alloc((size_t)P.best_bytes) && words.alloc(WS_WORDS * 8);
    }
};

// Phase times of a profiled call.  The rounds repeat their phases and the host
// waits between them, so seven marks do not do: a mark before and one after
// every group of launches, summed per phase afterwards.
enum WsPhase : int { WS_T_IDLE = -1, WS_T_INIT = 0, WS_T_PICK = 1, WS_T_CHASE = 2, WS_T_FILTER = 3, WS_T_WRITE = 4 };
struct WsClock {
    bool on;
    hipStream_t s;
    std::vector<std::pair<int, hipEvent_t>> marks;   // (the phase that ends here, the event)
    void mark(int phase) {
        if (!on) return;
        hipEvent_t e = nullptr;
        if (hipEventCreate(&e) != hipSuccess) return;
        hipEventRecord(e, s);
        marks.emplace_back(phase, e);
    }
    // after the stream was waited for
    void read(double* ms) {
        for (int i = 0; i < 8; ++i) ms[i] = 0.0;
        float t = 0.f;
        for (size_t k = 1; k < marks.size(); ++k)
            if (marks[k].first >= 0 && hipEventElapsedTime(&t, marks[k - 1].second, marks[k].second) == hipSuccess)
                ms[marks[k].first] += t;
        if (marks.size() > 1 && hipEventElapsedTime(&t, marks.front().second, marks.back().second) == hipSuccess)
            ms[6] = t;
    }
    ~WsClock() {
        for (auto& m : marks) hipEventDestroy(m.second);
    }
};

int read_words(const WsArgs& A, hipStream_t s, unsigned long long* h) {
    return ctg::read_words(A.words, WS_WORDS * 8, s, h);
}

int zero_words(const WsArgs& A, int first, int n, hipStream_t s) {
    CTG_CHECK(hipMemsetAsync(A.words + first, 0, (size_t)n * 8, s));
    return CTG_OK;
}

int cap_error(const char* who, const char* what) {
    set_error(std::string(who) + ": " + what + " (the forest is corrupt)");
    return CTG_ERR_HIP;
}

// One flood of A into out.  with_keys: the first flood of a call, which reads
// the heights; *nan is then set, and nothing written, where they hold a NaN.
// h: the call's words as last read.
int flood(const char* who, const WsArgs& A, int with_keys, uint64_t* out, WsClock& clk, hipStream_t s,
          unsigned long long* h, uint64_t* rounds, bool* nan) {
    const int64_t V = (int64_t)A.box.n[0] * A.box.n[1] * A.box.n[2];
    int rc;
    *rounds = 0;
    if ((rc = zero_words(A, WS_W_SEEDED, 3, s)) != CTG_OK) return rc;
    if ((rc = zero_words(A, WS_W_MAX, 2, s)) != CTG_OK) return rc;
    clk.mark(WS_T_IDLE);
    CTG_CHECK(launch_ws_init(A, with_keys, s));
    clk.mark(WS_T_INIT);
    if ((rc = read_words(A, s, h)) != CTG_OK) return rc;
    if (with_keys && h[WS_W_NAN]) {
        *nan = true;
        return CTG_OK;
    }
    const int64_t U = V - (int64_t)h[WS_W_SEEDED];
    if (U == V) {   // no seed: every voxel stays 0
        CTG_CHECK(hipMemsetAsync(out, 0, (size_t)V * 8, s));
        h[WS_W_MAX] = 0;
        h[WS_W_ZERO] = (unsigned long long)V;
        return CTG_OK;
    }
    const int cap = ws_round_cap(U);
    bool finished = U == 0;
    for (int round = 0; round < cap && !finished; ++round) {
        if ((rc = zero_words(A, WS_W_HOOKS, 2, s)) != CTG_OK) return rc;
        clk.mark(WS_T_IDLE);
        CTG_CHECK(launch_ws_pick(A, s));
        clk.mark(WS_T_PICK);
        if ((rc = read_words(A, s, h)) != CTG_OK) return rc;
        ++*rounds;
        if (h[WS_W_ERR]) return cap_error(who, "a root picked an edge outside the box");
        if (h[WS_W_HOOKS] == 0) {
            finished = true;
            break;
        }
        clk.mark(WS_T_IDLE);
        CTG_CHECK(launch_ws_apply(A, s));
        for (int k = 0;; ++k) {
            if (k == WS_CHASE_LAUNCHES) return cap_error(who, "a chain passed its step cap");
            if (k > 0 && (rc = zero_words(A, WS_W_SHORT, 1, s)) != CTG_OK) return rc;
            CTG_CHECK(launch_ws_chase(A, s));
            clk.mark(WS_T_CHASE);
            if ((rc = read_words(A, s, h)) != CTG_OK) return rc;
            if (!h[WS_W_SHORT]) break;
            clk.mark(WS_T_IDLE);
        }
    }
    if (!finished) return cap_error(who, "the rounds passed their cap");
    clk.mark(WS_T_IDLE);
    CTG_CHECK(launch_ws_write(A, out, s));
    clk.mark(WS_T_WRITE);
    return read_words(A, s, h);
}

}  // namespace

extern "C" {

int ctg_seeded_watershed(const float* hmap, const void* seeds, int seed_bits, const int64_t* shape,
                         const int64_t* begin, const int64_t* end, int flags, uint64_t size_filter, uint64_t* out,
                         int mem, void* stream, uint64_t* info) {
    const char* who = "ctg_seeded_watershed";
    ApiCall c;
    if (info) info[0] = info[1] = info[2] = info[3] = 0;
    if (!hmap || !seeds || !shape || !out) {
        set_error("ctg_seeded_watershed: null argument");
        return CTG_ERR_ARG;
    }
    if (seed_bits != 32 && seed_bits != 64) {
        set_error("ctg_seeded_watershed: seed_bits must be 32 or 64");
        return CTG_ERR_ARG;
    }
    if (flags & ~CTG_WS_2D) {
        set_error("ctg_seeded_watershed: unknown flag");
        return CTG_ERR_ARG;
    }
    if (!mem_ok(who, mem)) return CTG_ERR_ARG;
    DenseCall D{who, mem};
    int rc = D.open(shape, begin, end, 0);
    if (rc) return rc;
    const int64_t V = D.V, *n = D.n;
    if (V > WS_MAX_VOXELS) {
        set_error("ctg_seeded_watershed: a box holds at most 2^30 voxels");
        return CTG_ERR_ARG;
    }
    if ((const void*)out == seeds && (seed_bits != 64 || V != (int64_t)D.elems)) {
        set_error("ctg_seeded_watershed: out may be the seeds only where they are 64-bit and the box is the whole array");
        return CTG_ERR_ARG;
    }
    if (V == 0) return CTG_OK;
    if ((rc = c.begin(stream)) != CTG_OK) return rc;
    hipStream_t s = D.s = c.s;
    const bool two_d = (flags & CTG_WS_2D) != 0;
    const WsPlan P = ws_plan(n, two_d);
    DevInput<float> dh;
    DevInput<char> dsd;
    DenseOut<uint64_t> o;
    WsScratch b;
    StreamWait wait{s};
    if ((rc = D.in(dh, hmap, 4)) != CTG_OK) return rc;
    if ((rc = D.in(dsd, seeds, (size_t)(seed_bits / 8))) != CTG_OK) return rc;
    if (!b.alloc(P)) return hip_status(hipErrorOutOfMemory, who);
    if ((rc = D.out(o, out, 8)) != CTG_OK) return rc;
    CTG_CHECK(hipMemsetAsync(b.words.p, 0, WS_WORDS * 8, s));
    WsArgs A{};
    A.hmap = dh.p;
    A.seeds = dsd.p;
    A.seed_bits = seed_bits;
    A.box = D.vol;
    A.two_d = two_d;
    A.parent = b.parent;
    A.key = b.key;
    A.best = b.best;
    A.pick = b.pick;
    A.words = b.words;
    WsClock clk{c.w().profiling != 0, s, {}};
    unsigned long long h[WS_WORDS] = {};
    uint64_t rounds = 0;
    bool nan = false;
    if ((rc = flood(who, A, 1, o.d, clk, s, h, &rounds, &nan)) != CTG_OK) return rc;
    if (nan) {
        set_error("ctg_seeded_watershed: the heights of the box hold a NaN");
        return CTG_ERR_ARG;
    }
    // a written label has a voxel: a limit of 0 or 1 drops nothing
    if (size_filter > 1 && h[WS_W_MAX] != 0) {
        clk.mark(WS_T_IDLE);
        const int64_t slab = V / P.slices;
        for (int64_t d = 0; d < P.slices; ++d) {
            const int64_t db[3] = {two_d ? d : 0, 0, 0}, de[3] = {two_d ? d + 1 : n[0], n[1], n[2]};
            ResultPtr r;
            rc = nested(r, [&](ctg_result** t) {
                return ctg_morphology(o.d, 64, n, db, de, nullptr, CTG_MEM_DEVICE, stream, t);
            });
            if (rc) return rc;
            CTG_CHECK(launch_ws_filter(o.d + d * slab, slab, r->nodes, r->moments, r->n_nodes, size_filter, b.words, s));
        }
        clk.mark(WS_T_FILTER);
        if ((rc = read_words(A, s, h)) != CTG_OK) return rc;
        if (h[WS_W_DROPPED]) {
            // the survivors, whole, are the seeds of the second flood
            A.seeds = o.d;
            A.seed_bits = 64;
            A.box = vol_box(n, call_box(n, nullptr, nullptr, 0));
            if ((rc = flood(who, A, 0, o.d, clk, s, h, &rounds, &nan)) != CTG_OK) return rc;
        }
    }
    CTG_CHECK(o.copy_back(s));
    CTG_CHECK(hipStreamSynchronize(s));
    if (c.w().profiling) clk.read(c.w().last_ms);
    if (info) {
        info[0] = h[WS_W_MAX];
        info[1] = h[WS_W_ZERO];
        info[2] = rounds;
        info[3] = h[WS_W_DROPPED];
    }
    return CTG_OK;
}

}  // extern "C"
