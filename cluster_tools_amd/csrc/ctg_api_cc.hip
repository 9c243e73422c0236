// C ABI of the thresholded components (include/ctg.h:
// ctg_threshold_components, ctg_merge_assignments) over the kernels of
// ctg_cc.hip.  The host decisions -- the tile grid, the seam threads, the
// segments of the numbering pass, the u32 limit -- are ctg_plan.h's (cc_grid,
// cc_segments, cc_nodes_fit).  No rocPRIM here: the numbering is the three
// launches k_uf_flatten, k_uf_scan, k_uf_write.
#include <hip/hip_runtime.h>

#include "ctg_api.h"
#include "ctg_uf.h"

using namespace ctg;

namespace {

// The pool buffers both calls need for n nodes, and the tail they share: number
// the roots and write the ids.
struct UfBuffers {
    DevBuf<uint32_t> parent, rank, seg, words;
    bool alloc(int64_t n) {
        return parent.alloc((size_t)n * 4) && rank.alloc((size_t)n * 4) &&
               seg.alloc((size_t)cc_segments(n) * 4) && words.alloc(CC_WORDS * 4);
    }
};

int cap_error(const char* who) {
    set_error(std::string(who) + ": a union-find chain passed its step cap (the parent table is corrupt)");
    return CTG_ERR_HIP;
}

}  // namespace

extern "C" {

int ctg_threshold_components(const void* data, int data_kind, const void* mask, const int64_t* shape,
                             const int64_t* begin, const int64_t* end, float threshold, int mode, int normalize,
                             int connectivity, uint64_t* out, int mem, void* stream, uint64_t* n_components) {
    const char* who = "ctg_threshold_components";
    ApiCall c;
    if (n_components) *n_components = 0;
    if (!data || !shape || !out || !n_components) {
        set_error("ctg_threshold_components: null argument");
        return CTG_ERR_ARG;
    }
    if (data_kind != CTG_DATA_F32 && data_kind != CTG_DATA_U8) {
        set_error("ctg_threshold_components: data_kind must be CTG_DATA_F32 or CTG_DATA_U8");
        return CTG_ERR_ARG;
    }
    if (mode != CTG_CC_GREATER && mode != CTG_CC_LESS && mode != CTG_CC_EQUAL) {
        set_error("ctg_threshold_components: mode must be CTG_CC_GREATER, CTG_CC_LESS or CTG_CC_EQUAL");
        return CTG_ERR_ARG;
    }
    if (connectivity < 1 || connectivity > 3) {
        set_error("ctg_threshold_components: connectivity must be 1, 2 or 3");
        return CTG_ERR_ARG;
    }
    if (!mem_ok(who, mem)) return CTG_ERR_ARG;
    DenseCall D{who, mem};
    int rc = D.open(shape, begin, end, CC_MAX_NODES);
    if (rc) return rc;
    const int64_t V = D.V;
    if (V == 0) return CTG_OK;
    if ((rc = c.begin(stream)) != CTG_OK) return rc;
    hipStream_t s = D.s = c.s;
    const CcGrid G = cc_grid(D.n);
    DevInput<char> dd;
    DevInput<uint8_t> dm;
    UfBuffers b;
    DenseOut<uint64_t> o;
    StreamWait wait{s};
    if ((rc = D.in(dd, data, data_kind == CTG_DATA_U8 ? 1 : 4)) != CTG_OK) return rc;
    if (mask && (rc = D.in(dm, mask, 1)) != CTG_OK) return rc;
    if (!b.alloc(V)) return hip_status(hipErrorOutOfMemory, who);
    if ((rc = D.out(o, out, 8)) != CTG_OK) return rc;
    uint32_t h[CC_WORDS] = {};
    h[CC_W_MIN] = 0xFFFFFFFFu;   // (f2ord words: the minimum starts at the top, the maximum at 0)
    CTG_CHECK(hipMemcpyAsync(b.words.p, h, sizeof(h), hipMemcpyHostToDevice, s));
    CcArgs A{};
    A.data = dd.p;
    A.mask = mask ? dm.p : nullptr;
    A.box = D.vol;
    for (int k = 0; k < 3; ++k) A.nt[k] = (uint32_t)G.nt[k];
    A.threshold = threshold;
    A.mode = mode;
    A.words = b.words;
    A.parent = b.parent;
    Ev ev{c.w(), s};
    ev.mark(0);
    if (normalize) CTG_CHECK(launch_cc_range(A, data_kind, s));
    ev.mark(1);
    CTG_CHECK(launch_cc_tile(A, G, data_kind, normalize, connectivity, s));
    ev.mark(2);
    CTG_CHECK(launch_cc_seams(A, G, connectivity, s));
    ev.mark(3);
    CTG_CHECK(launch_uf_flatten(b.parent, V, b.rank, b.seg, b.words, s));
    ev.mark(4);
    CTG_CHECK(launch_uf_scan(b.seg, G.segs, b.words, s));
    ev.mark(5);
    CTG_CHECK(launch_uf_write(b.parent, b.rank, b.seg, V, 1, o.d, s));
    ev.mark(6);
    CTG_CHECK(o.copy_back(s));
    if ((rc = read_words(b.words, sizeof(h), s, h)) != CTG_OK) return rc;
    wait.disarm();
    if (c.w().profiling && (rc = read_phase_times(c.w(), s)) != CTG_OK) return rc;
    if (h[CC_W_ERR] & CC_ERR_CAP) return cap_error(who);
    *n_components = h[CC_W_TOTAL];
    return CTG_OK;
}

int ctg_merge_assignments(const uint64_t* pairs, int64_t n, uint64_t n_labels, uint64_t* table, int mem,
                          void* stream, uint64_t* max_id) {
    const char* who = "ctg_merge_assignments";
    ApiCall c;
    if (max_id) *max_id = 0;
    if (!max_id || n < 0 || (n > 0 && !pairs) || (n_labels > 0 && !table)) {
        set_error("ctg_merge_assignments: bad arguments");
        return CTG_ERR_ARG;
    }
    if (!mem_ok(who, mem)) return CTG_ERR_ARG;
    if (!cc_nodes_fit(n_labels) || n >= (1ll << 38)) {
        set_error("ctg_merge_assignments: 2^32 labels or more, or 2^38 pairs or more");
        return CTG_ERR_UNSUPPORTED;
    }
    if (n_labels == 0) {
        if (n == 0) return CTG_OK;
        set_error("ctg_merge_assignments: pairs without labels");
        return CTG_ERR_ARG;
    }
    int rc = c.begin(stream);
    if (rc) return rc;
    hipStream_t s = c.s;
    const int64_t N = (int64_t)n_labels;
    DevInput<uint64_t> dp;
    UfBuffers b;
    DenseOut<uint64_t> o;
    StreamWait wait{s};
    if ((rc = dp.put(pairs, (size_t)n * 16, mem, s, who)) != CTG_OK) return rc;
    if (n > 0 && ((uintptr_t)dp.p & 15u)) {
        set_error("ctg_merge_assignments: pairs must be aligned to 16 bytes");
        return CTG_ERR_ARG;
    }
    if (!b.alloc(N)) return hip_status(hipErrorOutOfMemory, who);
    uint32_t h[CC_WORDS] = {};
    CTG_CHECK(hipMemsetAsync(b.words.p, 0, CC_WORDS * 4, s));
    Ev ev{c.w(), s};
    ev.mark(0);
    CTG_CHECK(launch_uf_init(b.parent, N, s));
    ev.mark(1);
    CTG_CHECK(launch_uf_pairs(dp, n, b.parent, (uint32_t)n_labels, b.words, s));
    ev.mark(2);
    // the pairs are checked before the table is touched
    if ((rc = read_words(b.words, sizeof(h), s, h)) != CTG_OK) return rc;
    if (h[CC_W_ERR] & CC_ERR_PAIR) {
        set_error("ctg_merge_assignments: a pair member is 0 or not below n_labels (" + std::to_string(n_labels) + ")");
        return CTG_ERR_ARG;
    }
    if (h[CC_W_ERR] & CC_ERR_CAP) return cap_error(who);
    if ((rc = hip_status(o.open(table, (size_t)N * 8, mem, false, s), who)) != CTG_OK) return rc;
    CTG_CHECK(launch_uf_flatten(b.parent, N, b.rank, b.seg, b.words, s));
    ev.mark(3);
    CTG_CHECK(launch_uf_scan(b.seg, cc_segments(N), b.words, s));
    ev.mark(4);
    // label 0 is a set of its own and the smallest root: its rank is 0, every other set's is 1 + its rank among the rest
    CTG_CHECK(launch_uf_write(b.parent, b.rank, b.seg, N, 0, o.d, s));
    ev.mark(5);
    ev.mark(6);
    CTG_CHECK(o.copy_back(s));
    if ((rc = read_words(b.words, sizeof(h), s, h)) != CTG_OK) return rc;
    wait.disarm();
    if (c.w().profiling && (rc = read_phase_times(c.w(), s)) != CTG_OK) return rc;
    if (h[CC_W_ERR] & CC_ERR_CAP) return cap_error(who);
    *max_id = (uint64_t)h[CC_W_TOTAL] - 1;
    return CTG_OK;
}

}  // extern "C"
