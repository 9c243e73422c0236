// C ABI of libctg.so (include/ctg.h): the multi-GPU exchange -- ctg_mgpu_slab,
// ctg_mgpu_sample, ctg_mgpu_split, ctg_mgpu_pack, ctg_mgpu_merge.  Each entry
// point is a sequence of the steps below.  What a step decides on the host is
// a pure function of ctg_plan.h (slab_range, exchange_plan: the count matrix
// is read there and nowhere else); the kernels and their launchers are
// ctg_mgpu.hip.  No kernel and no rocPRIM here.
//
// Lifetime rule (ctg_api_scan.hip): the merge's scratch is read by queued
// kernels, so MergeScratch synchronises the stream before it returns its
// buffers to the pool, on every return path.
#include <hip/hip_runtime.h>

#include "ctg_api.h"

using namespace ctg;

// ---------------------------------------------------------------------------
// argument checks
// ---------------------------------------------------------------------------
static bool mgpu_args(const ctg_result* r, int world, const char* who) {
    if (!r || world <= 0 || world > CTG_MGPU_MAX_WORLD) {
        set_error(std::string(who) + ": bad arguments (world size must be 1.." +
                  std::to_string(CTG_MGPU_MAX_WORLD) + ")");
        return false;
    }
    return true;
}

// What pack and merge check alike once the plan is known: the counts cover the
// rank's table and, with words to move, there is a buffer for them (no_buffer,
// with the call's own message) and the deferred records are still the call's.
static int exchange_args(const char* who, const ctg_result* local, const ExchangePlan& p, int64_t words,
                         bool no_buffer, const char* no_buffer_msg) {
    if (p.rows != local->n_edges || p.nodes != local->n_nodes) {
        set_error(std::string(who) + ": counts do not cover this rank's table");
        return CTG_ERR_ARG;
    }
    if (words > 0 && no_buffer) {
        set_error(std::string(who) + ": " + no_buffer_msg);
        return CTG_ERR_ARG;
    }
    if (words > 0 && local->defer.on && local->defer.gen != ws(local->device).gen) {
        set_error(std::string(who) + ": the CTG_DEFER_STATS table's records were overwritten by a later call");
        return CTG_ERR_STALE;
    }
    return CTG_OK;
}

// ---------------------------------------------------------------------------
// the steps of ctg_mgpu_merge
// ---------------------------------------------------------------------------
static int merge_status(hipError_t e) { return hip_status(e, "ctg_mgpu_merge"); }

// the shard's nodes: the own range of the local table in place (the shard
// takes the table over), or the own range and every received id, unique
static int shard_nodes(ApiCall& c, ctg_result* L, const int64_t* recv, const ExchangePlan& p) {
    ctg_result* r = c.r.get();
    if (p.recv.nodes() == 0) {
        r->nodes = L->nodes + p.n_lo;
        r->n_nodes = p.n_cnt;
        r->owned.push_back(std::exchange(L->nodes, nullptr));
        return CTG_OK;
    }
    const int64_t total = p.n_cnt + p.recv.nodes();
    DevBuf<uint64_t> list(std::max<size_t>((size_t)total * 8, 16));
    if (!list) return merge_status(hipErrorOutOfMemory);
    int rc = merge_status(mgpu_node_list(p.recv, recv, L->nodes + p.n_lo, p.n_cnt, list, c.s));
    if (rc) return rc;
    ResultPtr U;   // (a failure's status and message pass through)
    rc = nested(U, [&](ctg_result** u) { return ctg_unique_values(list, total, CTG_MEM_DEVICE, c.s, u); });
    if (rc) return rc;
    r->nodes = U->nodes;
    r->n_nodes = U->n_nodes;
    r->owned.push_back(std::exchange(U->nodes, nullptr));
    return CTG_OK;
}

// nothing received, nothing to drop: the own range of the local table IS the
// shard's edges and features (no kernel, no copy)
static void shard_own_range(ctg_result* L, const ExchangePlan& p, ctg_result* r) {
    r->edges = L->edges + 2 * p.e_lo;
    r->features = L->features ? L->features + N_FEATURES * p.e_lo : nullptr;
    r->n_edges = p.e_cnt;
    r->owned.push_back(std::exchange(L->edges, nullptr));
    r->owned.push_back(std::exchange(L->features, nullptr));
}

// The merge's scratch: per received row (M), per own row (e_cnt) and per slot
// of the merged order (e_cnt + M).  All or nothing.
struct MergeScratch {
    hipStream_t s;
    DevBuf<uint32_t> order, head, rid, run0;       // M (run0: M + 1): sorted order and runs
    DevBuf<uint64_t> skeys, mkeys;                 // 2M
    DevBuf<double> mfeats;                         // 10M
    DevBuf<uint32_t> mkeep, mnew, nrank;           // M
    DevBuf<int64_t> mins;                          // M
    DevBuf<uint32_t> touched;                      // e_cnt
    DevBuf<uint32_t> keep, fpos;                   // e_cnt + M
    size_t m = 0, own = 0, slots = 0;              // the three lengths, at least 1
    StreamWait wait{s, false};                     // armed once alloc() ran
    explicit MergeScratch(hipStream_t stream) : s(stream) {}
    bool alloc(const ExchangePlan& p) {
        wait.arm();
        m = (size_t)std::max<int64_t>(p.recv.rows(), 1);
        own = (size_t)std::max<int64_t>(p.e_cnt, 1);
        slots = (size_t)std::max<int64_t>(p.e_cnt + p.recv.rows(), 1);
        const auto words = [](size_t n) { return std::max<size_t>(n * 4, 16); };
        return order.alloc(words(m)) && head.alloc(words(m)) && rid.alloc(words(m)) && run0.alloc(words(m + 1)) &&
               skeys.alloc(m * 16) && mkeys.alloc(m * 16) && mfeats.alloc(m * N_FEATURES * 8) &&
               mkeep.alloc(words(m)) && mnew.alloc(words(m)) && nrank.alloc(words(m)) && mins.alloc(words(2 * m)) &&
               touched.alloc(words(own)) && keep.alloc(words(slots)) && fpos.alloc(words(slots));
    }
};

static MergeIO merge_io(const ctg_result* L, const int64_t* recv, const ExchangePlan& p, const MergeScratch& m,
                        const uint32_t* nK, double hist_lo, double hist_hi) {
    MergeIO io{};
    io.own_edges = L->edges + 2 * p.e_lo;
    io.own_feats = L->features + N_FEATURES * p.e_lo;
    io.own_wide = L->stats ? L->stats + WREC_WORDS * p.e_lo : nullptr;
    io.own_sums = L->stat_sums ? L->stat_sums + p.e_lo : nullptr;
    if (!L->stats) io.defer = L->defer;
    io.own_row0 = p.e_lo;
    io.n_own = p.e_cnt;
    io.recv = reinterpret_cast<const uint64_t*>(recv);
    io.order = m.order;
    io.skeys = m.skeys;
    io.run0 = m.run0;
    io.nK = nK;
    io.mkeys = m.mkeys;
    io.mfeats = m.mfeats;
    io.mkeep = m.mkeep;
    io.mnew = m.mnew;
    io.mins = m.mins;
    io.touched = m.touched;
    io.partial_adj = L->partial_adj;
    io.scale = (double)NBINS / (hist_hi - hist_lo);
    io.offset = hist_lo;
    return io;
}

// the kept rows of the merged order into the shard's own tables, and their number
static int assemble(ApiCall& c, const MergeIO& io, const MergeScratch& m, int64_t n_slots, MergeCounts* mc) {
    ctg_result* r = c.r.get();
    r->edges = (uint64_t*)dev_alloc(m.slots * 16);
    r->features = (double*)dev_alloc(m.slots * N_FEATURES * 8);
    r->owned.push_back(r->edges);
    r->owned.push_back(r->features);
    if (!r->edges || !r->features) return merge_status(hipErrorOutOfMemory);
    int rc = merge_status(mgpu_scatter(io, m.nrank, m.keep, m.fpos, n_slots, r->edges, r->features, &mc->rows, c.s));
    if (rc) return rc;
    uint32_t* rows_host = &reinterpret_cast<MergeCounts*>(c.w().small_host + SLOT_MERGE)->rows;
    if ((rc = merge_status(hipMemcpyAsync(rows_host, &mc->rows, 4, hipMemcpyDeviceToHost, c.s))) != CTG_OK) return rc;
    if ((rc = merge_status(hipStreamSynchronize(c.s))) != CTG_OK) return rc;
    r->n_edges = n_slots ? *rows_host : 0;
    return CTG_OK;
}

// The shard's edges and features where rows were received (or keys may have to
// be dropped): order the received rows, number their runs, combine every run
// with the own row of its key, give every row its slot, assemble.
static int merge_rows(ApiCall& c, ctg_result* L, const int64_t* recv, const ExchangePlan& p, double hist_lo,
                      double hist_hi) {
    // needs a CTG_KEEP_STATS partial table (rows, or CTG_DEFER_STATS records);
    // reported as HIP's "invalid argument" since the first release
    if ((!L->stats && !L->defer.on) || !L->features) return merge_status(hipErrorInvalidValue);
    if (p.too_large()) {
        set_error("ctg_mgpu_merge: more than 2^32 rows in one shard (split the slab over more ranks)");
        return CTG_ERR_UNSUPPORTED;
    }
    Workspace& w = c.w();
    hipStream_t s = c.s;
    const ExchangeSegs& S = p.recv;
    const int64_t M = S.rows(), n_slots = p.e_cnt + M;
    MergeScratch m(s);
    if (!m.alloc(p)) return merge_status(hipErrorOutOfMemory);
    MergeCounts* mc = reinterpret_cast<MergeCounts*>(w.small + SLOT_MERGE);
    const MergeIO io = merge_io(L, recv, p, m, &mc->keys, hist_lo, hist_hi);
    int rc = merge_status(hipMemsetAsync(mc, 0, sizeof(MergeCounts), s));
    if (!rc) rc = merge_status(hipMemsetAsync(m.mnew, 0, m.m * 4, s));
    if (!rc) rc = merge_status(hipMemsetAsync(m.touched, 0, m.own * 4, s));
    if (!rc && M > 0) {
        rc = merge_status(mgpu_order(S, recv, m.order, m.skeys, s));
        if (!rc) rc = merge_status(mgpu_runs(w, M, m.skeys, m.head, m.rid, m.run0, &mc->keys, s));
        if (!rc) rc = merge_status(mgpu_combine(w, S, io, m.nrank, s));
    }
    if (!rc) rc = merge_status(mgpu_slots(w, io, m.nrank, n_slots, m.keep, m.fpos, s));
    return rc ? rc : assemble(c, io, m, n_slots, mc);
}

// ---------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------
extern "C" {

int ctg_mgpu_slab(int64_t Z, int world_size, int rank, const int64_t* offsets, int n_channels, int64_t* out) {
    if (Z <= 0 || world_size <= 0 || rank < 0 || rank >= world_size || !out || n_channels < 0 ||
        (n_channels > 0 && !offsets)) {
        set_error("ctg_mgpu_slab: invalid arguments");
        return CTG_ERR_ARG;
    }
    if (world_size > Z) {
        set_error("ctg_mgpu_slab: more ranks than z planes");
        return CTG_ERR_ARG;
    }
    const SlabRange r = slab_range(Z, world_size, rank, offsets, n_channels);
    if (r.up > 0 && world_size > 1) {
        set_error("ctg_mgpu_slab: positive z offsets need an upper halo, which the z-slab layout does not have");
        return CTG_ERR_UNSUPPORTED;
    }
    out[0] = r.read_begin;
    out[1] = r.z0;
    out[2] = r.z1;
    return CTG_OK;
}

// (sample and pack use no workspace member; begin() finds the workspace the
// local call left ready)
int ctg_mgpu_sample(const ctg_result* local, int64_t* meta, void* stream) {
    ApiCall c;
    if (!mgpu_args(local, 1, "ctg_mgpu_sample") || !meta) return CTG_ERR_ARG;
    if (int rc = c.begin(stream)) return rc;
    CTG_CHECK(mgpu_sample(local->edges, local->n_edges, meta, c.s));
    return CTG_OK;
}

int ctg_mgpu_split(const ctg_result* local, const int64_t* meta_all, int world_size, int64_t* counts, void* stream) {
    ApiCall c;
    if (!mgpu_args(local, world_size, "ctg_mgpu_split") || !meta_all || !counts) return CTG_ERR_ARG;
    if (int rc = c.begin(stream)) return rc;
    Workspace& w = c.w();
    // one splitter buffer per device: a split on another stream must not
    // overwrite it while an earlier split's k_mgpu_bounds still reads it
    if (w.mgpu_spl_ev) CTG_CHECK(hipStreamWaitEvent(c.s, w.mgpu_spl_ev, 0));
    else CTG_CHECK(hipEventCreateWithFlags(&w.mgpu_spl_ev, hipEventDisableTiming));
    CTG_CHECK(mgpu_split(local->edges, local->n_edges, local->nodes, local->n_nodes, meta_all, world_size,
                         w.mgpu_spl, counts, c.s));
    CTG_CHECK(hipEventRecord(w.mgpu_spl_ev, c.s));
    return CTG_OK;
}

int ctg_mgpu_pack(const ctg_result* local, const int64_t* counts_all, int world_size, int rank, int64_t* send,
                  void* stream) {
    ApiCall c;
    if (!mgpu_args(local, world_size, "ctg_mgpu_pack") || !counts_all || rank < 0 || rank >= world_size)
        return CTG_ERR_ARG;
    const ExchangePlan p = exchange_plan(counts_all, world_size, rank);
    int rc = exchange_args("ctg_mgpu_pack", local, p, p.send.words(),
                           !send || (!(local->stats && local->stat_sums) && !local->defer.on),
                           "rows to send need a CTG_KEEP_STATS table and a send buffer");
    if (rc || (rc = c.begin(stream)) != CTG_OK) return rc;
    CTG_CHECK(mgpu_pack(local, p.send, send, c.s));
    // a CTG_DEFER_STATS table is packed from the workspace's records, which the
    // next scan on any stream overwrites: that pack is waited for
    if (local->defer.on) CTG_CHECK(hipStreamSynchronize(c.s));
    return CTG_OK;
}

int ctg_mgpu_merge(ctg_result* local, const int64_t* recv, const int64_t* counts_all, int world_size, int rank,
                   double hist_lo, double hist_hi, void* stream, ctg_result** out) {
    ApiCall c;
    if (!mgpu_args(local, world_size, "ctg_mgpu_merge") || !counts_all || !out || rank < 0 || rank >= world_size ||
        !(hist_hi > hist_lo))
        return CTG_ERR_ARG;
    *out = nullptr;
    if (!local->owned.empty()) {   // a shard's arrays are interior pointers of its owned blocks
        set_error("ctg_mgpu_merge: the local table is itself a merge shard; pass the rank's local call");
        return CTG_ERR_ARG;
    }
    const ExchangePlan p = exchange_plan(counts_all, world_size, rank);
    int rc = exchange_args("ctg_mgpu_merge", local, p, p.recv.words(), !recv, "null receive buffer");
    if (rc || (rc = c.begin(stream, new_result)) != CTG_OK) return rc;
    if ((rc = shard_nodes(c, local, recv, p)) != CTG_OK) return rc;
    if (p.recv.rows() == 0 && !local->partial_adj) shard_own_range(local, p, c.r.get());
    else if ((rc = merge_rows(c, local, recv, p, hist_lo, hist_hi)) != CTG_OK) return rc;
    local->n_edges = 0;
    local->n_nodes = 0;
    return c.end(false, out);
}

}  // extern "C"
