// The shared back half of every call: records (n, with keys (u<<32|v) or
// (u,v) pairs) -> sorted run table -> reduced edge / feature tables -> nodes.
#include <hip/hip_runtime.h>
#include <cstdlib>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_run_length_encode.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/device/device_select.hpp>

#include <algorithm>

#include "ctg_internal.h"

namespace ctg {

// Record sort: (u,v) keys packed to 2*nb bits (34 at 1.3e5 labels).  rocPRIM's
// gfx950 default sorts 8 bits per onesweep pass (5 passes at 34 bits, each a
// launch with its own decoupled look-back); 10-bit digits cut that to 4 (34 bits)
// and the sort from 0.185 to 0.151 ms at 512^3 (11+ bits exceed the LDS of the
// histogram kernel).
#ifndef CTG_SORT_BITS
#define CTG_SORT_BITS 10
#endif
#ifndef CTG_SORT_BLOCK
#define CTG_SORT_BLOCK 1024
#endif
#ifndef CTG_SORT_IPT
#define CTG_SORT_IPT 8
#endif
#if CTG_SORT_BITS
using RecordSortConfig = rocprim::radix_sort_config<
    rocprim::default_config, rocprim::default_config,
    rocprim::radix_sort_onesweep_config<rocprim::kernel_config<256, 16>,
                                        rocprim::kernel_config<CTG_SORT_BLOCK, CTG_SORT_IPT>, CTG_SORT_BITS,
                                        rocprim::block_radix_rank_algorithm::match>>;
#else
using RecordSortConfig = rocprim::default_config;
#endif

// the sort switches of ctg_plan.h, read per call: A/B runs and tests switch them
static SortSwitches sort_switches() {
    auto off = [](const char* name) {
        const char* e = getenv(name);
        return e && e[0] == '0';
    };
    SortSwitches sw;
    sw.packed = !off("CTG_SORT_PACKED");
    sw.bucket = !off("CTG_BUCKET_SORT");
    if (const char* e = getenv("CTG_BUCKET_SORT_PAIRS")) sw.bucket_pairs = e[0] == '1';
    sw.group = !off("CTG_GROUP_SORT");
    const char* gf = getenv("CTG_GROUP_FIRST");
    sw.group_first = gf && gf[0] == '1';
    return sw;
}

// Step 1's result: the runs of equal keys lie in the sort scratch's uniq /
// runs / offs, their count in w.small[SLOT_RUNS]; sorted position r is record
// slot perm(r).
struct RunTable {
    bool packed;   // the slots are the low ib bits of sk_out (else the u32 permutation idx_out)
    int ib;
    Perm perm(const SortScratch& S) const {
        return Perm{packed ? nullptr : S.idx_out, packed ? S.sk_out : nullptr, packed ? ib : 0};
    }
};

// record sort -> run table (phase marks 2, 3)
static hipError_t sort_to_runs(Workspace& w, const ReduceJob& J, int nb, int ub, Ev& ev, hipStream_t s, RunTable& T) {
    const int64_t n = J.n;
    const SortScratch& S = w.sort;
    uint32_t* dE_all = w.small + SLOT_RUNS;
    hipError_t e = hipSuccess;
    const int ib = J.regions ? bits_for((uint64_t)std::max<int64_t>(J.R.cap - 1, 1)) : 0;
    // block-tagged keys (ctg_rag_blocks, J.ub set) are not spread over their top bits
    const bool spread = J.ub == 0;
    const RecordSortPlan plan =
        plan_record_sort(J.keys != nullptr, J.regions != nullptr, n, ub, nb, ib, spread, sort_switches());
    T = RunTable{plan.packed, ib};
    // what ctg_last_sort reports: host values this function holds anyway
    SortReport& rep = w.last_sort;
    rep = SortReport{};
    rep.path = (int)plan.path;
    rep.packed = plan.packed;
    rep.group_tried = plan.try_group;
    rep.ib = ib;
    rep.nb = nb;
    rep.ub = ub;
    rep.n = n;
    if (plan.try_group) {
        bool grouped = false;
        ev.mark(2);   // (phases: the whole group sort is "sort")
        CTG_TRY(group_sort_runs(J.keys, J.R.rcap, *J.regions, n, nb, ub, ib, J.min_u, J.max_v, w.gsort,
                                w.small_host + SLOT_GROUP_SORT, S.sk_out, S.idx_out, S.uniq, S.runs, S.offs, dE_all, &grouped, &rep, s));
        if (grouped) {
            ev.mark(3);
            rep.group_done = 1;
            rep.path = CTG_SORT_PATH_GROUP;
            rep.packed = 0;
            T.packed = false;   // (key, slot) runs and a u32 slot permutation, as for unpackable records
            return hipSuccess;
        }
    }
    if (J.keys && J.regions)
        e = launch_pack_regions(J.keys, J.R.rcap, *J.regions, nb, T.packed ? ib : 0, S.sk_in, S.idx_in, s);
    else if (J.keys) e = launch_pack_keys(n, J.keys, nb, S.sk_in, S.idx_in, s);
    else e = launch_pack_pairs(n, J.pairs, nb, S.sk_in, S.idx_in, s);
    if (e != hipSuccess) return e;
    ev.mark(2);
    bool have_offs = false;   // run offsets already written (bucket paths)
    switch (plan.path) {
    case SortPath::BucketKeys: {
        // MSD bucket pass + segmented sort of the key bits (ctg_sort.hip):
        // 4 fused launches instead of 4 onesweep passes with their fills
        const KeyRange kr = packed_key_range(J.min_u, J.max_v, nb, ib);
        uint32_t nbk = 0;
        CTG_TRY(bucket_sort_keys(S.sk_in, S.uniq, S.sk_out, n, ib, ib + ub + nb, kr.kmin, kr.kmax, w.bsort, w.temp,
                                 &nbk, s));
        ev.mark(3);
        // runs from the buckets: unique keys, lengths and offsets in one go
        e = bucket_runs(S.sk_out, n, ib, nbk, w.bsort, S.uniq, S.runs, S.offs, dE_all, s);
        have_offs = true;
        break;
    }
    case SortPath::OnesweepKeys: {
        CTG_TRY(with_temp(w.temp, [&](void* t, size_t& tb) {
            return rocprim::radix_sort_keys<RecordSortConfig>(t, tb, S.sk_in, S.sk_out, (size_t)n, (unsigned)ib,
                                                              (unsigned)(ib + ub + nb), s);
        }));
        ev.mark(3);
        auto key_only = rocprim::make_transform_iterator(S.sk_out, [ib] __device__(uint64_t k) { return k >> ib; });
        e = with_temp(w.temp, [&](void* t, size_t& tb) {
            return rocprim::run_length_encode(t, tb, key_only, (unsigned)n, S.uniq, S.runs, dE_all, s);
        });
        break;
    }
    case SortPath::BucketPairs: {
        // tmp buffers: S.uniq (keys) and S.keep (values) are free until the
        // run-length pass / the reduction
        uint32_t nbk = 0;
        CTG_TRY(bucket_sort_pairs(S.sk_in, S.idx_in, S.uniq, S.keep, S.sk_out, S.idx_out, n, ub + nb, w.bsort,
                                  w.temp, &nbk, s));
        ev.mark(3);
        // runs never cross the MSD buckets: unique keys, lengths and offsets per bucket
        e = bucket_runs(S.sk_out, n, 0, nbk, w.bsort, S.uniq, S.runs, S.offs, dE_all, s);
        have_offs = true;
        break;
    }
    case SortPath::OnesweepPairsWide:
    case SortPath::OnesweepPairsDefault:
        CTG_TRY(with_temp(w.temp, [&](void* t, size_t& tb) {
            return plan.path == SortPath::OnesweepPairsWide
                       ? rocprim::radix_sort_pairs<RecordSortConfig>(t, tb, S.sk_in, S.sk_out, S.idx_in, S.idx_out,
                                                                     (size_t)n, 0u, (unsigned)(ub + nb), s)
                       : rocprim::radix_sort_pairs(t, tb, S.sk_in, S.sk_out, S.idx_in, S.idx_out, (size_t)n, 0u,
                                                   (unsigned)(ub + nb), s);
        }));
        ev.mark(3);
        e = with_temp(w.temp, [&](void* t, size_t& tb) {
            return rocprim::run_length_encode(t, tb, S.sk_out, (unsigned)n, S.uniq, S.runs, dE_all, s);
        });
        break;
    }
    if (e != hipSuccess || have_offs) return e;
    // offsets over the n-bound: entries past E_all are never read
    return with_temp(w.temp, [&](void* t, size_t& tb) {
        return rocprim::exclusive_scan(t, tb, S.runs, S.offs, 0u, (size_t)n, rocprim::plus<uint32_t>(), s);
    });
}

// reduce the runs to edge / feature rows, compacted where rows may drop
static hipError_t reduce_runs(Workspace& w, const ReduceJob& J, int nb, const RunTable& T, hipStream_t s,
                              ctg_result* res) {
    const int64_t n = J.n;
    const SortScratch& S = w.sort;
    uint32_t* dE_all = w.small + SLOT_RUNS;
    uint32_t* dE = w.small + SLOT_EDGES;
    // outputs (uncompacted), sized by the bound n
    const bool may_drop = J.need_adj || J.ignore_label;
    // CTG_DEFER_STATS: result row e is run e of the records (no compaction),
    // whose statistics the exchange rebuilds where it needs them
    const bool defer = J.defer_stats && J.keep_stats && J.stats && !J.wide && !may_drop;
    const bool wide_out = J.keep_stats && J.stats && !defer;
    DevBuf<uint64_t> edges(n * 16);
    DevBuf<double> feats;
    DevBuf<uint32_t> wstats;
    DevBuf<double2> wsums;
    if (J.stats) feats.alloc(n * N_FEATURES * 8);
    if (wide_out) {
        wstats.alloc(n * WREC_WORDS * 4);
        wsums.alloc(n * 16);
    }
    if (!edges || (J.stats && !feats) || (wide_out && (!wstats || !wsums))) return hipErrorOutOfMemory;
    ReduceOut O{};
    O.edges = edges;
    O.feats = feats;
    O.keep = may_drop ? S.keep : nullptr;
    O.wstats = wstats;
    O.wsums = wsums;
    O.count_out = may_drop ? nullptr : dE;   // no compaction: the kernel copies the count
    O.n_rec = n;
#ifdef CTG_DIAG   // diagnostic reduce ablations exist only in diagnostic builds (make variant EXTRA=-DCTG_DIAG)
    {
        static const int ablate = [] { const char* v = getenv("CTG_REDUCE_ABLATE"); return v ? atoi(v) : 0; }();
        O.ablate = ablate;
    }
#else
    O.ablate = 0;
#endif
    // features-only narrow reduce: edges past 2^16 samples are listed for the
    // wide-histogram kernel (w.small[SLOT_HEAVY]: their count)
    DevBuf<uint32_t> heavy;
    const bool list_heavy = !J.wide && J.stats && !O.wstats;
    if (list_heavy && !heavy.alloc(n * 4)) return hipErrorOutOfMemory;
    const Perm perm = T.perm(S);
    hipError_t e = launch_reduce(n, dE_all, S.uniq, S.runs, S.offs, perm.p32, perm.p64, perm.ib, J.R, J.wide, J.stats,
                                 nb, J.umask, J.need_adj, J.ignore_label, J.scale, J.offset, O, s, heavy,
                                 list_heavy ? w.small + SLOT_HEAVY : nullptr);
    heavy.reset();   // stream-ordered reuse
    if (e != hipSuccess) return e;
    if (may_drop) {
        CTG_TRY(with_temp(w.temp, [&](void* t, size_t& tb) {
            return rocprim::exclusive_scan(t, tb, S.keep, S.pos, 0u, (size_t)n, rocprim::plus<uint32_t>(), s);
        }));
        DevBuf<uint64_t> c_edges(n * 16);
        DevBuf<double> c_feats;
        DevBuf<uint32_t> c_wstats;
        DevBuf<double2> c_wsums;
        if (O.feats) c_feats.alloc(n * N_FEATURES * 8);
        if (O.wstats) {
            c_wstats.alloc(n * WREC_WORDS * 4);
            c_wsums.alloc(n * 16);
        }
        if (!c_edges || (O.feats && !c_feats) || (O.wstats && (!c_wstats || !c_wsums))) return hipErrorOutOfMemory;
        ReduceOut C2{};
        C2.edges = c_edges;
        C2.feats = c_feats;
        C2.wstats = c_wstats;
        C2.wsums = c_wsums;
        CTG_TRY(launch_compact(n, dE_all, S.keep, S.pos, O, C2, dE, s));
        // the uncompacted tables go back to the pool (stream-ordered reuse)
        edges.reset(c_edges.release());
        feats.reset(c_feats.release());
        wstats.reset(c_wstats.release());
        wsums.reset(c_wsums.release());
    }
    res->edges = edges.release();
    res->features = feats.release();
    res->stats = wstats.release();
    res->stat_sums = wsums.release();
    if (defer) {
        res->defer.on = 1;
        res->defer.offs = S.offs;
        res->defer.runs = S.runs;
        res->defer.perm = perm;
        res->defer.hist = J.R.hist;
        res->defer.gen = w.gen;
        res->defer.n_runs = n;      // (the run count, set by the caller once read back)
        res->defer.n_rec = n;
        res->defer.rec_cap = J.R.cap;
    }
    return hipSuccess;
}

// nodes = unique endpoints of every unique key (before filtering); reads the
// device-resident counts back: counts[0..2] = runs, kept edges, nodes
static hipError_t collect_nodes(Workspace& w, const ReduceJob& J, int nb, hipStream_t s, ctg_result* res,
                                uint32_t* counts) {
    const int64_t n = J.n;
    const SortScratch& S = w.sort;
    uint32_t* dE_all = w.small + SLOT_RUNS;
    uint32_t* dN = w.small + SLOT_NODES;
    static_assert(SLOT_RUNS == 0 && SLOT_EDGES == 1 && SLOT_NODES == 2, "counts[] is read back as one range");
    // the first k of the device counts, after everything queued so far
    auto read_counts = [&](int k) {
        hipError_t e_ = hipMemcpyAsync(w.small_host, w.small, k * sizeof(uint32_t), hipMemcpyDeviceToHost, s);
        if (e_ == hipSuccess) e_ = hipStreamSynchronize(s);
        for (int i = 0; i < k && e_ == hipSuccess; ++i) counts[i] = w.small_host[i];
        return e_;
    };
    if (J.skip_nodes) {
        res->nodes = (uint64_t*)dev_alloc(8);
        return read_counts(2);
    }
    if (J.max_v < (1ull << 30)) {
        // bitmap over [smallest u, max label] (every node is an edge end, >= the
        // smallest u; a z-slab's labels start far above 0): one pass over the
        // sorted key table
        const uint32_t wbase = (uint32_t)(std::min<uint64_t>(J.min_u, J.max_v) >> 5);
        const int64_t W = (int64_t)(J.max_v >> 5) - wbase + 1;
        DevBuf<uint32_t> bits(W * 4), off(W * 4);
        const int64_t node_cap = std::min<int64_t>(W * 32, 2 * n);
        res->nodes = (uint64_t*)dev_alloc(node_cap * 8);
        if (!bits || !off || !res->nodes) return hipErrorOutOfMemory;
        CTG_TRY(hipMemsetAsync(bits, 0, W * 4, s));
        CTG_TRY(launch_mark_nodes(n, dE_all, S.uniq, nb, bits, W, wbase, s));
        // word offsets = exclusive scan of the words' popcounts (read through the scan's input iterator)
        // (tried: the scan and the expansion in one workgroup for small label ranges -- 0.053 -> 0.115 ms
        // at 512^3, the serial per-thread expansion loses to the wide launch)
        auto popc = rocprim::make_transform_iterator((uint32_t*)bits,
                                                     [] __device__(uint32_t b) { return (uint32_t)__popc(b); });
        CTG_TRY(with_temp(w.temp, [&](void* t, size_t& tb) {
            return rocprim::exclusive_scan(t, tb, popc, (uint32_t*)off, 0u, (size_t)W, rocprim::plus<uint32_t>(), s);
        }));
        CTG_TRY(launch_bits_to_nodes(W, bits, off, res->nodes, dN, node_cap, wbase, s));
        const hipError_t e = read_counts(3);
        bits.reset();
        off.reset();
        return e;
    }
    CTG_TRY(read_counts(2));
    const int64_t E_all = counts[0];
    DevBuf<uint32_t> ep(std::max<int64_t>(E_all, 1) * 8), ep2(std::max<int64_t>(E_all, 1) * 8),
        nodes32(std::max<int64_t>(E_all, 1) * 8);
    if (!ep || !ep2 || !nodes32) return hipErrorOutOfMemory;
    CTG_TRY(launch_endpoints(E_all, S.uniq, nb, ep, s));
    CTG_TRY(with_temp(w.temp, [&](void* t, size_t& tb) {
        return rocprim::radix_sort_keys(t, tb, (uint32_t*)ep, (uint32_t*)ep2, (size_t)(2 * E_all), 0u, (unsigned)nb, s);
    }));
    CTG_TRY(with_temp(w.temp, [&](void* t, size_t& tb) {
        return rocprim::unique(t, tb, (uint32_t*)ep2, (uint32_t*)nodes32, dN, (size_t)(2 * E_all),
                               rocprim::equal_to<uint32_t>(), s);
    }));
    CTG_TRY(hipMemcpyAsync(w.small_host + SLOT_NODES, dN, 4, hipMemcpyDeviceToHost, s));
    CTG_TRY(hipStreamSynchronize(s));
    counts[2] = w.small_host[SLOT_NODES];
    res->nodes = (uint64_t*)dev_alloc(std::max<int64_t>(counts[2], 1) * 8);
    if (!res->nodes) return hipErrorOutOfMemory;
    CTG_TRY(launch_u32_to_u64(counts[2], nodes32, res->nodes, s));
    const hipError_t e = hipStreamSynchronize(s);
    ep.reset();
    ep2.reset();
    nodes32.reset();
    return e;
}

hipError_t reduce_records(Workspace& w, const ReduceJob& J, hipStream_t s, ctg_result* res) {
    // Device-resident counts: the run count E_all, the kept edge count E and
    // the node count N stay in w.small (SLOT_RUNS .. SLOT_NODES) until one read-back at the end;
    // every kernel in between bounds itself by them, and buffers are sized by
    // the record count n (an upper bound), so the back half issues no
    // host synchronisation (except on the rare node path for labels >= 2^30).
    Ev ev{w, s};
    ++w.gen;   // the sort / run buffers are about to be overwritten
    const int64_t n = J.n;
    const int nb = bits_for(J.max_v);
    const int ub = J.ub ? J.ub : nb;
    if (nb > 32 || ub > 32) return hipErrorInvalidValue;
    if (n == 0) {
        w.last_sort = SortReport{};   // (path -1: nothing to sort)
        w.last_sort.nb = nb;
        w.last_sort.ub = ub;
        res->n_edges = 0;
        res->edges = (uint64_t*)dev_alloc(16);
        res->features = J.stats ? (double*)dev_alloc(N_FEATURES * 8) : nullptr;
        if (J.keep_stats && J.stats) {
            res->stats = (uint32_t*)dev_alloc(WREC_WORDS * 4);
            res->stat_sums = (double2*)dev_alloc(16);
        }
        res->nodes = (uint64_t*)dev_alloc(8);
        res->n_nodes = 0;
        if (J.single_label_ptr) {
            CTG_TRY(hipMemcpyAsync(res->nodes, J.single_label_ptr, 8, hipMemcpyDeviceToDevice, s));
            res->n_nodes = 1;
        }
        for (int i = 2; i <= 6; ++i) ev.mark(i);
        return hipStreamSynchronize(s);
    }
    if (!w.sort.reserve(n)) return hipErrorOutOfMemory;
    RunTable T{};
    CTG_TRY(sort_to_runs(w, J, nb, ub, ev, s, T));
    ev.mark(4);
    CTG_TRY(reduce_runs(w, J, nb, T, s, res));
    ev.mark(5);
    uint32_t counts[3] = {0, 0, 0};
    CTG_TRY(collect_nodes(w, J, nb, s, res, counts));
    res->n_edges = counts[1];
    res->n_nodes = counts[2];
    if (res->defer.on) res->defer.n_runs = counts[0];
    if (counts[0] == 0) {   // no edge at all: the owned origin voxel's label is the only node
        res->n_nodes = 0;
        if (J.single_label_ptr) {
            CTG_TRY(hipMemcpyAsync(res->nodes, J.single_label_ptr, 8, hipMemcpyDeviceToDevice, s));
            CTG_TRY(hipStreamSynchronize(s));
            res->n_nodes = 1;
        }
    }
    ev.mark(6);
    return hipSuccess;
}

}  // namespace ctg
