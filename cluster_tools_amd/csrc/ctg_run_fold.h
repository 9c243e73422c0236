// The record back half of the label-table calls (label overlaps, segment morphology, region features): what follows
// a tile-table scan (ctg_tile_table.h) or a merge kernel.  n (key, record) pairs are sorted by key and their runs
// numbered (sort_and_number), then every run is folded into one row of the result.  The protocol (DESIGN.md 3,
// "Record back half") is stated once, in run_fold; k_overlap_runs, k_morph_runs and k_region_runs are policies over
// it, and the host halves -- fold_records, scan_tables, merge_rows -- take what differs as callables.  Every buffer
// is call-sized and comes from the pool (DevBuf); nothing touches the workspace's record or sort buffers, so a
// CTG_DEFER_STATS handle stays valid across these calls.
#pragma once
#include "ctg_tile_table.h"

namespace ctg {

// The fold of the sorted records, one thread per sorted position, 256 a workgroup.  Position i belongs to row
// seg = scan[i].lo - 1: scan is the inclusive prefix sum of the run heads, so the positions of a row are contiguous.
// n < RECORD_LIMIT, so the row numbers fit 32 bits and all ones, the seg of the lanes past n, is no row.
// A wave folds its 64 positions per row by segmented suffix folds over __shfl_down: at distance o a lane takes its
// partner's fold if the partner is in the wave (the wave-edge rule, lane + o < WAVE: a shuffle past the edge returns
// the lane's own value, which must not be folded twice) and has the same seg -- then every lane between them has it
// too.  After the six steps the first lane of every segment of the wave (lane 0, or a lane whose predecessor has
// another seg) holds the segment's fold and applies it to the row by the policy's atomics: one atomic set per (wave,
// row), none contended unless a row spans waves.  The rows hold the fold's identity before the launch and nothing
// else writes them, so no order of the waves leaves a stale or a lost part.  The run head of a row (the low scan
// word steps) names it.  The policy P supplies what differs:
//   Value               what a lane folds
//   load(v, i, in)      v = the record of sorted position i; the fold's identity when !in
//   combine(v, o, take) v = v (+) the partner's at distance o if take; it does its own shuffles: every lane calls it
//   apply(seg, v)       the atomic set of a segment's fold on row seg
//   name(i, seg, head, sc, sp)   what position i writes besides: the row's name where head, and whatever else the
//                       scan words of i and i - 1 (sc, sp) decide
template <class P>
__device__ __forceinline__ void run_fold(const P& pol, int64_t n, const uint64_t* __restrict__ scan, int64_t rows) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = threadIdx.x & (WAVE - 1);
    const bool in = i < n;
    const uint64_t sc = in ? scan[i] : 0ull, sp = (in && i) ? scan[i - 1] : 0ull;
    const uint32_t seg = in ? (uint32_t)sc - 1u : 0xFFFFFFFFu;
    typename P::Value v;
    pol.load(v, i, in);
#pragma unroll   // (six steps, their distances constants)
    for (int o = 1; o < WAVE; o <<= 1) {
        const uint32_t so = __shfl_down(seg, o, WAVE);
        pol.combine(v, o, lane + o < WAVE && so == seg);
    }
    const uint32_t sprev = __shfl_up(seg, 1, WAVE);
    if (!in) return;
    if (lane == 0 || sprev != seg) {
        CTG_IDX(seg, rows);
        pol.apply(seg, v);
    }
    pol.name(i, seg, (uint32_t)sc != (uint32_t)sp, sc, sp);
}

// record slots before the sort: idx[i] = i
template <typename T>
__global__ void k_iota(int64_t n, T* __restrict__ idx) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) idx[i] = (T)i;
}

// n (key, payload) records -> rows: sort by the keys' low end_bit bits, number the runs, fold them.  n in (0,
// RECORD_LIMIT).  The payload is what the sort carries along: the records' own u32 slots (SLOTS: made here, the
// argument is ignored) or, for the overlaps, the counts themselves.  rows(ks, ps, scan, N, H) gets the sorted keys and
// payloads, the scan words, the number of rows and of distinct high key halves; it allocates the family's rows, sets
// them to the fold's identity, launches the runs kernel and what follows it, and swaps the rows into the result.
// Marks phases 3 and 4 (sort_and_number) and 5.
template <bool SLOTS, class Payload, class Rows>
hipError_t fold_records(Workspace& w, const uint64_t* key, const Payload* payload, int64_t n, unsigned end_bit,
                        hipStream_t s, Rows&& rows) {
    Ev ev{w, s};
    DevBuf<uint64_t> ks((size_t)n * 8), scan((size_t)n * 8);
    DevBuf<Payload> idx, ps((size_t)n * sizeof(Payload));
    if (!ks || !scan || !ps) return hipErrorOutOfMemory;
    if constexpr (SLOTS) {
        if (!(payload = idx.alloc((size_t)n * sizeof(Payload)))) return hipErrorOutOfMemory;
        hipLaunchKernelGGL(k_iota<Payload>, grid_for(n), dim3(256), 0, s, n, idx.p);
        CTG_TRY(hipGetLastError());
    }
    uint64_t last = 0;
    CTG_TRY(sort_and_number(w, key, payload, n, end_bit, s, ks.p, ps.p, scan.p, &last));
    idx.reset();
    CTG_TRY(rows(ks.p, ps.p, scan.p, (int64_t)(uint32_t)last, (int64_t)(last >> 32)));
    ev.mark(5);
    return hipSuccess;
}

// buf takes the place of a result's table
template <class T, class U>
void swap_in(T*& table, DevBuf<U>& buf) {
    dev_free(table);
    table = (T*)buf.release();
}

// The scan of a box of `voxels` voxels into call-sized records (a u64 key and `words` Rec each) and their fold into r.
// launch(rkey, rec, cap) queues the family's tile-table scan, reduce(rkey, rec, m) is its fold_records.  *overflow set:
// r is untouched.  A scan that leaves no record (every voxel ignored) keeps r's empty placeholders if allow_empty,
// and is an error otherwise (the morphology has no ignore label).  Marks phases 0 to 2 (scan_into_records) and 6.
template <class Rec, class Launch, class Reduce>
hipError_t scan_tables(Workspace& w, int64_t voxels, hipStream_t s, int words, Launch&& launch, Reduce&& reduce,
                       bool allow_empty, ctg_result* r, unsigned* overflow) {
    Ev ev{w, s};
    DevBuf<uint64_t> rkey;
    DevBuf<Rec> rec;
    int64_t m = 0;
    CTG_TRY(scan_into_records(
        w, voxels, s,
        [&](int64_t cap) {
            rkey.reset();
            rec.reset();
            if (!rkey.alloc((size_t)cap * 8) || !rec.alloc((size_t)cap * words * sizeof(Rec)))
                return hipErrorOutOfMemory;
            return launch(rkey.p, rec.p, cap);
        },
        &m, overflow));
    if (*overflow) return hipSuccess;
    // (the API refuses boxes of RECORD_LIMIT voxels or more)
    if (m >= RECORD_LIMIT || (m <= 0 && !allow_empty)) return hipErrorInvalidValue;
    r->n_records = m;
    r->n_direct = (int64_t)w.counters_host->n_direct;
    if (m == 0) {   // the caller's empty placeholders stay
        for (int i = 3; i <= 6; ++i) ev.mark(i);
        return hipSuccess;
    }
    CTG_TRY(reduce(rkey.p, rec.p, m));
    ev.mark(6);
    return hipSuccess;
}

// n > 0 float64 rows (device) -> records of `words` u64 -> r.  kernel(n, rows, key, rec, bad) is the family's merge
// kernel, which ors 1 into the device word *bad for a row it refuses; reduce(key, rec) is its fold_records over keys
// of 53 bits.  *bad set: r is untouched.  Marks phases 0 to 2 and 6.
template <class Kernel, class Reduce>
hipError_t merge_rows(Workspace& w, const double* rows, int64_t n, int words, Kernel kernel, Reduce&& reduce,
                      hipStream_t s, ctg_result* r, int* bad) {
    *bad = 0;
    Ev ev{w, s};
    DevBuf<uint64_t> key((size_t)n * 8), rec((size_t)n * words * 8);
    if (!key || !rec) return hipErrorOutOfMemory;
    CTG_TRY(hipMemsetAsync(w.counters, 0, sizeof(Counters), s));
    ev.mark(0);
    hipLaunchKernelGGL(kernel, grid_for(n), dim3(256), 0, s, n, rows, key.p, rec.p, &w.counters->label_overflow);
    CTG_TRY(hipGetLastError());
    ev.mark(1);
    ev.mark(2);
    CTG_TRY(hipMemcpyAsync(w.counters_host, w.counters, sizeof(Counters), hipMemcpyDeviceToHost, s));
    CTG_TRY(hipStreamSynchronize(s));
    if (w.counters_host->label_overflow) {
        *bad = 1;
        return hipSuccess;
    }
    CTG_TRY(reduce(key.p, rec.p));
    ev.mark(6);
    r->n_records = n;
    return hipSuccess;
}
}  // namespace ctg
