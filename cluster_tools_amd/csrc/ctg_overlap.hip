// Label overlaps (node labels): the contingency table of two label volumes.
// Replaces the array work of ndist.computeAndSerializeLabelOverlaps
// (node_labels/block_node_labels.py:161), ndist.mergeAndSerializeOverlaps
// (node_labels/merge_node_labels.py:149) and the arg-max those callers take.
//
//   k_overlap_scan   box of (labels, values) -> (key = a32 << 32 | b32, count u32)
//                    records, one per (tile flush, pair): a tile-table scan
//                    (ctg_tile_table.h)
//   radix sort       records by key (rocPRIM radix_sort_pairs)   \ sort_and_number, shared
//   k_overlap_heads  run heads of the sorted keys: a new (a, b), a new a   / with the other two
//   k_overlap_runs   run sums in u64 -> the sorted unique (a, b) table, its
//                    counts, the distinct a (nodes) and their CSR row offsets: a
//                    run fold (ctg_run_fold.h)
//   k_overlap_argmax per node: the b with the largest count, ties to the smallest b
#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include <algorithm>

#include "ctg_run_fold.h"

namespace ctg {

constexpr int OV_CAP = 2048;      // LDS table entries (u64 key + u32 count: 24 KiB)

// The tile-table policy of the overlaps: key = a32 << 32 | b32, payload one u32
// count (a no-return add; a tile holds 8192 voxels: no wrap).  Voxels with
// values == ignore are skipped (with_ignore); the high halves of the counted
// labels / values raise bit 0 / bit 1 of label_overflow.
template <typename LabelT, typename ValueT>
struct OverlapTable {
    using Key = uint64_t;
    static constexpr Key EMPTY = EMPTY_KEY;
    static constexpr int CAP = OV_CAP;
    static constexpr bool SET = false, HOLES = true;
    const LabelT* __restrict__ A;
    const ValueT* __restrict__ B;
    int with_ignore;
    uint64_t ignore;
    uint64_t* keys;
    uint32_t* tcnt;
    uint64_t* __restrict__ rkey;
    uint32_t* __restrict__ rcnt;
    unsigned long long* count;
    Counters* C;
    struct Voxel {
        uint64_t a, b;
    };
    __device__ Voxel load(int64_t p, bool in) const { return Voxel{in ? (uint64_t)A[p] : 0ull, in ? (uint64_t)B[p] : 0ull}; }
    __device__ bool valid(const Voxel& v, bool in) const { return in && !(with_ignore && v.b == ignore); }
    __device__ Key key(const Voxel& v) const { return ((uint64_t)(uint32_t)v.a << 32) | (uint32_t)v.b; }
    __device__ uint32_t overflow(const Voxel& v) const { return ((v.a >> 32) ? 1u : 0u) | ((v.b >> 32) ? 2u : 0u); }
    __device__ NoFold fold(const Voxel&, bool, uint64_t, int) const { return {}; }
    __device__ uint32_t head(uint32_t run, int, int, int, NoFold) const { return run; }
    __device__ void add(uint32_t h, uint32_t run) const { atomicAdd(&tcnt[h], run); }
    __device__ void put_direct(uint64_t slot, Key key, uint32_t run, int64_t, int64_t, int64_t, NoFold) const {
        rkey[slot] = key;
        rcnt[slot] = run;
    }
    __device__ void put_flush(uint64_t slot, int e, Key key, const TileBox&) const {
        rkey[slot] = key;
        rcnt[slot] = tcnt[e];
    }
    __device__ void clear(int e) const {
        keys[e] = EMPTY;
        tcnt[e] = 0;
    }
};

template <typename LabelT, typename ValueT>
__global__ __launch_bounds__(TT_THREADS) void k_overlap_scan(const LabelT* __restrict__ A,
                                                              const ValueT* __restrict__ B, int64_t Y, int64_t X,
                                                              int64_t bz, int64_t by, int64_t bx, int64_t ez,
                                                              int64_t ey, int64_t ex, int with_ignore,
                                                              uint64_t ignore, uint64_t* __restrict__ rkey,
                                                              uint32_t* __restrict__ rcnt, int64_t cap,
                                                              Counters* C) {
    __shared__ uint64_t tkey[OV_CAP];
    __shared__ uint32_t tcnt[OV_CAP];
    const OverlapTable<LabelT, ValueT> pol{A, B, with_ignore, ignore, tkey, tcnt, rkey, rcnt, &C->n_records, C};
    tile_table_scan(pol, tile_of_grid(Y, X, bz, by, bx, ez, ey, ex), cap);
}

template <typename LabelT, typename ValueT>
static hipError_t launch_overlap_scan_t(const void* A, const void* B, const int64_t* shape, const int64_t* b,
                                        const int64_t* e, int with_ignore, uint64_t ignore, uint64_t* rkey,
                                        uint32_t* rcnt, int64_t cap, Counters* C, hipStream_t s) {
    dim3 grid;
    CTG_TRY(tile_grid(b, e, &grid));
    hipLaunchKernelGGL((k_overlap_scan<LabelT, ValueT>), grid, dim3(TT_THREADS), 0, s, (const LabelT*)A,
                       (const ValueT*)B, shape[1], shape[2], b[0], b[1], b[2], e[0], e[1], e[2], with_ignore, ignore,
                       rkey, rcnt, cap, C);
    return hipGetLastError();
}

static hipError_t launch_overlap_scan(const void* A, int abits, const void* B, int bbits, const int64_t* shape,
                                      const int64_t* b, const int64_t* e, int with_ignore, uint64_t ignore,
                                      uint64_t* rkey, uint32_t* rcnt, int64_t cap, Counters* C, hipStream_t s) {
    if (abits == 32)
        return bbits == 32 ? launch_overlap_scan_t<uint32_t, uint32_t>(A, B, shape, b, e, with_ignore, ignore, rkey,
                                                                       rcnt, cap, C, s)
                           : launch_overlap_scan_t<uint32_t, uint64_t>(A, B, shape, b, e, with_ignore, ignore, rkey,
                                                                       rcnt, cap, C, s);
    return bbits == 32 ? launch_overlap_scan_t<uint64_t, uint32_t>(A, B, shape, b, e, with_ignore, ignore, rkey, rcnt,
                                                                   cap, C, s)
                       : launch_overlap_scan_t<uint64_t, uint64_t>(A, B, shape, b, e, with_ignore, ignore, rkey, rcnt,
                                                                   cap, C, s);
}

// sorted keys -> per record: bit 0 a new (a, b), bit 32 a new a; their
// inclusive prefix sums number the table rows (low word) and nodes (high word)
__global__ void k_overlap_heads(int64_t n, const uint64_t* __restrict__ key, uint64_t* __restrict__ flags) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t k = key[i], p = i ? key[i - 1] : ~k;
    flags[i] = (k != p ? 1ull : 0ull) | ((k >> 32) != (p >> 32) ? 1ull << 32 : 0ull);
}

// The run-fold policy of the overlaps (ctg_run_fold.h): the sort's payload is
// the count itself, summed in u64 (merged counts pass 2^32) and added to
// counts, zeroed before the launch.  A run head writes its (a, b) pair, the
// first row of a node (the high scan word steps) the node and its row offset.
template <typename CountT>
struct OverlapRuns {
    using Value = uint64_t;
    const uint64_t* __restrict__ key;
    const CountT* __restrict__ cnt;
    uint64_t *__restrict__ pairs, *__restrict__ nodes;
    unsigned long long* __restrict__ counts;
    int64_t* __restrict__ row_off;
    int64_t n, E, N;
    __device__ __forceinline__ void load(Value& v, int64_t i, bool in) const { v = in ? (uint64_t)cnt[i] : 0ull; }
    __device__ __forceinline__ void combine(Value& v, int o, bool take) const {
        const uint64_t vo = shfl_down_u64(v, o);
        v += take ? vo : 0ull;
    }
    __device__ __forceinline__ void apply(uint32_t seg, const Value& v) const {
        atomicAdd(&counts[seg], (unsigned long long)v);
    }
    __device__ __forceinline__ void name(int64_t i, uint32_t seg, bool head, uint64_t sc, uint64_t sp) const {
        const uint64_t k = key[i];
        if (head) {
            pairs[2 * (int64_t)seg] = k >> 32;
            pairs[2 * (int64_t)seg + 1] = k & 0xFFFFFFFFull;
        }
        if ((sc >> 32) != (sp >> 32)) {
            const int64_t nd = (int64_t)(sc >> 32) - 1;
            CTG_IDX(nd, N);
            nodes[nd] = k >> 32;
            row_off[nd] = (int64_t)seg;
        }
        if (i == n - 1) row_off[N] = E;
    }
};

template <typename CountT>
__global__ __launch_bounds__(256) void k_overlap_runs(int64_t n, const uint64_t* __restrict__ key,
                                                      const CountT* __restrict__ cnt,
                                                      const uint64_t* __restrict__ scan, uint64_t* __restrict__ pairs,
                                                      unsigned long long* __restrict__ counts,
                                                      uint64_t* __restrict__ nodes, int64_t* __restrict__ row_off,
                                                      int64_t E, int64_t N) {
    run_fold(OverlapRuns<CountT>{key, cnt, pairs, nodes, counts, row_off, n, E, N}, n, scan, E);
}

// One thread per node: the first largest count of its rows -- b ascends within
// a node, so ties go to the smallest b.  out_* are dense over [lb, le) and
// zeroed before the launch.
__global__ void k_overlap_argmax(int64_t N, const uint64_t* __restrict__ nodes, const int64_t* __restrict__ row_off,
                                 const uint64_t* __restrict__ pairs, const uint64_t* __restrict__ counts, int64_t E,
                                 uint64_t lb, uint64_t le, uint64_t* __restrict__ out_l,
                                 uint64_t* __restrict__ out_c) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= N) return;
    const uint64_t a = nodes[j];
    if (a < lb || a >= le) return;
    uint64_t best = 0, bl = 0;
    for (int64_t r = row_off[j]; r < row_off[j + 1]; ++r) {
        CTG_IDX(r, E);
        const uint64_t c = counts[r];
        if (c > best) {
            best = c;
            bl = pairs[2 * r + 1];
        }
    }
    out_l[a - lb] = bl;
    if (out_c) out_c[a - lb] = best;
}

__global__ void k_overlap_pack(int64_t n, const uint64_t* __restrict__ pairs, uint64_t* __restrict__ key) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) key[i] = (pairs[2 * i] << 32) | (uint32_t)pairs[2 * i + 1];
}

// dense ids -> labels, per column (null table: the column holds labels already)
__global__ void k_overlap_map_back(int64_t E, uint64_t* __restrict__ pairs, const uint64_t* __restrict__ Ua,
                                   int64_t na, const uint64_t* __restrict__ Ub, int64_t nb) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= E) return;
    if (Ua) {
        CTG_IDX(pairs[2 * i], na);
        pairs[2 * i] = Ua[pairs[2 * i]];
    }
    if (Ub) {
        CTG_IDX(pairs[2 * i + 1], nb);
        pairs[2 * i + 1] = Ub[pairs[2 * i + 1]];
    }
}

// rank of x in the sorted table U, or 0xFFFFFFFF if absent
__global__ void k_overlap_find(const uint64_t* __restrict__ U, int64_t n, uint64_t x, uint32_t* out) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (U[mid] < x) lo = mid + 1;
        else hi = mid;
    }
    *out = (lo < n && U[lo] == x) ? (uint32_t)lo : 0xFFFFFFFFu;
}

// (ctg_internal.h)  Marks phases 3 and 4; instantiated for the two record types below.
template <typename ValueT>
hipError_t sort_and_number(Workspace& w, const uint64_t* key, const ValueT* val, int64_t n, unsigned end_bit,
                           hipStream_t s, uint64_t* ks, ValueT* vs, uint64_t* scan, uint64_t* last) {
    Ev ev{w, s};
    DevBuf<uint64_t> flags((size_t)n * 8);
    if (!flags) return hipErrorOutOfMemory;
    CTG_TRY(with_temp(w.temp, [&](void* t, size_t& tb) {
        return rocprim::radix_sort_pairs(t, tb, key, ks, val, vs, (size_t)n, 0u, end_bit, s);
    }));
    ev.mark(3);
    hipLaunchKernelGGL(k_overlap_heads, grid_for(n), dim3(256), 0, s, n, ks, flags.p);
    CTG_TRY(hipGetLastError());
    CTG_TRY(with_temp(w.temp, [&](void* t, size_t& tb) {
        return rocprim::inclusive_scan(t, tb, flags.p, scan, (size_t)n, rocprim::plus<uint64_t>(), s);
    }));
    CTG_TRY(hipMemcpyAsync(last, scan + (n - 1), 8, hipMemcpyDeviceToHost, s));
    CTG_TRY(hipStreamSynchronize(s));
    ev.mark(4);
    return hipSuccess;
}
template hipError_t sort_and_number<uint32_t>(Workspace&, const uint64_t*, const uint32_t*, int64_t, unsigned,
                                              hipStream_t, uint64_t*, uint32_t*, uint64_t*, uint64_t*);
template hipError_t sort_and_number<uint64_t>(Workspace&, const uint64_t*, const uint64_t*, int64_t, unsigned,
                                              hipStream_t, uint64_t*, uint64_t*, uint64_t*, uint64_t*);

// n (key, count) records -> the result's table: equal keys add their counts
template <typename CountT>
static hipError_t overlap_reduce_t(Workspace& w, const uint64_t* key, const CountT* cnt, int64_t n, hipStream_t s,
                                   ctg_result* r) {
    return fold_records<false>(
        w, key, cnt, n, 64u, s, [&](const uint64_t* ks, const CountT* cs, const uint64_t* scan, int64_t E, int64_t N) {
            DevBuf<uint64_t> pairs((size_t)E * 16), counts((size_t)E * 8), nodes((size_t)N * 8);
            DevBuf<int64_t> row_off((size_t)(N + 1) * 8);
            if (!pairs || !counts || !nodes || !row_off) return hipErrorOutOfMemory;
            CTG_TRY(hipMemsetAsync(counts.p, 0, (size_t)E * 8, s));
            hipLaunchKernelGGL(k_overlap_runs<CountT>, grid_for(n), dim3(256), 0, s, n, ks, cs, scan, pairs.p,
                               (unsigned long long*)counts.p, nodes.p, row_off.p, E, N);
            CTG_TRY(hipGetLastError());
            swap_in(r->edges, pairs);
            swap_in(r->counts, counts);
            swap_in(r->nodes, nodes);
            swap_in(r->row_off, row_off);
            r->n_edges = E;
            r->n_nodes = N;
            return hipSuccess;
        });
}

hipError_t overlap_reduce(Workspace& w, const uint64_t* key, const uint64_t* cnt, int64_t n, hipStream_t s,
                          ctg_result* r) {
    return overlap_reduce_t<uint64_t>(w, key, cnt, n, s, r);
}

hipError_t overlap_tables(Workspace& w, const void* A, int abits, const void* B, int bbits, const int64_t* shape,
                          const int64_t* b, const int64_t* e, int with_ignore, uint64_t ignore, hipStream_t s,
                          ctg_result* r, unsigned* overflow) {
    return scan_tables<uint32_t>(
        w, (e[0] - b[0]) * (e[1] - b[1]) * (e[2] - b[2]), s, 1,
        [&](uint64_t* rkey, uint32_t* rcnt, int64_t cap) {
            return launch_overlap_scan(A, abits, B, bbits, shape, b, e, with_ignore, ignore, rkey, rcnt, cap,
                                       w.counters, s);
        },
        [&](const uint64_t* rkey, const uint32_t* rcnt, int64_t m) { return overlap_reduce_t(w, rkey, rcnt, m, s, r); },
        true, r, overflow);
}

hipError_t launch_overlap_pack(int64_t n, const uint64_t* pairs, uint64_t* key, hipStream_t s) {
    hipLaunchKernelGGL(k_overlap_pack, grid_for(n), dim3(256), 0, s, n, pairs, key);
    return hipGetLastError();
}

hipError_t launch_overlap_map_back(int64_t E, uint64_t* pairs, const uint64_t* Ua, int64_t na, const uint64_t* Ub,
                                   int64_t nb, hipStream_t s) {
    if (E == 0 || (!Ua && !Ub)) return hipSuccess;
    hipLaunchKernelGGL(k_overlap_map_back, grid_for(E), dim3(256), 0, s, E, pairs, Ua, na, Ub, nb);
    return hipGetLastError();
}

hipError_t launch_overlap_find(const uint64_t* U, int64_t n, uint64_t x, uint32_t* out, hipStream_t s) {
    hipLaunchKernelGGL(k_overlap_find, dim3(1), dim3(1), 0, s, U, n, x, out);
    return hipGetLastError();
}

hipError_t launch_overlap_argmax(const ctg_result* r, uint64_t lb, uint64_t le, uint64_t* out_l, uint64_t* out_c,
                                 hipStream_t s) {
    if (r->n_nodes == 0) return hipSuccess;
    hipLaunchKernelGGL(k_overlap_argmax, grid_for(r->n_nodes), dim3(256), 0, s, r->n_nodes, r->nodes, r->row_off,
                       r->edges, r->counts, r->n_edges, lb, le, out_l, out_c);
    return hipGetLastError();
}

CTG_BOUNDS_TAKE(overlap)

}  // namespace ctg
