// Label overlaps (node labels): the contingency table of two label volumes.
// Replaces the array work of ndist.computeAndSerializeLabelOverlaps
// (node_labels/block_node_labels.py:161), ndist.mergeAndSerializeOverlaps
// (node_labels/merge_node_labels.py:149) and the arg-max those callers take.
//
//   k_overlap_scan   box of (labels, values) -> (key = a32 << 32 | b32, count u32)
//                    records, one per (tile flush, pair), through an LDS hash
//                    table per workgroup
//   radix sort       records by key (rocPRIM radix_sort_pairs)
//   k_overlap_heads  run heads of the sorted keys: a new (a, b), a new a
//   k_overlap_runs   run sums in u64 -> the sorted unique (a, b) table, its
//                    counts, the distinct a (nodes) and their CSR row offsets
//   k_overlap_argmax per node: the b with the largest count, ties to the smallest b
//
// Every buffer here is call-sized and comes from the pool (DevBuf); nothing
// touches the workspace's record or sort buffers, so a CTG_DEFER_STATS handle
// stays valid across these calls.
#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include <algorithm>

#include "ctg_internal.h"

namespace ctg {

constexpr int OV_THREADS = 256;   // 4 waves: 4 planes per step, as k_unique_tiles
constexpr int OV_TILE_Z = 16;
constexpr int OV_CAP = 2048;      // LDS table entries (u64 key + u32 count: 24 KiB)
constexpr int OV_PROBES = 32;     // linear probes before a head gives up on the table
static_assert((OV_CAP & (OV_CAP - 1)) == 0 && OV_CAP % OV_THREADS == 0, "table capacity");

// One workgroup per 64 x TILE_Y x 16 tile of the box.  A wave takes one row at
// a time: equal consecutive pairs collapse to their head lane (run length from
// the ballot of heads), and only heads touch the table -- CAS on the key word,
// a no-return add on the u32 count (a tile holds 8192 voxels: no wrap).  The
// table is written out when more than half full and at tile end, one global
// reservation per flush; a head that finds no slot within OV_PROBES writes its
// record directly (one reservation per wave row).  Records past `cap` are
// dropped: n_records still counts them and the host runs again with room.
// Voxels with values == ignore are skipped (with_ignore); the high halves of
// the counted labels / values raise bit 0 / bit 1 of label_overflow.
template <typename LabelT, typename ValueT>
__global__ __launch_bounds__(OV_THREADS) void k_overlap_scan(const LabelT* __restrict__ A,
                                                              const ValueT* __restrict__ B, int64_t Y, int64_t X,
                                                              int64_t bz, int64_t by, int64_t bx, int64_t ez,
                                                              int64_t ey, int64_t ex, int with_ignore,
                                                              uint64_t ignore, uint64_t* __restrict__ rkey,
                                                              uint32_t* __restrict__ rcnt, int64_t cap,
                                                              Counters* C) {
    __shared__ uint64_t tkey[OV_CAP];
    __shared__ uint32_t tcnt[OV_CAP];
    __shared__ uint32_t used;
    __shared__ uint32_t wpos;
    __shared__ unsigned long long base;
    const int tid = threadIdx.x;
    for (int e = tid; e < OV_CAP; e += OV_THREADS) {
        tkey[e] = EMPTY_KEY;
        tcnt[e] = 0;
    }
    if (tid == 0) used = 0;
    __syncthreads();
    const int lane = tid & (WAVE - 1), wave = tid >> 6;
    const int64_t x = bx + (int64_t)blockIdx.x * WAVE + lane;
    const int64_t y0 = by + (int64_t)blockIdx.y * TILE_Y;
    const int64_t z0 = bz + (int64_t)blockIdx.z * OV_TILE_Z;
    const bool in = x < ex;
    uint32_t over = 0;
    for (int zs = 0; zs < OV_TILE_Z; zs += OV_THREADS / WAVE) {
        const int64_t z = z0 + zs + wave;
        if (z < ez) {   // (wave-uniform, like the row bound below)
            for (int dy = 0; dy < TILE_Y; ++dy) {
                const int64_t y = y0 + dy;
                if (y >= ey) break;
                const int64_t p = (z * Y + y) * X + x;
                const uint64_t a = in ? (uint64_t)A[p] : 0ull, b = in ? (uint64_t)B[p] : 0ull;
                const bool valid = in && !(with_ignore && b == ignore);
                if (valid) over |= ((a >> 32) ? 1u : 0u) | ((b >> 32) ? 2u : 0u);
                const uint64_t key = ((uint64_t)(uint32_t)a << 32) | (uint32_t)b;
                const uint64_t prev = shfl_up_u64(key);
                const bool pvalid = __shfl_up((int)valid, 1, WAVE) != 0;
                const bool head = valid && (lane == 0 || !pvalid || prev != key);
                // a run ends before the next head or skipped lane
                const uint64_t bound = __ballot(head || !valid);
                bool direct = false;
                uint32_t run = 0;
                if (head) {
                    const uint64_t above = lane == WAVE - 1 ? 0ull : bound >> (lane + 1);
                    run = above ? (uint32_t)__ffsll((unsigned long long)above) : (uint32_t)(WAVE - lane);
                    direct = true;
                    if (key != EMPTY_KEY) {   // (the one pair that looks like a free slot goes direct)
                        uint32_t h = hash_key(key) & (OV_CAP - 1);
                        for (int q = 0; q < OV_PROBES; ++q) {
                            uint64_t cur = tkey[h];
                            if (cur == EMPTY_KEY) {
                                cur = atomicCAS((unsigned long long*)&tkey[h], (unsigned long long)EMPTY_KEY,
                                                (unsigned long long)key);
                                if (cur == EMPTY_KEY) {
                                    atomicAdd(&used, 1u);
                                    cur = key;
                                }
                            }
                            if (cur == key) {
                                atomicAdd(&tcnt[h], run);
                                direct = false;
                                break;
                            }
                            h = (h + 1) & (OV_CAP - 1);
                        }
                    }
                }
                const uint64_t dm = __ballot(direct);
                if (dm) {
                    const uint32_t n = (uint32_t)__popcll(dm);
                    const uint32_t rank =
                        __builtin_amdgcn_mbcnt_hi((uint32_t)(dm >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)dm, 0));
                    unsigned long long b0 = 0;
                    if (lane == 0) {
                        b0 = atomicAdd(&C->n_records, (unsigned long long)n);
                        atomicAdd(&C->n_direct, (unsigned long long)n);
                    }
                    b0 = bcast0_u64(b0);
                    if (direct && b0 + rank < (unsigned long long)cap) {
                        CTG_IDX(b0 + rank, cap);
                        rkey[b0 + rank] = key;
                        rcnt[b0 + rank] = run;
                    }
                }
            }
        }
        __syncthreads();
        if (used > OV_CAP / 2 || zs + OV_THREADS / WAVE >= OV_TILE_Z) {   // (uniform: read after the barrier)
            if (tid == 0) {
                base = used ? atomicAdd(&C->n_records, (unsigned long long)used) : 0ull;
                wpos = 0;
            }
            __syncthreads();
            // compaction order is irrelevant (sorted afterwards)
            for (int e = tid; e < OV_CAP; e += OV_THREADS) {
                const uint64_t k = tkey[e];
                const bool live = k != EMPTY_KEY;
                const uint64_t m = __ballot(live);
                if (m) {
                    const uint32_t rank =
                        __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0));
                    uint32_t w0 = 0;
                    if (lane == 0) w0 = atomicAdd(&wpos, (uint32_t)__popcll(m));
                    w0 = __shfl(w0, 0, WAVE);
                    if (live) {
                        const unsigned long long slot = base + w0 + rank;
                        if (slot < (unsigned long long)cap) {
                            CTG_IDX(slot, cap);
                            rkey[slot] = k;
                            rcnt[slot] = tcnt[e];
                        }
                        tkey[e] = EMPTY_KEY;
                        tcnt[e] = 0;
                    }
                }
            }
            __syncthreads();
            if (tid == 0) used = 0;
            __syncthreads();
        }
    }
    for (int o = 32; o > 0; o >>= 1) over |= (uint32_t)__shfl_xor((int)over, o, WAVE);
    if (lane == 0 && over) atomicOr(&C->label_overflow, (unsigned long long)over);
}

template <typename LabelT, typename ValueT>
static hipError_t launch_overlap_scan_t(const void* A, const void* B, const int64_t* shape, const int64_t* b,
                                        const int64_t* e, int with_ignore, uint64_t ignore, uint64_t* rkey,
                                        uint32_t* rcnt, int64_t cap, Counters* C, hipStream_t s) {
    const int64_t gx = (e[2] - b[2] + WAVE - 1) / WAVE, gy = (e[1] - b[1] + TILE_Y - 1) / TILE_Y,
                  gz = (e[0] - b[0] + OV_TILE_Z - 1) / OV_TILE_Z;
    if (gx > 0x7FFFFFFFll || gy > 65535 || gz > 65535) return hipErrorInvalidValue;
    hipLaunchKernelGGL((k_overlap_scan<LabelT, ValueT>), dim3((unsigned)gx, (unsigned)gy, (unsigned)gz),
                       dim3(OV_THREADS), 0, s, (const LabelT*)A, (const ValueT*)B, shape[1], shape[2], b[0], b[1],
                       b[2], e[0], e[1], e[2], with_ignore, ignore, rkey, rcnt, cap, C);
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

// Record i of the sorted list belongs to table row scan[i].lo - 1 of node
// scan[i].hi - 1.  A wave sums the counts of its 64 records per row (segmented
// suffix sums by shuffles; u64: merged counts pass 2^32) and the first lane of
// every segment adds the sum to the row -- one atomic per (wave, row), none
// contended unless a row spans waves.  counts is zeroed before the launch.
template <typename CountT>
__global__ __launch_bounds__(256) void k_overlap_runs(int64_t n, const uint64_t* __restrict__ key,
                                                      const CountT* __restrict__ cnt,
                                                      const uint64_t* __restrict__ scan, uint64_t* __restrict__ pairs,
                                                      unsigned long long* __restrict__ counts,
                                                      uint64_t* __restrict__ nodes, int64_t* __restrict__ row_off,
                                                      int64_t E, int64_t N) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = threadIdx.x & (WAVE - 1);
    const bool in = i < n;
    const uint64_t sc = in ? scan[i] : 0ull, sp = (in && i) ? scan[i - 1] : 0ull;
    const uint32_t seg = in ? (uint32_t)sc - 1u : 0xFFFFFFFFu;   // (rows < 2^32 - 1: the record limit)
    uint64_t v = in ? (uint64_t)cnt[i] : 0ull;
    for (int o = 1; o < WAVE; o <<= 1) {
        const uint64_t vo = shfl_down_u64(v, o);
        const uint32_t so = __shfl_down(seg, o, WAVE);
        if (lane + o < WAVE && so == seg) v += vo;
    }
    const uint32_t sprev = __shfl_up(seg, 1, WAVE);
    if (!in) return;
    if (lane == 0 || sprev != seg) {
        CTG_IDX(seg, E);
        atomicAdd(&counts[seg], (unsigned long long)v);
    }
    const uint64_t k = key[i];
    if ((uint32_t)sc != (uint32_t)sp) {
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

static dim3 grid_for(int64_t n) { return dim3((unsigned)((n + 255) / 256)); }

// n (key, count) records -> the result's table: sort by key, number the runs,
// sum them.  n in (0, 2^32 - 1).
template <typename CountT>
static hipError_t overlap_reduce_t(Workspace& w, const uint64_t* key, const CountT* cnt, int64_t n, hipStream_t s,
                                   ctg_result* r) {
    Ev ev{w, s};
    DevBuf<uint64_t> ks((size_t)n * 8), flags((size_t)n * 8), scan((size_t)n * 8);
    DevBuf<CountT> cs((size_t)n * sizeof(CountT));
    if (!ks || !flags || !scan || !cs) return hipErrorOutOfMemory;
    CTG_TRY(with_temp(w.temp, [&](void* t, size_t& tb) {
        return rocprim::radix_sort_pairs(t, tb, key, ks.p, cnt, cs.p, (size_t)n, 0u, 64u, s);
    }));
    ev.mark(3);
    hipLaunchKernelGGL(k_overlap_heads, grid_for(n), dim3(256), 0, s, n, ks.p, flags.p);
    CTG_TRY(hipGetLastError());
    CTG_TRY(with_temp(w.temp, [&](void* t, size_t& tb) {
        return rocprim::inclusive_scan(t, tb, flags.p, scan.p, (size_t)n, rocprim::plus<uint64_t>(), s);
    }));
    uint64_t last = 0;
    CTG_TRY(hipMemcpyAsync(&last, scan.p + (n - 1), 8, hipMemcpyDeviceToHost, s));
    CTG_TRY(hipStreamSynchronize(s));
    flags.reset();
    const int64_t E = (int64_t)(uint32_t)last, N = (int64_t)(last >> 32);
    ev.mark(4);
    DevBuf<uint64_t> pairs((size_t)E * 16), counts((size_t)E * 8), nodes((size_t)N * 8);
    DevBuf<int64_t> row_off((size_t)(N + 1) * 8);
    if (!pairs || !counts || !nodes || !row_off) return hipErrorOutOfMemory;
    CTG_TRY(hipMemsetAsync(counts.p, 0, (size_t)E * 8, s));
    hipLaunchKernelGGL(k_overlap_runs<CountT>, grid_for(n), dim3(256), 0, s, n, ks.p, cs.p, scan.p, pairs.p,
                       (unsigned long long*)counts.p, nodes.p, row_off.p, E, N);
    CTG_TRY(hipGetLastError());
    ev.mark(5);
    dev_free(r->edges);
    dev_free(r->nodes);
    dev_free(r->counts);
    dev_free(r->row_off);
    r->edges = pairs.release();
    r->counts = counts.release();
    r->nodes = nodes.release();
    r->row_off = row_off.release();
    r->n_edges = E;
    r->n_nodes = N;
    return hipSuccess;
}

hipError_t overlap_reduce(Workspace& w, const uint64_t* key, const uint64_t* cnt, int64_t n, hipStream_t s,
                          ctg_result* r) {
    return overlap_reduce_t<uint64_t>(w, key, cnt, n, s, r);
}

hipError_t overlap_tables(Workspace& w, const void* A, int abits, const void* B, int bbits, const int64_t* shape,
                          const int64_t* b, const int64_t* e, int with_ignore, uint64_t ignore, hipStream_t s,
                          ctg_result* r, unsigned* overflow) {
    *overflow = 0;
    Ev ev{w, s};
    const int64_t nb = (e[0] - b[0]) * (e[1] - b[1]) * (e[2] - b[2]);
    // a record per voxel at most; coarse labellings need a small fraction of that
    int64_t cap = std::min<int64_t>(nb, std::max<int64_t>(1 << 12, nb / 16));
    for (int attempt = 0; attempt < 3; ++attempt) {
        DevBuf<uint64_t> rkey((size_t)cap * 8);
        DevBuf<uint32_t> rcnt((size_t)cap * 4);
        if (!rkey || !rcnt) return hipErrorOutOfMemory;
        CTG_TRY(hipMemsetAsync(w.counters, 0, sizeof(Counters), s));
        ev.mark(0);
        CTG_TRY(launch_overlap_scan(A, abits, B, bbits, shape, b, e, with_ignore, ignore, rkey, rcnt, cap,
                                    w.counters, s));
        ev.mark(1);
        ev.mark(2);
        CTG_TRY(hipMemcpyAsync(w.counters_host, w.counters, sizeof(Counters), hipMemcpyDeviceToHost, s));
        CTG_TRY(hipStreamSynchronize(s));
        if (w.counters_host->label_overflow) {
            *overflow = (unsigned)w.counters_host->label_overflow;
            return hipSuccess;
        }
        const int64_t m = (int64_t)w.counters_host->n_records;
        if (m > cap) {
            // which heads miss the table depends on the order of arrival, so a
            // second run may count a few more: the third gets a slot per voxel
            cap = attempt == 0 ? std::min<int64_t>(nb, m + m / 8 + 1024) : nb;
            continue;
        }
        if (m >= 0xFFFFFFFFll) return hipErrorInvalidValue;   // (the API refuses boxes that large)
        r->n_records = m;
        r->n_direct = (int64_t)w.counters_host->n_direct;
        if (m == 0) {   // every voxel ignored: the caller's empty placeholders stay
            for (int i = 3; i <= 6; ++i) ev.mark(i);
            return hipSuccess;
        }
        CTG_TRY(overlap_reduce_t<uint32_t>(w, rkey, rcnt, m, s, r));
        ev.mark(6);
        return hipSuccess;
    }
    return hipErrorOutOfMemory;   // (unreachable: the third attempt holds every voxel)
}

hipError_t launch_overlap_heads(int64_t n, const uint64_t* key, uint64_t* flags, hipStream_t s) {
    hipLaunchKernelGGL(k_overlap_heads, grid_for(n), dim3(256), 0, s, n, key, flags);
    return hipGetLastError();
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
