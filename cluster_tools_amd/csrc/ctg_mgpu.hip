// Multi-GPU combine of the z-slab partial tables: the device
// side of one rank's exchange step, between RCCL collectives that the host
// layer (cluster_tools_amd/dist.py) issues over torch.distributed.
//
// The reference combines per-block results in two tasks --
// graph/merge_sub_graphs.py:130-135 (ndist.mergeSubgraphs) and
// features/merge_edge_features.py:141-147 (ndist.mergeFeatureBlocks) -- by
// re-reading every block's chunks.  Here every rank holds the sorted partial
// table of its slab (edges, 10 features and the mergeable wide statistics of
// each edge, CTG_KEEP_STATS) and the global table is range-partitioned by the
// lower label u:
//
//   ctg_mgpu_sample  an evenly spaced sample of this rank's u column
//                    (all-gathered by the host)
//   ctg_mgpu_split   range splitters from the gathered samples (exact integer
//                    weights, so every rank derives the same ones) and the
//                    rows / node ids this rank sends to every rank
//                    (all-gathered by the host: every rank then knows every
//                    segment size of the all_to_all)
//   ctg_mgpu_pack    the rows and node ids for the other ranks, one segment
//                    per destination, in one launch
//   ctg_mgpu_merge   after the all_to_all: the received rows are merged with
//                    this rank's own range -- stats of equal keys combined
//                    (Chan's rule on the shifted sums, histograms added),
//                    features re-finalised only for those keys, every other
//                    own row kept as the local call computed it.  With nothing
//                    received the own range IS the shard (no kernel, no copy).
#include <algorithm>
#include <cstring>

#include <rocprim/rocprim.hpp>

#include "ctg_internal.h"
#include "ctg_stats.h"

namespace ctg {

constexpr int MS = CTG_MGPU_SAMPLES;
constexpr int ROW = CTG_MGPU_ROW_WORDS;       // int64 words per exchanged row
constexpr uint64_t SIGN = 1ull << 63;         // u ^ SIGN: unsigned order as int64 order

// ---------------------------------------------------------------------------
// sample and split
// ---------------------------------------------------------------------------
__global__ void k_mgpu_sample(const uint64_t* __restrict__ edges, int64_t E, int64_t* __restrict__ meta) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < MS) meta[i] = E ? (int64_t)(edges[2 * ((int64_t)i * E / MS)] ^ SIGN) : 0;
    if (i == MS) meta[MS] = E;
}

// The one binary search: the first i of [0, n) that does not come before the
// sought position -- before(i) holds on a prefix of the range.  A lower bound
// asks "element i < x", an upper bound "element i <= x".
template <class I, class Before>
__device__ __forceinline__ I first_not(I n, Before before) {
    I lo = 0, hi = n;
    while (lo < hi) {
        const I mid = (lo + hi) >> 1;
        if (before(mid)) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// Splitters: sample j of rank r (value v, sorted per rank) stands for
// count_r / MS rows.  In the total order (v, r, j) its cumulative weight,
// scaled by MS to integers, is CW = sum_r' count_r' * c_r', with c_r' the
// samples of rank r' at or before it (r' < r: <= v; r' > r: < v; r' = r: j+1).
// Splitter k (1..W-1) is the v of the one sample whose weight interval
// (CW - count_r, CW] holds total * MS * k / W -- exact integer arithmetic, so
// every rank finds the same splitters from the same gathered samples, and no
// atomics are needed (the crossing sample writes its splitter alone).
__global__ void k_mgpu_splitters(const int64_t* __restrict__ meta_all, int world, uint64_t* __restrict__ spl) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= world * MS) return;
    const int r = e / MS, j = e % MS;
    const uint64_t cnt_r = (uint64_t)meta_all[(int64_t)r * (MS + 1) + MS];
    if (cnt_r == 0) return;
    const int64_t v = meta_all[(int64_t)r * (MS + 1) + j];
    uint64_t cw = 0, total = 0;
    for (int q = 0; q < world; ++q) {
        const int64_t* row = meta_all + (int64_t)q * (MS + 1);
        const uint64_t cq = (uint64_t)row[MS];
        total += cq;
        if (cq == 0) continue;
        const int c = q < r   ? first_not(MS, [&](int i) { return row[i] <= v; })
                      : q > r ? first_not(MS, [&](int i) { return row[i] < v; })
                              : j + 1;
        cw += cq * (uint64_t)c;
    }
    const uint64_t lo = (cw - cnt_r) * (uint64_t)world, hi = cw * (uint64_t)world;
    for (int k = 1; k < world; ++k) {
        const uint64_t t = total * (uint64_t)MS * (uint64_t)k;
        if (lo < t && t <= hi) spl[k - 1] = (uint64_t)v ^ SIGN;
    }
}

// first row of a sorted (u,v) table (stride words per row) whose u >= x
__device__ __forceinline__ int64_t lower_u(const uint64_t* col, int stride, int64_t n, uint64_t x) {
    return first_not(n, [&](int64_t i) { return col[i * stride] < x; });
}

// rows / node ids of this rank that fall in every rank's u range
// [spl[d-1], spl[d]) -> counts[2d], counts[2d+1]
__global__ void k_mgpu_bounds(const uint64_t* __restrict__ edges, int64_t E, const uint64_t* __restrict__ nodes,
                              int64_t N, const uint64_t* __restrict__ spl, int world, int64_t* __restrict__ counts) {
    const int d = threadIdx.x;
    if (d >= world) return;
    const int64_t e0 = d == 0 ? 0 : lower_u(edges, 2, E, spl[d - 1]);
    const int64_t e1 = d == world - 1 ? E : lower_u(edges, 2, E, spl[d]);
    const int64_t n0 = d == 0 ? 0 : lower_u(nodes, 1, N, spl[d - 1]);
    const int64_t n1 = d == world - 1 ? N : lower_u(nodes, 1, N, spl[d]);
    counts[2 * d] = max(e1 - e0, (int64_t)0);
    counts[2 * d + 1] = max(n1 - n0, (int64_t)0);
}

// ---------------------------------------------------------------------------
// pack: one segment per destination, rows then node ids (the segment tables,
// ExchangeSegs, and their lookup seg_of are ctg_plan.h's: exchange_plan)
// ---------------------------------------------------------------------------
// a row = (u, v, S1 bits, S2 bits, the 48-word wide record as 24 u64)
__global__ void k_mgpu_pack(ExchangeSegs S, const uint64_t* __restrict__ edges, const double2* __restrict__ sums,
                            const uint64_t* __restrict__ wide64, const uint64_t* __restrict__ nodes,
                            uint64_t* __restrict__ out) {
    const int64_t total = S.words();
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += (int64_t)gridDim.x * blockDim.x) {
        const int s = seg_of(S.w_off, S.n, i);
        const int64_t off = i - S.w_off[s], row_words = (S.row0[s + 1] - S.row0[s]) * ROW;
        uint64_t val;
        if (off < row_words) {
            const int64_t r = S.e_start[s] + off / ROW;
            const int w = (int)(off % ROW);
            if (w < 2) val = edges[2 * r + w];
            else if (!wide64) continue;   // CTG_DEFER_STATS: k_mgpu_pack_deferred writes the statistics
            else if (w < 4) {
                const double2 sm = sums[r];
                val = (uint64_t)__double_as_longlong(w == 2 ? sm.x : sm.y);
            } else {
                val = wide64[r * (WREC_WORDS / 2) + (w - 4)];
            }
        } else {
            val = nodes[S.n_start[s] + (off - row_words)];
        }
        out[i] = val;
    }
}

// CTG_DEFER_STATS: one thread per row to send -- its statistics rebuilt from
// its records (words 2..27 of the row; k_mgpu_pack writes the key words).
// Boundary maps only: every key is an edge (the reduce's need_adj 0 sets ADJ).
__global__ __launch_bounds__(256) void k_mgpu_pack_deferred(ExchangeSegs S, DeferredStats D,
                                                            uint64_t* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= S.rows()) return;
    const int s = seg_of(S.row0, S.n, i);
    const int64_t a = i - S.row0[s], r = S.e_start[s] + a;
    uint32_t h[NSLOTS];
#pragma unroll
    for (int j = 0; j < NSLOTS; ++j) h[j] = 0;
    uint32_t cnt = 0, flags = ADJ_FLAG, mn = ORD_POS_INF, mx = ORD_NEG_INF;
    Moments mo;
    edge_from_records(D, r, h, cnt, flags, mn, mx, mo);
    uint32_t w[WREC_WORDS];
    wide_row(h, cnt, flags, mn, mx, mo, w);
    uint64_t* o = out + S.w_off[s] + a * ROW;
    o[2] = (uint64_t)__double_as_longlong(mo.S1);
    o[3] = (uint64_t)__double_as_longlong(mo.S2);
#pragma unroll
    for (int t = 0; t < WREC_WORDS / 2; ++t) o[4 + t] = (uint64_t)w[2 * t] | ((uint64_t)w[2 * t + 1] << 32);
}

// ---------------------------------------------------------------------------
// merge
// ---------------------------------------------------------------------------
__device__ __forceinline__ bool key_lt(uint64_t au, uint64_t av, uint64_t bu, uint64_t bv) {
    return au < bu || (au == bu && av < bv);
}

__device__ __forceinline__ const uint64_t* recv_row(const ExchangeSegs& S, const uint64_t* recv, int s, int64_t a) {
    return recv + S.w_off[s] + a * ROW;
}

// rows of segment q with key < (u,v) (lower) or <= (upper)
__device__ __forceinline__ int64_t seg_rank(const ExchangeSegs& S, const uint64_t* recv, int q, uint64_t u,
                                            uint64_t v, bool upper) {
    return first_not(S.row0[q + 1] - S.row0[q], [&](int64_t i) {
        const uint64_t* p = recv_row(S, recv, q, i);
        return upper ? !key_lt(u, v, p[0], p[1]) : key_lt(p[0], p[1], u, v);
    });
}

// Received rows in one sorted order without a sort: every source's segment is
// sorted, so row a of segment s lands at a + (rows of the other segments that
// precede it; ties go to the lower source).  order[pos] = global row index.
__global__ void k_mgpu_order(ExchangeSegs S, const uint64_t* __restrict__ recv, uint32_t* __restrict__ order,
                             uint64_t* __restrict__ skeys) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= S.rows()) return;
    const int s = seg_of(S.row0, S.n, j);
    const int64_t a = j - S.row0[s];
    const uint64_t* p = recv_row(S, recv, s, a);
    const uint64_t u = p[0], v = p[1];
    int64_t pos = a;
    for (int q = 0; q < S.n; ++q)
        if (q != s) pos += seg_rank(S, recv, q, u, v, q < s);
    order[pos] = (uint32_t)j;
    skeys[2 * pos] = u;
    skeys[2 * pos + 1] = v;
}

__global__ void k_mgpu_heads(int64_t M, const uint64_t* __restrict__ skeys, uint32_t* __restrict__ head) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= M) return;
    head[p] = (p == 0 || skeys[2 * p] != skeys[2 * p - 2] || skeys[2 * p + 1] != skeys[2 * p - 1]) ? 1u : 0u;
}

// first sorted position of every run (rid = exclusive scan of the heads); K
// (the unique received keys) in *nK
__global__ void k_mgpu_runs(int64_t M, const uint32_t* __restrict__ head, const uint32_t* __restrict__ rid,
                            uint32_t* __restrict__ run0, uint32_t* __restrict__ nK) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= M) return;
    if (head[p]) run0[rid[p]] = (uint32_t)p;
    if (p == M - 1) {
        const uint32_t K = rid[p] + head[p];
        *nK = K;
        run0[K] = (uint32_t)M;
    }
}

// position of (u,v) in a sorted (u,v) table of n rows: lower bound
__device__ __forceinline__ int64_t lower_uv(const uint64_t* t, int64_t n, uint64_t u, uint64_t v) {
    return first_not(n, [&](int64_t i) { return key_lt(t[2 * i], t[2 * i + 1], u, v); });
}

// One thread per unique received key: its own-range match (binary search),
// the combined statistics of the own row and every received row of the key,
// and the re-finalised feature row.
__global__ __launch_bounds__(256) void k_mgpu_combine(ExchangeSegs S, MergeIO io) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= (int64_t)*io.nK) return;
    CTG_IDX(*io.nK, S.rows() + 1);   // unique received keys within the received rows
    const uint32_t p0 = io.run0[k], p1 = io.run0[k + 1];
    CTG_IDX(p1, S.rows() + 1);
    CTG_IDX(p0, p1);
    const uint64_t u = io.skeys[2 * (int64_t)p0], v = io.skeys[2 * (int64_t)p0 + 1];
    const int64_t ins = lower_uv(io.own_edges, io.n_own, u, v);
    const bool found = ins < io.n_own && io.own_edges[2 * ins] == u && io.own_edges[2 * ins + 1] == v;
    uint32_t h[NSLOTS];
#pragma unroll
    for (int j = 0; j < NSLOTS; ++j) h[j] = 0;
    uint32_t cnt = 0, flags = 0, mn = ORD_POS_INF, mx = ORD_NEG_INF;
    Moments mo;
    uint32_t w[WREC_WORDS];
    if (found && io.defer.on) {   // the own row's records (boundary maps: every key an edge)
        flags = ADJ_FLAG;
        edge_from_records(io.defer, io.own_row0 + ins, h, cnt, flags, mn, mx, mo);
        io.touched[ins] = (uint32_t)k + 1u;
    } else if (found) {
        const uint4* q = reinterpret_cast<const uint4*>(io.own_wide + ins * WREC_WORDS);
#pragma unroll
        for (int j = 0; j < WREC_WORDS / 4; ++j) {
            const uint4 x = q[j];
            w[4 * j] = x.x; w[4 * j + 1] = x.y; w[4 * j + 2] = x.z; w[4 * j + 3] = x.w;
        }
        const double2 sm = io.own_sums[ins];
        add_wide(w, sm.x, sm.y, h, cnt, flags, mn, mx, mo);
        io.touched[ins] = (uint32_t)k + 1u;
    }
    for (uint32_t p = p0; p < p1; ++p) {
        const uint32_t j = io.order[p];
        CTG_IDX(j, S.rows());
        const int s = seg_of(S.row0, S.n, (int64_t)j);
        const uint64_t* r = recv_row(S, io.recv, s, (int64_t)j - S.row0[s]);
#pragma unroll
        for (int t = 0; t < WREC_WORDS / 2; ++t) {
            const uint64_t x = r[4 + t];
            w[2 * t] = (uint32_t)x;
            w[2 * t + 1] = (uint32_t)(x >> 32);
        }
        add_wide(w, __longlong_as_double((long long)r[2]), __longlong_as_double((long long)r[3]), h, cnt, flags,
                 mn, mx, mo);
    }
    io.mkeys[2 * k] = u;
    io.mkeys[2 * k + 1] = v;
    io.mkeep[k] = (!io.partial_adj || (flags & ADJ_FLAG)) ? 1u : 0u;
    io.mnew[k] = found ? 0u : 1u;
    io.mins[k] = ins;
    finalize_row(h, cnt, mn, mx, mo, io.scale, io.offset, io.mfeats + k * N_FEATURES);
}

// received keys absent from the own range (nrank = exclusive scan of mnew)
__device__ __forceinline__ uint32_t new_keys(const MergeIO& io, const uint32_t* nrank, int64_t K) {
    return K ? nrank[K - 1] + io.mnew[K - 1] : 0u;
}

// The merged-order slot of entry i of (own rows, then received keys): own row
// i -> i + (new keys below it); new key k = i - n_own -> (own rows below it) +
// (new keys before it).  Received keys that are not new have no slot.
__device__ __forceinline__ int64_t merged_slot(const MergeIO& io, const uint32_t* nrank, int64_t K, uint32_t n_new,
                                               int64_t i) {
    if (i >= io.n_own) return io.mins[i - io.n_own] + nrank[i - io.n_own];
    const int64_t b = K ? lower_uv(io.mkeys, K, io.own_edges[2 * i], io.own_edges[2 * i + 1]) : 0;
    return i + (b < K ? (int64_t)nrank[b] : (int64_t)n_new);
}

// the slot of every own row and every new received key, and its keep flag
__global__ void k_mgpu_slots(MergeIO io, const uint32_t* __restrict__ nrank, uint32_t* __restrict__ keep,
                             int64_t n_slots) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t K = (int64_t)*io.nK;
    const uint32_t n_new = new_keys(io, nrank, K);
    // slots past the merged table (the buffer is sized by the bound n_own + M)
    if (i >= io.n_own + (int64_t)n_new && i < n_slots) keep[i] = 0u;
    if (i == 0) CTG_IDX(io.n_own + (int64_t)n_new, n_slots + 1);
    if (i < io.n_own) {
        const uint32_t t = io.touched[i];
        const uint32_t kp = t ? io.mkeep[t - 1]
                              : ((!io.partial_adj || (io.own_wide[i * WREC_WORDS + 42] & ADJ_FLAG)) ? 1u : 0u);
        keep[merged_slot(io, nrank, K, n_new, i)] = kp;
    } else if (i < io.n_own + K && io.mnew[i - io.n_own]) {
        const int64_t slot = merged_slot(io, nrank, K, n_new, i);
        CTG_IDX(slot, n_slots);
        keep[slot] = io.mkeep[i - io.n_own];
    }
}

// rows to their final positions (fpos = exclusive scan of keep over the slots)
__global__ void k_mgpu_scatter(MergeIO io, const uint32_t* __restrict__ nrank, const uint32_t* __restrict__ keep,
                               const uint32_t* __restrict__ fpos, int64_t n_slots, uint64_t* __restrict__ out_e,
                               double* __restrict__ out_f, uint32_t* __restrict__ n_out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t K = (int64_t)*io.nK;
    if (i == 0) *n_out = n_slots ? fpos[n_slots - 1] + keep[n_slots - 1] : 0u;
    const uint64_t* ke;
    const double* kf;
    if (i < io.n_own) {
        const uint32_t t = io.touched[i];
        ke = io.own_edges + 2 * i;
        kf = t ? io.mfeats + (int64_t)(t - 1) * N_FEATURES : io.own_feats + i * N_FEATURES;
    } else if (i < io.n_own + K) {
        const int64_t k = i - io.n_own;
        if (!io.mnew[k]) return;
        ke = io.mkeys + 2 * k;
        kf = io.mfeats + k * N_FEATURES;
    } else {
        return;
    }
    const int64_t slot = merged_slot(io, nrank, K, new_keys(io, nrank, K), i);
    CTG_IDX(slot, n_slots);
    if (!keep[slot]) return;
    const int64_t f = fpos[slot];
    out_e[2 * f] = ke[0];
    out_e[2 * f + 1] = ke[1];
    const double2* s2 = reinterpret_cast<const double2*>(kf);
    double2* d2 = reinterpret_cast<double2*>(out_f + f * N_FEATURES);
#pragma unroll
    for (int j = 0; j < N_FEATURES / 2; ++j) d2[j] = s2[j];
}

// node ids of the own range and every received segment -> one list
__global__ void k_mgpu_node_list(ExchangeSegs S, const uint64_t* __restrict__ recv, const uint64_t* __restrict__ own,
                                 int64_t n_own, uint64_t* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_own + S.nodes()) return;
    if (i < n_own) {
        out[i] = own[i];
        return;
    }
    const int s = seg_of(S.node0, S.n, i - n_own);
    const int64_t a = i - n_own - S.node0[s];
    const int64_t rows = S.row0[s + 1] - S.row0[s];
    out[i] = recv[S.w_off[s] + rows * ROW + a];
}


// ---------------------------------------------------------------------------
// launchers (called from ctg_api_mgpu.hip; declared in ctg_internal.h)
// ---------------------------------------------------------------------------
static unsigned grid_of(int64_t n) { return (unsigned)std::max<int64_t>((n + 255) / 256, 1); }

static const uint64_t* u64(const int64_t* p) { return reinterpret_cast<const uint64_t*>(p); }

// exclusive prefix sum of n u32 (rocPRIM, the workspace's temp buffer)
static hipError_t excl_scan(GrowBuf& temp, const uint32_t* in, uint32_t* out, int64_t n, hipStream_t s) {
    if (n == 0) return hipSuccess;
    return with_temp(temp, [&](void* t, size_t& tb) {
        return rocprim::exclusive_scan(t, tb, in, out, 0u, (size_t)n, rocprim::plus<uint32_t>(), s);
    });
}

hipError_t mgpu_sample(const uint64_t* edges, int64_t E, int64_t* meta, hipStream_t s) {
    hipLaunchKernelGGL(k_mgpu_sample, dim3((MS + 1 + 255) / 256), dim3(256), 0, s, edges, E, meta);
    return hipGetLastError();
}

hipError_t mgpu_split(const uint64_t* edges, int64_t E, const uint64_t* nodes, int64_t N, const int64_t* meta_all,
                      int world, uint64_t* spl, int64_t* counts, hipStream_t s) {
    if (world > 1) {
        hipError_t e = hipMemsetAsync(spl, 0, (size_t)(world - 1) * 8, s);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(k_mgpu_splitters, dim3((world * MS + 255) / 256), dim3(256), 0, s, meta_all, world, spl);
    }
    hipLaunchKernelGGL(k_mgpu_bounds, dim3(1), dim3(CTG_MGPU_MAX_WORLD), 0, s, edges, E, nodes, N, spl, world,
                       counts);
    return hipGetLastError();
}

hipError_t mgpu_pack(const ctg_result* r, const ExchangeSegs& S, int64_t* send, hipStream_t s) {
    if (S.words() == 0) return hipSuccess;
    const bool defer = r->defer.on && !r->stats;
    const int64_t blocks = std::min<int64_t>((S.words() + 255) / 256, 8192);
    hipLaunchKernelGGL(k_mgpu_pack, dim3((unsigned)blocks), dim3(256), 0, s, S, r->edges, r->stat_sums,
                       defer ? nullptr : reinterpret_cast<const uint64_t*>(r->stats), r->nodes,
                       reinterpret_cast<uint64_t*>(send));
    if (defer && S.rows() > 0)
        hipLaunchKernelGGL(k_mgpu_pack_deferred, dim3((unsigned)((S.rows() + 255) / 256)), dim3(256), 0, s, S,
                           r->defer, reinterpret_cast<uint64_t*>(send));
    return hipGetLastError();
}

hipError_t mgpu_node_list(const ExchangeSegs& S, const int64_t* recv, const uint64_t* own, int64_t n_own,
                          uint64_t* out, hipStream_t s) {
    hipLaunchKernelGGL(k_mgpu_node_list, dim3(grid_of(n_own + S.nodes())), dim3(256), 0, s, S, u64(recv), own, n_own,
                       out);
    return hipGetLastError();
}

hipError_t mgpu_order(const ExchangeSegs& S, const int64_t* recv, uint32_t* order, uint64_t* skeys, hipStream_t s) {
    hipLaunchKernelGGL(k_mgpu_order, dim3(grid_of(S.rows())), dim3(256), 0, s, S, u64(recv), order, skeys);
    return hipGetLastError();
}

hipError_t mgpu_runs(Workspace& w, int64_t M, const uint64_t* skeys, uint32_t* head, uint32_t* rid, uint32_t* run0,
                     uint32_t* nK, hipStream_t s) {
    hipLaunchKernelGGL(k_mgpu_heads, dim3(grid_of(M)), dim3(256), 0, s, M, skeys, head);
    CTG_TRY(hipGetLastError());
    CTG_TRY(excl_scan(w.temp, head, rid, M, s));
    hipLaunchKernelGGL(k_mgpu_runs, dim3(grid_of(M)), dim3(256), 0, s, M, head, rid, run0, nK);
    return hipGetLastError();
}

hipError_t mgpu_combine(Workspace& w, const ExchangeSegs& S, const MergeIO& io, uint32_t* nrank, hipStream_t s) {
    hipLaunchKernelGGL(k_mgpu_combine, dim3(grid_of(S.rows())), dim3(256), 0, s, S, io);
    CTG_TRY(hipGetLastError());
    return excl_scan(w.temp, io.mnew, nrank, S.rows(), s);
}

hipError_t mgpu_slots(Workspace& w, const MergeIO& io, const uint32_t* nrank, int64_t n_slots, uint32_t* keep,
                      uint32_t* fpos, hipStream_t s) {
    hipLaunchKernelGGL(k_mgpu_slots, dim3(grid_of(n_slots)), dim3(256), 0, s, io, nrank, keep, n_slots);
    CTG_TRY(hipGetLastError());
    return excl_scan(w.temp, keep, fpos, n_slots, s);
}

hipError_t mgpu_scatter(const MergeIO& io, const uint32_t* nrank, const uint32_t* keep, const uint32_t* fpos,
                        int64_t n_slots, uint64_t* out_e, double* out_f, uint32_t* n_out, hipStream_t s) {
    hipLaunchKernelGGL(k_mgpu_scatter, dim3(grid_of(n_slots)), dim3(256), 0, s, io, nrank, keep, fpos, n_slots, out_e,
                       out_f, n_out);
    return hipGetLastError();
}

CTG_BOUNDS_TAKE(mgpu)

}  // namespace ctg
