// Applying a node assignment to a label volume: out[i] = A(labels[i] + off),
// zeros unshifted.  Replaces the array work of write/write.py: the
// `seg[mask] += off` of write.py:194-200 with nifty.tools.take (write.py:166,
// a dense table) or np.unique + a dict + nifty.tools.takeDict
// (write.py:170-181, a sparse one), and the nine other takeDict callers.
//
//   k_take_build   (key, value) pairs -> the hash table of ctg_take.h, one
//                  insert per thread; counts duplicates, folds the largest value
//   k_take_max     the largest value of a dense table
//   k_take         the map itself over a list of segments (one per block of a
//                  job, each with its label offset)
//
// k_take is elementwise and memory bound: 8 B read and 8 B written per voxel
// (4 B read with uint32 labels, nothing written in the check-only form) plus
// the gather from the table.  A workgroup takes one chunk of TAKE_CHUNK voxels
// of one segment, which it finds by a binary search of the host-built chunk
// prefix (as k_unique_blocks finds its block).  A lane takes two consecutive
// voxels per step with one 16-byte load and one 16-byte store (8-byte loads
// for uint32 labels); pairs are aligned in memory, so where a segment starts
// or ends on the odd half of a pair that voxel goes alone, in the 8-byte form.
// The volume streams through once: its loads and stores are nontemporal, which
// leaves the L2 to the table.
//
// Sparse lookups collapse runs, as the tile-table scans do: equal consecutive
// labels (in voxel order across the lanes of a wave, two per lane) probe once.
// A lane probes for its first voxel only where the lane below ended on another
// label, and for its second only where it differs from the first; every other
// voxel takes the value of the nearest lane below that probed (the highest
// such bit of the ballot below the lane) with a ds_bpermute.  A run stops at
// the wave edge.  Dense lookups do not collapse: see DESIGN.md 5, "Write".
//
// Every buffer here is call-sized and comes from the pool (DevBuf); nothing
// touches the workspace's record or sort buffers, so a CTG_DEFER_STATS handle
// stays valid across these calls.
#include <hip/hip_runtime.h>

#include "ctg_internal.h"
#include "ctg_take.h"

namespace ctg {

constexpr int TAKE_THREADS = 256;
static_assert(TAKE_CHUNK % (2 * TAKE_THREADS) == 0, "a chunk is whole steps of the workgroup");

typedef unsigned long long u64x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ uint64_t umax(uint64_t a, uint64_t b) { return a > b ? a : b; }
__device__ __forceinline__ uint64_t umin(uint64_t a, uint64_t b) { return a < b ? a : b; }
__device__ __forceinline__ uint64_t shfl_u64(uint64_t v, int src) {
    const uint32_t lo = __shfl((uint32_t)v, src, WAVE), hi = __shfl((uint32_t)(v >> 32), src, WAVE);
    return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ uint64_t shfl_xor_u64(uint64_t v, int o) {
    const uint32_t lo = __shfl_xor((uint32_t)v, o, WAVE), hi = __shfl_xor((uint32_t)(v >> 32), o, WAVE);
    return ((uint64_t)hi << 32) | lo;
}

__global__ __launch_bounds__(256) void k_take_build(const uint64_t* __restrict__ keys,
                                                    const uint64_t* __restrict__ vals, int64_t n, uint64_t* t,
                                                    uint64_t cap, unsigned long long* stat) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool in = i < n;
    int dup = 0;
    uint64_t v = 0;
    if (in) {
        v = vals[i];
        dup = take_insert(
            t, cap, keys[i], v,
            [](uint64_t* p, uint64_t expect, uint64_t want) {
                return (uint64_t)atomicCAS((unsigned long long*)p, (unsigned long long)expect, (unsigned long long)want);
            },
            [](uint64_t* p) { return (uint64_t)atomicAdd((unsigned long long*)p, 1ull); });
    }
    const uint64_t dm = __ballot(dup != 0);
    for (int o = 32; o > 0; o >>= 1) v = umax(v, shfl_xor_u64(v, o));
    if ((threadIdx.x & (WAVE - 1)) == 0) {
        if (dm) atomicAdd(&stat[0], (unsigned long long)__popcll(dm));
        if (v) atomicMax(&stat[1], (unsigned long long)v);
    }
}

__global__ __launch_bounds__(256) void k_take_max(const uint64_t* __restrict__ table, int64_t n,
                                                  unsigned long long* stat) {
    uint64_t v = 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        v = umax(v, table[i]);
    for (int o = 32; o > 0; o >>= 1) v = umax(v, shfl_xor_u64(v, o));
    if ((threadIdx.x & (WAVE - 1)) == 0 && v) atomicMax(&stat[1], (unsigned long long)v);
}

// the two labels at L[i], L[i + 1] (both inside the chunk: i is pair-aligned)
__device__ __forceinline__ void load_pair(const uint64_t* L, int64_t i, uint64_t* a, uint64_t* b) {
    const u64x2 v = __builtin_nontemporal_load((const u64x2*)(L + i));
    *a = v.x;
    *b = v.y;
}
__device__ __forceinline__ void load_pair(const uint32_t* L, int64_t i, uint64_t* a, uint64_t* b) {
    const u32x2 v = __builtin_nontemporal_load((const u32x2*)(L + i));
    *a = v.x;
    *b = v.y;
}

// A(l + off) into *v; true where it is missing (out of range, absent, or the
// shift wrapped), and *v is then the shifted label
template <bool DENSE>
__device__ __forceinline__ bool take_one(const TakeArgs& A, uint64_t l, uint64_t off, uint64_t* v) {
    const uint64_t s = l + (l ? off : 0ull);
    *v = s;
    if (s < l) return true;   // wrapped past 2^64
    if constexpr (DENSE) {
        if (s >= A.size) return true;
        *v = A.table[s];
        return false;
    } else {
        uint64_t val;
        if (!take_lookup(A.table, A.size, s, &val)) return true;
        *v = val;
        return false;
    }
}

// LabelT: uint64_t or uint32_t; DENSE: table[s], else the hash table;
// COLLAPSE: runs probe once; WRITE: false is the check-only form, which holds
// no store instruction
template <typename LabelT, bool DENSE, bool COLLAPSE, bool WRITE>
__global__ __launch_bounds__(TAKE_THREADS) void k_take(const TakeArgs A) {
    // the segment of this workgroup: prefix[k] <= blockIdx.x < prefix[k + 1] (wave-uniform)
    const uint32_t t = blockIdx.x;
    int k = 0, khi = A.n_seg;
    while (khi - k > 1) {
        const int mid = (k + khi) >> 1;
        if (A.prefix[mid] <= t) k = mid;
        else khi = mid;
    }
    const uint64_t off = A.seg_off[k];
    const int64_t lo = A.seg_begin[k] + (int64_t)(t - A.prefix[k]) * TAKE_CHUNK;
    const int64_t se = A.seg_begin[k + 1], hi = se < lo + TAKE_CHUNK ? se : lo + TAKE_CHUNK;
    // pairs are aligned in memory: the first may hold the voxel below lo, which is not ours
    const int64_t base = lo - ((lo + A.par) & 1);
    const int64_t span = hi - base;
    const LabelT* L = (const LabelT*)A.labels;   // (no __restrict__: in place, out is the same array)
    const int lane = threadIdx.x & (WAVE - 1);
    uint32_t nz = 0;
    uint64_t nmiss = 0, first = ~0ull;
    for (int64_t p0 = threadIdx.x - lane; 2 * p0 < span; p0 += TAKE_THREADS) {   // (wave-uniform trip count)
        const int64_t i = base + 2 * (p0 + lane);
        const bool in0 = i >= lo && i < hi, in1 = i + 1 < hi;
        uint64_t l0 = 0, l1 = 0;
        if (in0 && in1) load_pair(L, i, &l0, &l1);
        else if (in0) l0 = __builtin_nontemporal_load(L + i);
        else if (in1) l1 = __builtin_nontemporal_load(L + i + 1);
        uint64_t v0 = 0, v1 = 0;
        bool m0 = false, m1 = false;
        if constexpr (COLLAPSE) {
            // a lane with one voxel holds it twice; the lanes with voxels are a prefix of the wave
            const bool lv = in0 || in1;
            const uint64_t e0 = in0 ? l0 : l1, e1 = in1 ? l1 : l0;
            const uint64_t below = shfl_up_u64(e1);
            const bool head = lv && (lane == 0 || below != e0), change = lv && e1 != e0;
            if (head) m0 = take_one<DENSE>(A, e0, off, &v0);
            if (change) m1 = take_one<DENSE>(A, e1, off, &v1);
            // what this lane hands up: its last voxel's value, where it probed for it or for the first
            const uint64_t probed = __ballot(head || change) & ((1ull << lane) - 1ull);
            const int src = probed ? 63 - __clzll((long long)probed) : 0;
            const uint64_t vs = shfl_u64(change ? v1 : v0, src);
            const int ms = __shfl((int)(change ? m1 : m0), src, WAVE);
            if (!head) {
                v0 = vs;
                m0 = ms != 0;
            }
            if (!change) {
                v1 = v0;
                m1 = m0;
            }
        } else {
            if (in0) m0 = take_one<DENSE>(A, l0, off, &v0);
            if (in1) m1 = take_one<DENSE>(A, l1, off, &v1);
        }
        if constexpr (WRITE) {
            if (in0 && in1 && A.wide_store) {
                u64x2 o;
                o.x = v0;
                o.y = v1;
                __builtin_nontemporal_store(o, (u64x2*)(A.out + i));
            } else {
                if (in0) __builtin_nontemporal_store((unsigned long long)v0, (unsigned long long*)(A.out + i));
                if (in1) __builtin_nontemporal_store((unsigned long long)v1, (unsigned long long*)(A.out + i + 1));
            }
        }
        nz += (uint32_t)__popcll(__ballot(in0 && l0 != 0)) + (uint32_t)__popcll(__ballot(in1 && l1 != 0));
        // the smallest missing label: shifted, or as it was where the shift wrapped
        if (in0 && m0) {
            ++nmiss;
            first = umin(first, v0 < l0 ? l0 : v0);
        }
        if (in1 && m1) {
            ++nmiss;
            first = umin(first, v1 < l1 ? l1 : v1);
        }
    }
    if (__ballot(nmiss != 0)) {   // (rare: a wave-uniform branch)
        for (int o = 32; o > 0; o >>= 1) {
            nmiss += shfl_xor_u64(nmiss, o);
            first = umin(first, shfl_xor_u64(first, o));
        }
        if (lane == 0) {
            atomicAdd(&A.missing[0], (unsigned long long)nmiss);
            atomicMin(&A.missing[1], (unsigned long long)first);
        }
    }
    // (one of nz_slots counters per segment, by workgroup: adds to one address queue up behind each other)
    if (lane == 0 && nz)
        atomicAdd(&A.seg_nonzero[(int64_t)k * A.nz_slots + (int64_t)(t & (uint32_t)(A.nz_slots - 1))],
                  (unsigned long long)nz);
}

hipError_t launch_take_build(const uint64_t* keys, const uint64_t* vals, int64_t n, uint64_t* table, uint64_t cap,
                             unsigned long long* stat, hipStream_t s) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_take_build, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, keys, vals, n, table, cap,
                       stat);
    return hipGetLastError();
}

hipError_t launch_take_max(const uint64_t* table, int64_t n, unsigned long long* stat, hipStream_t s) {
    if (n == 0) return hipSuccess;
    const int64_t blocks = std::min<int64_t>((n + 255) / 256, 4096);
    hipLaunchKernelGGL(k_take_max, dim3((unsigned)blocks), dim3(256), 0, s, table, n, stat);
    return hipGetLastError();
}

// Dense lookups do not collapse runs: the same-address lanes of the gather coalesce anyway, and the
// shuffles cost more than they save (1024^3: 3.18 against 3.46 ms, DESIGN.md 5 "Write")
constexpr bool TAKE_DENSE_COLLAPSE = false;

template <typename LabelT, bool DENSE, bool COLLAPSE>
static void launch_take_w(const TakeArgs& A, uint32_t chunks, hipStream_t s) {
    if (A.out) hipLaunchKernelGGL((k_take<LabelT, DENSE, COLLAPSE, true>), dim3(chunks), dim3(TAKE_THREADS), 0, s, A);
    else hipLaunchKernelGGL((k_take<LabelT, DENSE, COLLAPSE, false>), dim3(chunks), dim3(TAKE_THREADS), 0, s, A);
}

hipError_t launch_take(const TakeArgs& A, int label_bits, bool dense, uint32_t chunks, hipStream_t s) {
    if (chunks == 0) return hipSuccess;
    if (dense) {
        if (label_bits == 32) launch_take_w<uint32_t, true, TAKE_DENSE_COLLAPSE>(A, chunks, s);
        else launch_take_w<uint64_t, true, TAKE_DENSE_COLLAPSE>(A, chunks, s);
    } else {
        if (label_bits == 32) launch_take_w<uint32_t, false, true>(A, chunks, s);
        else launch_take_w<uint64_t, false, true>(A, chunks, s);
    }
    return hipGetLastError();
}

}  // namespace ctg
