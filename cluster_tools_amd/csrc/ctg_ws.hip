// Seeded watershed: the flood of a height map from seeds, as the minimum
// spanning forest of the box's grid graph with the seeded voxels contracted
// into one root (include/ctg.h: ctg_seeded_watershed).  Replaces
// vigra.analysis.watershedsNew(hmap, seeds=...) of
// watershed/watershed_from_seeds.py:143-204 and its other callers.  The order,
// the pick, the hook and the chase are ctg_ws.h's; the kernels here are the
// loops around them, a thread per voxel in box-linear order (x fastest, so a
// wave reads rows):
//
//   k_ws_init     every voxel its own root, flagged where its seed is not 0; the
//                 heights' keys and the NaN flag; the seeded voxels counted
//   k_ws_pick     <0> a seedless component's smallest (max, min) over its voxels'
//                 offers, by a 64-bit atomic minimum at its root; <1> the smallest
//                 edge id among the offers that tie on it, by a 32-bit one
//   k_ws_hook     a picking root's new entry (ws_hook) into its `best` word --
//                 not into parent, which the other roots' decisions still read
//   k_ws_apply    ... and from there into parent; the root's round words reset
//   k_ws_chase    every entry up its chain (ws_chase), agent-scope atomics only
//   k_ws_write    out[i] = the seed of i's root
//   k_ws_filter / k_ws_dropped   the size filter over a morphology table
//
// Each is a launch of its own: what one writes, the next reads (the L2s of two
// XCDs are not coherent within a launch).  Counters are summed per workgroup
// and added once: atomics to one address queue up behind each other.
#include <hip/hip_runtime.h>

#include "ctg_internal.h"
#include "ctg_ws.h"

namespace ctg {

namespace {

struct AgentLoad {
    __device__ uint32_t operator()(const uint32_t* p) const {
        return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
};

__device__ __forceinline__ WsBox box_of_args(const WsArgs& A) {
    return WsBox{{A.box.n[0], A.box.n[1], A.box.n[2]}, A.two_d};
}
__device__ __forceinline__ int64_t voxels_of(const WsArgs& A) { return (int64_t)A.box.n[0] * A.box.n[1] * A.box.n[2]; }
// the array element of box voxel i
__device__ __forceinline__ int64_t element_of(const WsArgs& A, uint32_t i) {
    const uint32_t x = i % A.box.n[2], y = (i / A.box.n[2]) % A.box.n[1], z = i / (A.box.n[1] * A.box.n[2]);
    return A.box.base + (int64_t)z * A.box.s_z + (int64_t)y * A.box.s_y + x;
}
__device__ __forceinline__ uint64_t seed_at(const WsArgs& A, int64_t e) {
    return A.seed_bits == 32 ? (uint64_t)((const uint32_t*)A.seeds)[e] : ((const uint64_t*)A.seeds)[e];
}

// the workgroup's sum of v, on thread 0
__device__ __forceinline__ unsigned long long block_sum(unsigned long long v) {
    __shared__ unsigned long long part[WS_THREADS / WAVE];
    for (int o = 32; o > 0; o >>= 1) v += shfl_down_u64(v, o);
    __syncthreads();   // (a second call reuses part)
    if ((threadIdx.x & (WAVE - 1)) == 0) part[threadIdx.x / WAVE] = v;
    __syncthreads();
    unsigned long long t = 0;
    if (threadIdx.x == 0)
        for (int k = 0; k < WS_THREADS / WAVE; ++k) t += part[k];
    return t;
}

}  // namespace

template <int KEYS>
__global__ __launch_bounds__(WS_THREADS) void k_ws_init(const WsArgs A) {
    const int64_t V = voxels_of(A);
    unsigned long long seeded = 0, nan = 0;
    for (int64_t i = (int64_t)blockIdx.x * WS_THREADS + threadIdx.x; i < V; i += (int64_t)gridDim.x * WS_THREADS) {
        const int64_t e = element_of(A, (uint32_t)i);
        const bool s = seed_at(A, e) != 0;
        seeded += s;
        A.parent[i] = s ? (uint32_t)i | WS_SEEDED : (uint32_t)i;
        A.best[i] = WS_NO_KEY;
        A.pick[i] = WS_NO_EDGE;
        if (KEYS) {
            const float h = A.hmap[e];
            nan += h != h;
            A.key[i] = ws_key(h);
        }
    }
    seeded = block_sum(seeded);
    nan = block_sum(nan);
    if (threadIdx.x == 0) {
        if (seeded) atomicAdd(&A.words[WS_W_SEEDED], seeded);
        if (nan) atomicOr(&A.words[WS_W_NAN], 1ull);
    }
}

template <int PASS>
__global__ __launch_bounds__(WS_THREADS) void k_ws_pick(const WsArgs A) {
    const int64_t V = voxels_of(A);
    const WsBox B = box_of_args(A);
    const uint32_t* __restrict__ parent = A.parent;
    const uint32_t* __restrict__ key = A.key;
    for (int64_t i = (int64_t)blockIdx.x * WS_THREADS + threadIdx.x; i < V; i += (int64_t)gridDim.x * WS_THREADS) {
        const uint32_t r = parent[i];
        if (r & WS_SEEDED) continue;   // finished
        const WsEdge e = ws_voxel_pick(
            B, (uint32_t)i, r, [&](uint32_t u) { return parent[u]; }, [&](uint32_t u) { return key[u]; });
        if (e.key == WS_NO_KEY) continue;
        if (PASS == 0) atomicMin(&A.best[r], (unsigned long long)e.key);
        else if (A.best[r] == e.key) atomicMin(&A.pick[r], e.id);
    }
}

__global__ __launch_bounds__(WS_THREADS) void k_ws_hook(const WsArgs A) {
    const int64_t V = voxels_of(A);
    const WsBox B = box_of_args(A);
    const uint32_t* __restrict__ parent = A.parent;
    const uint32_t* __restrict__ pick = A.pick;
    unsigned long long hooks = 0, bad = 0;
    for (int64_t i = (int64_t)blockIdx.x * WS_THREADS + threadIdx.x; i < V; i += (int64_t)gridDim.x * WS_THREADS) {
        if (parent[i] != (uint32_t)i) continue;   // a seedless root holds its own index, unflagged
        const uint32_t id = pick[i];
        if (id == WS_NO_EDGE) continue;
        // (an id that an atomic minimum of this call wrote names two voxels of the box)
        if ((int64_t)(id / 3u) + ws_axis_step(B, (int)(id % 3u)) >= V) {
            bad = 1;
            A.best[i] = (unsigned long long)i;
            continue;
        }
        const uint32_t t = ws_hook(
            B, (uint32_t)i, id, [&](uint32_t u) { return parent[u]; }, [&](uint32_t u) { return pick[u]; });
        A.best[i] = (unsigned long long)t;
        hooks += t != (uint32_t)i;
    }
    hooks = block_sum(hooks);
    bad = block_sum(bad);
    if (threadIdx.x == 0) {
        if (hooks) atomicAdd(&A.words[WS_W_HOOKS], hooks);
        if (bad) atomicOr(&A.words[WS_W_ERR], 1ull);
    }
}

__global__ __launch_bounds__(WS_THREADS) void k_ws_apply(const WsArgs A) {
    const int64_t V = voxels_of(A);
    for (int64_t i = (int64_t)blockIdx.x * WS_THREADS + threadIdx.x; i < V; i += (int64_t)gridDim.x * WS_THREADS) {
        if (A.parent[i] != (uint32_t)i || A.pick[i] == WS_NO_EDGE) continue;
        A.parent[i] = (uint32_t)A.best[i];
        A.best[i] = WS_NO_KEY;
        A.pick[i] = WS_NO_EDGE;
    }
}

__global__ __launch_bounds__(WS_THREADS) void k_ws_chase(const WsArgs A) {
    const int64_t V = voxels_of(A);
    const AgentLoad load{};
    bool done = true;
    for (int64_t i = (int64_t)blockIdx.x * WS_THREADS + threadIdx.x; i < V; i += (int64_t)gridDim.x * WS_THREADS) {
        const uint32_t x = load(&A.parent[i]);
        if (x == (uint32_t)i || (x & WS_SEEDED)) continue;
        const uint32_t r = ws_chase(A.parent, x, load, &done);
        if (r != x) __hip_atomic_store(&A.parent[i], r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    const unsigned long long left = block_sum(done ? 0ull : 1ull);
    if (threadIdx.x == 0 && left) atomicOr(&A.words[WS_W_SHORT], 1ull);
}

__global__ __launch_bounds__(WS_THREADS) void k_ws_write(const WsArgs A, uint64_t* out) {
    const int64_t V = voxels_of(A);
    unsigned long long zero = 0, top = 0;
    for (int64_t i = (int64_t)blockIdx.x * WS_THREADS + threadIdx.x; i < V; i += (int64_t)gridDim.x * WS_THREADS) {
        const uint32_t p = A.parent[i];
        // (in place, out is the seeds: a seeded voxel is rewritten with its own label, and nothing reads an
        // unseeded one)
        const uint64_t l = (p & WS_SEEDED) ? seed_at(A, element_of(A, p & WS_INDEX)) : 0ull;
        out[i] = l;
        zero += l == 0;
        top = l > top ? l : top;
    }
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long other = shfl_down_u64(top, o);
        top = other > top ? other : top;
    }
    if ((threadIdx.x & (WAVE - 1)) == 0 && top) atomicMax(&A.words[WS_W_MAX], top);
    zero = block_sum(zero);
    if (threadIdx.x == 0 && zero) atomicAdd(&A.words[WS_W_ZERO], zero);
}

// the row of label l in the ascending table nodes[0 .. n), which holds it
__device__ __forceinline__ int64_t row_of(const uint64_t* __restrict__ nodes, int64_t n, uint64_t l) {
    int64_t lo = 0, hi = n - 1;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (nodes[mid] < l) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(WS_THREADS) void k_ws_filter(uint64_t* out, int64_t n, const uint64_t* __restrict__ nodes,
                                                          const uint64_t* __restrict__ moments, int64_t n_nodes,
                                                          uint64_t size) {
    for (int64_t i = (int64_t)blockIdx.x * WS_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * WS_THREADS) {
        const uint64_t l = out[i];
        if (l == 0) continue;
        const int64_t j = row_of(nodes, n_nodes, l);
        if (nodes[j] == l && moments[j * MORPH_WORDS] < size) out[i] = 0;
    }
}

__global__ __launch_bounds__(WS_THREADS) void k_ws_dropped(const uint64_t* __restrict__ nodes,
                                                           const uint64_t* __restrict__ moments, int64_t n_nodes,
                                                           uint64_t size, unsigned long long* words) {
    unsigned long long dropped = 0;
    for (int64_t j = (int64_t)blockIdx.x * WS_THREADS + threadIdx.x; j < n_nodes; j += (int64_t)gridDim.x * WS_THREADS)
        dropped += nodes[j] != 0 && moments[j * MORPH_WORDS] < size;
    dropped = block_sum(dropped);
    if (threadIdx.x == 0 && dropped) atomicAdd(&words[WS_W_DROPPED], dropped);
}

static unsigned ws_grid(const WsArgs& A) { return (unsigned)ws_grid((int64_t)A.box.n[0] * A.box.n[1] * A.box.n[2]); }

hipError_t launch_ws_init(const WsArgs& A, int with_keys, hipStream_t s) {
    if (with_keys) hipLaunchKernelGGL(k_ws_init<1>, dim3(ws_grid(A)), dim3(WS_THREADS), 0, s, A);
    else hipLaunchKernelGGL(k_ws_init<0>, dim3(ws_grid(A)), dim3(WS_THREADS), 0, s, A);
    return hipGetLastError();
}

hipError_t launch_ws_pick(const WsArgs& A, hipStream_t s) {
    hipLaunchKernelGGL(k_ws_pick<0>, dim3(ws_grid(A)), dim3(WS_THREADS), 0, s, A);
    hipLaunchKernelGGL(k_ws_pick<1>, dim3(ws_grid(A)), dim3(WS_THREADS), 0, s, A);
    hipLaunchKernelGGL(k_ws_hook, dim3(ws_grid(A)), dim3(WS_THREADS), 0, s, A);
    return hipGetLastError();
}

hipError_t launch_ws_apply(const WsArgs& A, hipStream_t s) {
    hipLaunchKernelGGL(k_ws_apply, dim3(ws_grid(A)), dim3(WS_THREADS), 0, s, A);
    return hipGetLastError();
}

hipError_t launch_ws_chase(const WsArgs& A, hipStream_t s) {
    hipLaunchKernelGGL(k_ws_chase, dim3(ws_grid(A)), dim3(WS_THREADS), 0, s, A);
    return hipGetLastError();
}

hipError_t launch_ws_write(const WsArgs& A, uint64_t* out, hipStream_t s) {
    hipLaunchKernelGGL(k_ws_write, dim3(ws_grid(A)), dim3(WS_THREADS), 0, s, A, out);
    return hipGetLastError();
}

hipError_t launch_ws_filter(uint64_t* out, int64_t n, const uint64_t* nodes, const uint64_t* moments, int64_t n_nodes,
                            uint64_t size, unsigned long long* words, hipStream_t s) {
    if (n == 0 || n_nodes == 0) return hipSuccess;
    hipLaunchKernelGGL(k_ws_filter, dim3((unsigned)ws_grid(n)), dim3(WS_THREADS), 0, s, out, n, nodes, moments, n_nodes,
                       size);
    hipLaunchKernelGGL(k_ws_dropped, dim3((unsigned)ws_grid(n_nodes)), dim3(WS_THREADS), 0, s, nodes, moments, n_nodes,
                       size, words);
    return hipGetLastError();
}

}  // namespace ctg
