// Thresholded components: the connected components of a thresholded box, and
// the union-find merge of block-offset ids.  Replaces the array work of
// thresholded_components/block_components.py:161-182 (vu.normalize, the
// comparison, np.sum, skimage.morphology.label, max) and of
// thresholded_components/merge_assignments.py:125-132 (nufd.boost_ufd,
// relabelConsecutive).
//
//   k_cc_range     the box's smallest and largest sample as f2ord words and its
//                  NaN flag, one atomic per workgroup (normalised calls only)
//   k_cc_tile      one workgroup per 64 x 8 x 16 tile, a wave per row: the
//                  predicate's ballot per row into LDS; an x-run is one node,
//                  named by its first voxel's tile-local raster index; rows are
//                  united with their earlier neighbour rows (ctg_plan.h:
//                  cc_neighbor_rows) by the lanes where two runs first touch
//                  (ctg_uf.h: contact_*), with atomic mins on an LDS parent
//                  table; then every foreground voxel's tile root goes out as a
//                  u32 box-linear index (background: UF_NONE)
//   k_cc_seams     the voxels on a tile's low x, y, z faces unite with their
//                  neighbours across those faces (edge and corner voxels with
//                  the diagonal partners of connectivity 2 and 3 as well)
//   k_uf_init / k_uf_pairs   the same union over (a, b) id pairs
//   k_uf_flatten   every node's root; a wave numbers the roots of its CC_SEG nodes
//   k_uf_scan      the exclusive prefix of the segments' root counts
//   k_uf_write     out[i] = rank of i's root + plus, two per lane
//
// Tile-local raster order (z, y, x) agrees with the box's, and every union
// keeps the smaller index as the root, so the root of a component is its first
// voxel in raster order and the rank of the root among all roots numbers the
// components 1 .. N in the order of their first voxels -- scipy.ndimage.label's
// numbering, exactly, not up to a permutation.
//
// parent[] is shared between workgroups in k_cc_seams, k_uf_pairs and
// k_uf_flatten: it is touched there with agent-scope atomics only (ctg_uf.h
// says why that suffices).  Every find and union is capped; past the cap the
// kernel raises CC_ERR_CAP in the call's words and the host reports it.
//
// Every buffer here is call-sized and comes from the pool (DevBuf); nothing
// touches the workspace's record or sort buffers, so a CTG_DEFER_STATS handle
// stays valid across these calls.
#include <hip/hip_runtime.h>

#include <cmath>

#include "ctg_internal.h"
#include "ctg_uf.h"

namespace ctg {

constexpr int CC_THREADS = CC_TILE_Y * WAVE;   // a wave per y row, CC_TILE_Z rows each
static_assert(TILE_X == WAVE, "lane = x");
static_assert(CC_SEG % WAVE == 0, "a segment is whole wave steps");

typedef unsigned long long cc_u64x2 __attribute__((ext_vector_type(2)));

// parent[] in LDS: coherent within the workgroup, but not to be kept in registers
struct LdsLoad {
    __device__ uint32_t operator()(const uint32_t* p) const {
        return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
};
// parent[] in device memory, shared between workgroups: served by the L2, never by this CU's L1
struct AgentLoad {
    __device__ uint32_t operator()(const uint32_t* p) const {
        return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
};
struct AtomicMin {
    __device__ uint32_t operator()(uint32_t* p, uint32_t v) const { return atomicMin(p, v); }
};

template <typename DataT>
__global__ __launch_bounds__(256) void k_cc_range(const CcArgs A) {
    const DataT* D = (const DataT*)A.data + A.box.base;
    const int64_t rows = (int64_t)A.box.n[0] * A.box.n[1];
    const int lane = threadIdx.x & (WAVE - 1);
    float lo = INFINITY, hi = -INFINITY;
    bool nan = false;
    // a wave per row of the box
    for (int64_t r = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / WAVE; r < rows;
         r += (int64_t)gridDim.x * blockDim.x / WAVE) {
        const DataT* row = D + (r / A.box.n[1]) * A.box.s_z + (r % A.box.n[1]) * A.box.s_y;
        for (uint32_t x = lane; x < A.box.n[2]; x += WAVE) {
            const float v = (float)row[x];
            nan |= v != v;
            lo = fminf(lo, v);   // (fminf / fmaxf skip a NaN: the flag carries it)
            hi = fmaxf(hi, v);
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        lo = fminf(lo, __shfl_xor(lo, o, WAVE));
        hi = fmaxf(hi, __shfl_xor(hi, o, WAVE));
    }
    // One atomic pair per workgroup, not per wave: atomics to one address queue up behind each
    // other (32 K waves of a 512^3 box: 0.79 ms for this kernel, whatever the box)
    __shared__ float slo[4], shi[4];
    __shared__ int snan[4];
    const int w = threadIdx.x / WAVE;
    const uint64_t any_nan = __ballot(nan);
    if (lane == 0) {
        slo[w] = lo;
        shi[w] = hi;
        snan[w] = any_nan != 0;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < 4; ++k) {
            lo = fminf(lo, slo[k]);
            hi = fmaxf(hi, shi[k]);
            snan[0] |= snan[k];
        }
        atomicMin(&A.words[CC_W_MIN], f2ord(lo));
        atomicMax(&A.words[CC_W_MAX], f2ord(hi));
        if (snan[0]) atomicOr(&A.words[CC_W_NAN], 1u);
    }
}

// DataT: float or uint8_t; CONN: 1, 2, 3; NORM: the reference's normalised
// value (vu.normalize, volume_utils.py:98-105): v = x - mn, then v /= mx where
// mx = max - mn > 0 -- two f32 operations, the divide correctly rounded
template <typename DataT, int CONN, bool NORM>
__global__ __launch_bounds__(CC_THREADS) void k_cc_tile(const CcArgs A) {
    __shared__ uint64_t bits[CC_ROWS];
    __shared__ uint32_t par[CC_ROWS * TILE_X];
    const int lane = threadIdx.x & (WAVE - 1), w = threadIdx.x / WAVE;
    uint32_t t = blockIdx.x;
    const uint32_t tx = t % A.nt[2];
    t /= A.nt[2];
    const uint32_t ty = t % A.nt[1], tz = t / A.nt[1];
    const uint32_t gx = tx * TILE_X + lane, gy = ty * CC_TILE_Y + w;
    const bool inxy = gx < A.box.n[2] && gy < A.box.n[1];
    float mn = 0.f, mx = 0.f;
    bool divide = false, dead = false;
    if constexpr (NORM) {
        // a NaN in the box: numpy's min is NaN, every normalised value is, and no comparison holds
        dead = A.words[CC_W_NAN] != 0;
        mn = ord2f(A.words[CC_W_MIN]);
        mx = ord2f(A.words[CC_W_MAX]) - mn;
        // (a box that holds -inf: x - mn is NaN there, so numpy's max is NaN and nothing is divided)
        divide = mx > 0.f && mn != -INFINITY;
    }
    const int64_t col = A.box.base + (int64_t)gy * A.box.s_y + gx;
    const DataT* D = (const DataT*)A.data;
#pragma unroll
    for (int z = 0; z < CC_TILE_Z; ++z) {
        const uint32_t gz = tz * CC_TILE_Z + z;
        bool f = false;
        if (inxy && gz < A.box.n[0] && !dead) {
            const int64_t i = col + (int64_t)gz * A.box.s_z;
            float v = (float)D[i];
            if constexpr (NORM) {
                v = v - mn;
                if (divide) v = v / mx;
            }
            f = A.mode == CTG_CC_GREATER ? v > A.threshold : A.mode == CTG_CC_LESS ? v < A.threshold : v == A.threshold;
            if (A.mask) f = f && A.mask[i] != 0;
        }
        const uint64_t m = __ballot(f);
        const int r = z * CC_TILE_Y + w;
        if (lane == 0) bits[r] = m;
        if ((run_starts(m) >> lane) & 1) par[r * TILE_X + lane] = (uint32_t)(r * TILE_X + lane);   // heads only
    }
    __syncthreads();
    constexpr CcRows R = cc_neighbor_rows(CONN);
    constexpr uint32_t CAP = CC_ROWS * TILE_X;
    int over = 0;
    for (int z = 0; z < CC_TILE_Z; ++z) {
        const int r = z * CC_TILE_Y + w;
        const uint64_t m = bits[r];
        if (!m) continue;   // (wave-uniform)
#pragma unroll
        for (int k = 0; k < R.n; ++k) {
            const int z2 = z + R.dz[k], y2 = w + R.dy[k];
            if (z2 < 0 || y2 < 0 || y2 >= CC_TILE_Y) continue;
            const int r2 = z2 * CC_TILE_Y + y2;
            const uint64_t m2 = bits[r2];
            if (!m2) continue;
            if ((contact_same(m, m2) >> lane) & 1)
                uf_union(par, (uint32_t)(r * TILE_X + run_head(m, lane)), (uint32_t)(r2 * TILE_X + run_head(m2, lane)),
                         CAP, LdsLoad(), AtomicMin(), &over);
            if (R.dil[k]) {
                if ((contact_up(m, m2) >> lane) & 1)
                    uf_union(par, (uint32_t)(r * TILE_X + lane), (uint32_t)(r2 * TILE_X + run_head(m2, lane - 1)), CAP,
                             LdsLoad(), AtomicMin(), &over);
                if ((contact_down(m, m2) >> lane) & 1)
                    uf_union(par, (uint32_t)(r * TILE_X + run_head(m, lane)), (uint32_t)(r2 * TILE_X + lane + 1), CAP,
                             LdsLoad(), AtomicMin(), &over);
            }
        }
    }
    __syncthreads();
    for (int z = 0; z < CC_TILE_Z; ++z) {
        const uint32_t gz = tz * CC_TILE_Z + z;
        if (!inxy || gz >= A.box.n[0]) continue;
        const int r = z * CC_TILE_Y + w;
        const uint64_t m = bits[r];
        uint32_t val = UF_NONE;
        if ((m >> lane) & 1) {
            const uint32_t root = uf_find(par, (uint32_t)(r * TILE_X + run_head(m, lane)), CAP, LdsLoad(), &over);
            const uint32_t lz = root / (CC_TILE_Y * TILE_X), ly = (root / TILE_X) % CC_TILE_Y, lx = root % TILE_X;
            val = (uint32_t)(((uint64_t)(tz * CC_TILE_Z + lz) * A.box.n[1] + (ty * CC_TILE_Y + ly)) * A.box.n[2] +
                             (tx * TILE_X + lx));
        }
        A.parent[((uint64_t)gz * A.box.n[1] + gy) * A.box.n[2] + gx] = val;
    }
    if (over) atomicOr(&A.words[CC_W_ERR], CC_ERR_CAP);
}

// One thread per low-face voxel (ctg_plan.h: cc_grid): first the x faces (every
// 64th column), then the y faces, then the z faces; a voxel on two faces is
// taken by the first.  It unites with each neighbour of its connectivity that
// lies across a low face of its tile -- with every voxel pair that spans two
// tiles, one of the two sits on the low face between them.
template <int CONN>
__global__ __launch_bounds__(256) void k_cc_seams(const CcArgs A, const CcGrid G) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= G.seam_threads) return;
    const int64_t n0 = A.box.n[0], n1 = A.box.n[1], n2 = A.box.n[2];
    const CcSeamVoxel v = cc_seam_voxel(G, n1, n2, i);
    if (!v.take) return;
    const AgentLoad load{};
    const uint32_t me = load(&A.parent[(v.z * n1 + v.y) * n2 + v.x]);
    if (me == UF_NONE) return;
    int over = 0;
#pragma unroll
    for (int dz = -1; dz <= 1; ++dz)
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
            for (int dx = -1; dx <= 1; ++dx) {
                if (!cc_seam_partner(CONN, v.z, v.y, v.x, dz, dy, dx)) continue;
                const int64_t qz = v.z + dz, qy = v.y + dy, qx = v.x + dx;
                if (qz < 0 || qy < 0 || qx < 0 || qz >= n0 || qy >= n1 || qx >= n2) continue;
                const uint32_t other = load(&A.parent[(qz * n1 + qy) * n2 + qx]);
                if (other == UF_NONE) continue;
                uf_union(A.parent, me, other, (uint32_t)(n0 * n1 * n2), load, AtomicMin(), &over);
            }
    if (over) atomicOr(&A.words[CC_W_ERR], CC_ERR_CAP);
}

__global__ __launch_bounds__(256) void k_uf_init(uint32_t* parent, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) parent[i] = (uint32_t)i;
}

__global__ __launch_bounds__(256) void k_uf_pairs(const uint64_t* __restrict__ pairs, int64_t n, uint32_t* parent,
                                                  uint32_t n_labels, uint32_t* words) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const cc_u64x2 p = *(const cc_u64x2*)(pairs + 2 * i);
    if (p.x == 0 || p.y == 0 || p.x >= n_labels || p.y >= n_labels) {
        atomicOr(&words[CC_W_ERR], CC_ERR_PAIR);
        return;
    }
    int over = 0;
    uf_union(parent, (uint32_t)p.x, (uint32_t)p.y, n_labels, AgentLoad(), AtomicMin(), &over);
    if (over) atomicOr(&words[CC_W_ERR], CC_ERR_CAP);
}

// A wave takes the CC_SEG nodes of one segment in order: each node's root
// replaces its entry (other waves that still read the entry see an ancestor
// either way), a root gets its rank among the roots of the segment
__global__ __launch_bounds__(256) void k_uf_flatten(uint32_t* parent, int64_t n, uint32_t* rank, uint32_t* seg,
                                                    uint32_t* words) {
    const int lane = threadIdx.x & (WAVE - 1);
    const int64_t sg = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / WAVE;
    const int64_t base = sg * CC_SEG;
    if (base >= n) return;   // (wave-uniform)
    const AgentLoad load{};
    uint32_t run = 0;
    int over = 0;
    for (int it = 0; it < CC_SEG / WAVE; ++it) {
        const int64_t p = base + it * WAVE + lane;
        bool root = false;
        if (p < n) {
            const uint32_t v = load(&parent[p]);
            if (v != UF_NONE) {
                const uint32_t r = uf_find(parent, v, (uint32_t)n, load, &over);
                root = r == (uint32_t)p;
                if (r != v) __hip_atomic_store(&parent[p], r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
        const uint64_t b = __ballot(root);
        if (root) rank[p] = run + (uint32_t)__popcll(b & ((1ull << lane) - 1ull));
        run += (uint32_t)__popcll(b);
    }
    if (lane == 0) seg[sg] = run;
    if (over) atomicOr(&words[CC_W_ERR], CC_ERR_CAP);
}

// one workgroup: seg[0 .. n_seg) -> its exclusive prefix, 1024 entries a step
__global__ __launch_bounds__(1024) void k_uf_scan(uint32_t* seg, int64_t n_seg, uint32_t* words) {
    __shared__ uint32_t wsum[16];
    __shared__ uint32_t carry;
    const int lane = threadIdx.x & (WAVE - 1), w = threadIdx.x / WAVE;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (int64_t base = 0; base < n_seg; base += 1024) {
        const int64_t i = base + threadIdx.x;
        const uint32_t v = i < n_seg ? seg[i] : 0u;
        uint32_t incl = v;
        for (int o = 1; o < WAVE; o <<= 1) {
            const uint32_t u = __shfl_up(incl, o, WAVE);
            if (lane >= o) incl += u;
        }
        if (lane == WAVE - 1) wsum[w] = incl;
        __syncthreads();
        uint32_t before = carry;
        for (int k = 0; k < w; ++k) before += wsum[k];
        if (i < n_seg) seg[i] = before + incl - v;
        __syncthreads();
        if (threadIdx.x == 1023) carry = before + incl;
        __syncthreads();
    }
    if (threadIdx.x == 0) words[CC_W_TOTAL] = carry;
}

__device__ __forceinline__ uint64_t uf_id(const uint32_t* __restrict__ rank, const uint32_t* __restrict__ seg,
                                          uint32_t root, uint64_t plus) {
    return root == UF_NONE ? 0ull : (uint64_t)seg[root / CC_SEG] + rank[root] + plus;
}

// two nodes per lane: one 8-byte load, one 16-byte store where out is 16-byte aligned (wide)
__global__ __launch_bounds__(256) void k_uf_write(const uint32_t* __restrict__ parent,
                                                  const uint32_t* __restrict__ rank,
                                                  const uint32_t* __restrict__ seg, int64_t n, uint64_t plus,
                                                  uint64_t* out, int wide) {
    const int64_t i = 2 * ((int64_t)blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= n) return;
    if (i + 1 < n) {
        const uint2 r = *(const uint2*)(parent + i);
        const uint64_t a = uf_id(rank, seg, r.x, plus), b = uf_id(rank, seg, r.y, plus);
        if (wide) {
            cc_u64x2 o;
            o.x = a;
            o.y = b;
            __builtin_nontemporal_store(o, (cc_u64x2*)(out + i));
        } else {
            out[i] = a;
            out[i + 1] = b;
        }
    } else {
        out[i] = uf_id(rank, seg, parent[i], plus);
    }
}

static unsigned blocks_for(int64_t threads, int per_block) { return (unsigned)((threads + per_block - 1) / per_block); }

hipError_t launch_cc_range(const CcArgs& A, int data_kind, hipStream_t s) {
    const int64_t rows = (int64_t)A.box.n[0] * A.box.n[1];
    const unsigned blocks = (unsigned)std::min<int64_t>((rows + 3) / 4, 2048);
    if (data_kind == CTG_DATA_U8) hipLaunchKernelGGL(k_cc_range<uint8_t>, dim3(blocks), dim3(256), 0, s, A);
    else hipLaunchKernelGGL(k_cc_range<float>, dim3(blocks), dim3(256), 0, s, A);
    return hipGetLastError();
}

template <typename DataT, int CONN>
static void launch_cc_tile_n(const CcArgs& A, unsigned tiles, int normalize, hipStream_t s) {
    if (normalize) hipLaunchKernelGGL((k_cc_tile<DataT, CONN, true>), dim3(tiles), dim3(CC_THREADS), 0, s, A);
    else hipLaunchKernelGGL((k_cc_tile<DataT, CONN, false>), dim3(tiles), dim3(CC_THREADS), 0, s, A);
}
template <typename DataT>
static void launch_cc_tile_c(const CcArgs& A, unsigned tiles, int normalize, int conn, hipStream_t s) {
    if (conn == 1) launch_cc_tile_n<DataT, 1>(A, tiles, normalize, s);
    else if (conn == 2) launch_cc_tile_n<DataT, 2>(A, tiles, normalize, s);
    else launch_cc_tile_n<DataT, 3>(A, tiles, normalize, s);
}

hipError_t launch_cc_tile(const CcArgs& A, const CcGrid& G, int data_kind, int normalize, int conn, hipStream_t s) {
    if (data_kind == CTG_DATA_U8) launch_cc_tile_c<uint8_t>(A, (unsigned)G.tiles, normalize, conn, s);
    else launch_cc_tile_c<float>(A, (unsigned)G.tiles, normalize, conn, s);
    return hipGetLastError();
}

hipError_t launch_cc_seams(const CcArgs& A, const CcGrid& G, int conn, hipStream_t s) {
    if (G.seam_threads == 0) return hipSuccess;
    const unsigned blocks = blocks_for(G.seam_threads, 256);
    if (conn == 1) hipLaunchKernelGGL(k_cc_seams<1>, dim3(blocks), dim3(256), 0, s, A, G);
    else if (conn == 2) hipLaunchKernelGGL(k_cc_seams<2>, dim3(blocks), dim3(256), 0, s, A, G);
    else hipLaunchKernelGGL(k_cc_seams<3>, dim3(blocks), dim3(256), 0, s, A, G);
    return hipGetLastError();
}

hipError_t launch_uf_init(uint32_t* parent, int64_t n, hipStream_t s) {
    hipLaunchKernelGGL(k_uf_init, dim3(blocks_for(n, 256)), dim3(256), 0, s, parent, n);
    return hipGetLastError();
}

hipError_t launch_uf_pairs(const uint64_t* pairs, int64_t n, uint32_t* parent, uint32_t n_labels, uint32_t* words,
                           hipStream_t s) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_uf_pairs, dim3(blocks_for(n, 256)), dim3(256), 0, s, pairs, n, parent, n_labels, words);
    return hipGetLastError();
}

hipError_t launch_uf_flatten(uint32_t* parent, int64_t n, uint32_t* rank, uint32_t* seg, uint32_t* words,
                             hipStream_t s) {
    hipLaunchKernelGGL(k_uf_flatten, dim3(blocks_for(cc_segments(n) * WAVE, 256)), dim3(256), 0, s, parent, n, rank, seg,
                       words);
    return hipGetLastError();
}

hipError_t launch_uf_scan(uint32_t* seg, int64_t n_seg, uint32_t* words, hipStream_t s) {
    hipLaunchKernelGGL(k_uf_scan, dim3(1), dim3(1024), 0, s, seg, n_seg, words);
    return hipGetLastError();
}

hipError_t launch_uf_write(const uint32_t* parent, const uint32_t* rank, const uint32_t* seg, int64_t n,
                           uint64_t plus, uint64_t* out, hipStream_t s) {
    const int wide = ((uintptr_t)out & 15u) == 0;
    hipLaunchKernelGGL(k_uf_write, dim3(blocks_for((n + 1) / 2, 256)), dim3(256), 0, s, parent, rank, seg, n, plus, out,
                       wide);
    return hipGetLastError();
}

}  // namespace ctg
