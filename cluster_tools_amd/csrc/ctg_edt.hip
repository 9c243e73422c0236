// The exact Euclidean distance transform of a box (include/ctg.h:
// ctg_distance_transform), three separable passes with the lanes along x in
// all of them, so every global access is a row segment:
//
//   k_edt_x     a wave per row: the source is read once, the seed predicate's
//               ballots go to LDS as the row's 64-bit words with one bit per
//               nonzero word above them, and every voxel finds its nearest
//               seed of the row by count-leading / count-trailing zeros
//               (ctg_edt.h: edt_row_distance) -- no serial scan.  |dx| goes
//               out as u16 (EDT_NONE16: no seed in the row); the seeds are
//               counted, folded per workgroup before the one global atomic.
//   k_edt_line  a lane per column, a wave per 64 columns: the lower envelope
//               of the line's parabolas on a per-lane stack (ctg_edt.h:
//               edt_push / edt_seek), in LDS or, for long lines, in a
//               call-sized buffer (ctg_plan.h: edt_line_plan).  The y pass
//               writes (|dy|, |dx|) as two u16; the last pass of a call (the z
//               pass, or the y pass where there is none) writes
//               (float)sqrt(edt_d2(offsets)), or D2 itself, and folds the arg-max of D2 and
//               the voxels without a seed into one partial per workgroup.
//   k_edt_fold  the partials -> the call's info words.
//
// Stack depth: a line of n positions pushes at most n entries, so depth k < n
// always; the LDS stack holds EDT_LDS_LINE entries a lane and is chosen only
// for n <= EDT_LDS_LINE, the buffer holds n a lane.
//
// Every buffer here is call-sized and comes from the pool; nothing touches the
// workspace's record or sort buffers.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "ctg_edt.h"
#include "ctg_internal.h"

namespace ctg {

namespace {

template <int KIND>
struct EdtSource;
template <>
struct EdtSource<0> {   // CTG_EDT_SRC_NONZERO, uint8
    static __device__ __forceinline__ bool test(const EdtSrc& A, int64_t i) { return ((const uint8_t*)A.src)[i] != 0; }
};
template <>
struct EdtSource<1> {   // CTG_EDT_SRC_GREATER, float32 (a NaN is not greater)
    static __device__ __forceinline__ bool test(const EdtSrc& A, int64_t i) {
        return ((const float*)A.src)[i] > A.threshold;
    }
};
template <>
struct EdtSource<2> {   // CTG_EDT_SRC_EQUAL, uint32 (widened: an id of 2^32 or above matches nothing)
    static __device__ __forceinline__ bool test(const EdtSrc& A, int64_t i) {
        return (uint64_t)((const uint32_t*)A.src)[i] == A.label;
    }
};
template <>
struct EdtSource<3> {   // CTG_EDT_SRC_EQUAL, uint64
    static __device__ __forceinline__ bool test(const EdtSrc& A, int64_t i) {
        return ((const uint64_t*)A.src)[i] == A.label;
    }
};

template <int KIND>
__global__ __launch_bounds__(EDT_X_WAVES * WAVE) void k_edt_x(const EdtSrc A, uint16_t* __restrict__ out,
                                                              unsigned long long* info) {
    __shared__ uint64_t words[EDT_X_WAVES][EDT_ROW_WORDS + EDT_ROW_SUPER];
    __shared__ unsigned long long wave_seeds[EDT_X_WAVES];
    const int wave = threadIdx.x / WAVE, lane = threadIdx.x & (WAVE - 1);
    const int nx = (int)A.box.n[2], nw = (nx + 63) >> 6, ns = (nw + 63) >> 6;
    const int64_t rows = (int64_t)A.box.n[0] * A.box.n[1];
    const int64_t groups = (rows + EDT_X_WAVES - 1) / EDT_X_WAVES;
    uint64_t* W = words[wave];
    uint64_t* S = W + EDT_ROW_WORDS;
    unsigned long long seeds = 0;
    // every wave of the workgroup takes the same number of turns (the barriers below)
    for (int64_t g = blockIdx.x; g < groups; g += gridDim.x) {
        const int64_t row = g * EDT_X_WAVES + wave;
        const bool live = row < rows;
        if (live) {
            const int64_t off = A.box.base + (row / A.box.n[1]) * A.box.s_z + (row % A.box.n[1]) * A.box.s_y;
            for (int w = 0; w < nw; ++w) {
                const int x = (w << 6) + lane;
                const bool p = x < nx && (EdtSource<KIND>::test(A, off + x) != (A.invert != 0));
                const uint64_t m = __ballot(p);
                if (lane == 0) W[w] = m;
                seeds += (unsigned long long)__popcll(m);
            }
        }
        __syncthreads();
        if (live) {
            for (int sw = 0; sw < ns; ++sw) {
                const int w = (sw << 6) + lane;
                const uint64_t m = __ballot(w < nw && W[w] != 0);
                if (lane == 0) S[sw] = m;
            }
        }
        __syncthreads();
        if (live) {
            uint16_t* o = out + row * nx;
            for (int x = lane; x < nx; x += WAVE) o[x] = (uint16_t)edt_row_distance(W, S, ns, x);
        }
        __syncthreads();   // (the next turn overwrites the words)
    }
    if (lane == 0) wave_seeds[wave] = seeds;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < EDT_X_WAVES; ++k) seeds += wave_seeds[k];
        if (seeds) atomicAdd(info, seeds);
    }
}

// a lane's stack: entry k of this lane
struct LdsStack {
    EdtEntry* p;   // &lds[lane]
    __device__ __forceinline__ EdtEntry get(int k) const { return p[k * WAVE]; }
    __device__ __forceinline__ void set(int k, EdtEntry e) { p[k * WAVE] = e; }
};
struct BufStack {
    EdtEntry* p;   // &buf[workgroup * 64 + lane]
    int64_t stride;   // entries per depth: 64 x the grid
    __device__ __forceinline__ EdtEntry get(int k) const { return p[k * stride]; }
    __device__ __forceinline__ void set(int k, EdtEntry e) { p[k * stride] = e; }
};

template <bool IN32, bool FINAL, bool LDS>
__global__ __launch_bounds__(WAVE) void k_edt_line(const EdtLineArgs A, int64_t groups) {
    const int lane = threadIdx.x;
    const int64_t nx = A.n[2], plane = (int64_t)A.n[1] * nx;
    const int64_t xg = (nx + WAVE - 1) / WAVE;
    const int len = (int)A.n[A.axis];
    const int64_t step = A.axis == 1 ? nx : plane, outer_stride = A.axis == 1 ? plane : nx;
    const EdtAxis X{A.p[1], A.p[2], A.p[A.axis] * A.p[A.axis], len};
    using Stack = typename std::conditional<LDS, LdsStack, BufStack>::type;
    Stack S;
    if constexpr (LDS) {
        __shared__ EdtEntry lds[EDT_LDS_LINE * WAVE];
        S.p = lds + lane;
    } else {
        S.p = A.stack + (int64_t)blockIdx.x * WAVE + lane;
        S.stride = (int64_t)gridDim.x * WAVE;
    }
    double best = -1.0;
    uint32_t best_i = 0;
    unsigned long long unseeded = 0;
    auto offer = [&](double d2, int64_t i) {
        if (d2 > best || (d2 == best && (uint32_t)i < best_i)) {
            best = d2;
            best_i = (uint32_t)i;
        }
    };
    for (int64_t g = blockIdx.x; g < groups; g += gridDim.x) {
        const int64_t x = (g % xg) * WAVE + lane;
        if (x >= nx) continue;
        const int64_t base = (g / xg) * outer_stride + x;
        int k = -1;
        EdtEntry top = 0;
        for (int q0 = 0; q0 < len; q0 += 4) {
            uint32_t v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int q = q0 + u;
                if (q < len) {
                    if constexpr (IN32) v[u] = ((const uint32_t*)A.in)[base + q * step];
                    else v[u] = ((const uint16_t*)A.in)[base + q * step];
                } else {
                    v[u] = IN32 ? EDT_NONE32 : EDT_NONE16;
                }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (v[u] == (IN32 ? EDT_NONE32 : EDT_NONE16)) continue;
                if constexpr (IN32) edt_push(S, k, top, (uint32_t)(q0 + u), v[u] & 0xFFFFu, v[u] >> 16, X);
                else edt_push(S, k, top, (uint32_t)(q0 + u), 0u, v[u], X);
            }
        }
        if (k < 0) {   // no seed in the line's domain
            for (int t = 0; t < len; ++t) {
                const int64_t i = base + t * step;
                if constexpr (FINAL) {
                    if (A.out_d2) ((double*)A.out)[i] = A.diag2;
                    else ((float*)A.out)[i] = (float)__dsqrt_rn(A.diag2);
                    offer(A.diag2, i);
                } else {
                    ((uint32_t*)A.out)[i] = EDT_NONE32;
                }
            }
            if (FINAL) unseeded += (unsigned long long)len;
            continue;
        }
        int j = 0;
        EdtEntry cur = S.get(0), nxt = edt_next(S, k, 0);
        for (int t = 0; t < len; ++t) {
            edt_seek(S, k, j, cur, nxt, (uint32_t)t);
            const int64_t i = base + t * step;
            const uint32_t q = edt_q(cur), d = (uint32_t)t > q ? (uint32_t)t - q : q - (uint32_t)t;
            if constexpr (FINAL) {
                const double d2 = A.axis == 1 ? edt_d2(0u, d, edt_b(cur), A.p) : edt_d2(d, edt_a(cur), edt_b(cur), A.p);
                if (A.out_d2) ((double*)A.out)[i] = d2;
                else ((float*)A.out)[i] = (float)__dsqrt_rn(d2);
                offer(d2, i);
            } else {
                ((uint32_t*)A.out)[i] = d | (edt_b(cur) << 16);
            }
        }
    }
    if constexpr (FINAL) {
        for (int o = 32; o > 0; o >>= 1) {
            const double ob = __shfl_down(best, o, WAVE);
            const uint32_t oi = __shfl_down(best_i, o, WAVE);
            unseeded += shfl_down_u64(unseeded, o);
            if (ob > best || (ob == best && oi < best_i)) {
                best = ob;
                best_i = oi;
            }
        }
        if (lane == 0) {
            unsigned long long* P = A.part + (int64_t)blockIdx.x * EDT_PART_WORDS;
            P[0] = (unsigned long long)__double_as_longlong(best);
            P[1] = best_i;
            P[2] = unseeded;
        }
    }
}

// n partials -> info[1] unseeded voxels, [2] the arg-max, [3] its D2 bits
__global__ __launch_bounds__(256) void k_edt_fold(const unsigned long long* part, int64_t n, unsigned long long* info) {
    __shared__ double sb[256];
    __shared__ uint32_t si[256];
    __shared__ unsigned long long su[256];
    double best = -1.0;
    uint32_t best_i = 0;
    unsigned long long unseeded = 0;
    for (int64_t i = threadIdx.x; i < n; i += 256) {
        const double d = __longlong_as_double((long long)part[i * EDT_PART_WORDS]);
        const uint32_t x = (uint32_t)part[i * EDT_PART_WORDS + 1];
        unseeded += part[i * EDT_PART_WORDS + 2];
        if (d > best || (d == best && x < best_i)) {
            best = d;
            best_i = x;
        }
    }
    sb[threadIdx.x] = best;
    si[threadIdx.x] = best_i;
    su[threadIdx.x] = unseeded;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < 256; ++k) {
            unseeded += su[k];
            if (sb[k] > best || (sb[k] == best && si[k] < best_i)) {
                best = sb[k];
                best_i = si[k];
            }
        }
        info[1] = unseeded;
        info[2] = best_i;
        info[3] = (unsigned long long)__double_as_longlong(best);
    }
}

template <bool IN32, bool FINAL>
void launch_line(const EdtLineArgs& A, const EdtLinePlan& P, hipStream_t s) {
    if (P.lds) hipLaunchKernelGGL((k_edt_line<IN32, FINAL, true>), dim3((unsigned)P.grid), dim3(WAVE), 0, s, A, P.groups);
    else hipLaunchKernelGGL((k_edt_line<IN32, FINAL, false>), dim3((unsigned)P.grid), dim3(WAVE), 0, s, A, P.groups);
}

}  // namespace

hipError_t launch_edt_x(const EdtSrc& A, int kind, uint16_t* out, unsigned long long* info, hipStream_t s) {
    const unsigned grid = (unsigned)edt_x_grid((int64_t)A.box.n[0] * A.box.n[1]);
    const dim3 block(EDT_X_WAVES * WAVE);
    if (kind == 0) hipLaunchKernelGGL(k_edt_x<0>, dim3(grid), block, 0, s, A, out, info);
    else if (kind == 1) hipLaunchKernelGGL(k_edt_x<1>, dim3(grid), block, 0, s, A, out, info);
    else if (kind == 2) hipLaunchKernelGGL(k_edt_x<2>, dim3(grid), block, 0, s, A, out, info);
    else hipLaunchKernelGGL(k_edt_x<3>, dim3(grid), block, 0, s, A, out, info);
    return hipGetLastError();
}

hipError_t launch_edt_line(const EdtLineArgs& A, const EdtLinePlan& P, hipStream_t s) {
    if (!A.final_pass) launch_line<false, false>(A, P, s);   // the y pass before a z pass
    else if (A.in32) launch_line<true, true>(A, P, s);
    else launch_line<false, true>(A, P, s);
    return hipGetLastError();
}

hipError_t launch_edt_fold(const unsigned long long* part, int64_t n, unsigned long long* info, hipStream_t s) {
    hipLaunchKernelGGL(k_edt_fold, dim3(1), dim3(256), 0, s, part, n, info);
    return hipGetLastError();
}

}  // namespace ctg
