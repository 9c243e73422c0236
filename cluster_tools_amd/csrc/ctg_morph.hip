// Segment morphology (MorphologyWorkflow): per label the voxel count, the
// coordinate sums (centre of mass) and the bounding box.  Replaces the array
// work of ndist.computeAndSerializeMorphology (morphology/block_morphology.py:134)
// and ndist.mergeAndSerializeMorphology (morphology/merge_morphology.py:130).
//
//   k_morph_scan   box of labels -> (key = label, 10-word moments) records, one
//                  per (tile flush, label), through an LDS table per workgroup
//   k_morph_merge  float64 rows [id, size, com, min, max] -> the same records
//   radix sort     (key, record slot) by key (rocPRIM radix_sort_pairs)
//   k_overlap_heads + inclusive scan   number the distinct labels
//   k_morph_runs   per label: n and the three sums add in u64, the box folds
//   k_morph_finish origin added in integers: sums += n * origin, box += origin
//   k_morph_rows   moments -> float64 rows, compact and / or dense over a label range
//
// Everything is integers until the one division of k_morph_rows, so a merged
// table equals the table of one call over the whole volume bit for bit -- as
// long as the merge can recover each row's integer sums: a row stores
// com = fl(S / n), and rint(com * n) == S while S < 2^51 (two roundings of
// relative error 2^-53 each: |com * n - S| <= S * 2^-52 < 1/2).  That covers a
// block of 2^32 voxels at coordinates up to 2^19.  Past the bound the merge is
// still computed; its sums, and with them the centre of mass, are then rounded.
//
// The LDS table, per entry (28 B; 512 entries = 14 KiB a workgroup), all in
// tile-local coordinates so that every update is one no-return LDS atomic:
//   key   u32   the label's low half (CAS; labels >= 2^32: Counters::label_overflow)
//   cnt   u32   voxels (add; a tile holds 2^13)
//   sums  u64   sum x (< 2^19) | sum y (< 2^16) << 19 | sum z (< 2^17) << 35 (one add)
//   xocc  u64   occupied x of the 64 (or); min / max = first / last set bit at flush
//   yzocc u32   occupied y (bits 0..7) and z (bits 8..23) (or)
// Four atomics per run head.  Six atomicMin / atomicMax words instead of the
// two occupancy words would be eight atomics per head and 44 B per entry.
// The capacity is set by occupancy, not by the labels a tile meets (about 50 at
// cell 10): the compiled scan takes 58 VGPRs and no scratch, so the LDS bounds
// the waves per SIMD -- measured at 512^3 / 1024^3, 2048 entries (56 KiB) 1.10 /
// 8.54 ms, 1024 0.51 / 3.80 ms, 512 0.40 / 2.97 ms, 256 0.41 / 3.01 ms.
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

constexpr int MO_THREADS = 256;   // 4 waves: 4 planes per step, as k_overlap_scan
constexpr int MO_TILE_Z = 16;
#ifndef CTG_MORPH_CAP
#define CTG_MORPH_CAP 512
#endif
constexpr int MO_CAP = CTG_MORPH_CAP;   // LDS table entries (A/B builds: make variant EXTRA=-DCTG_MORPH_CAP=...)
constexpr int MO_PROBES = 32;     // linear probes before a head gives up on the table
constexpr uint32_t MO_EMPTY = 0xFFFFFFFFu;
constexpr int MO_SY = 19, MO_SZ = 35;   // bit positions of sum y / sum z in the packed sums
static_assert((MO_CAP & (MO_CAP - 1)) == 0 && MO_CAP % MO_THREADS == 0, "table capacity");
static_assert(WAVE * TILE_Y * MO_TILE_Z * (WAVE - 1) < (1 << MO_SY) &&
                  WAVE * TILE_Y * MO_TILE_Z * (TILE_Y - 1) < (1 << (MO_SZ - MO_SY)) &&
                  (uint64_t)WAVE * TILE_Y * MO_TILE_Z * (MO_TILE_Z - 1) < (1ull << (64 - MO_SZ)) && TILE_Y <= 8 &&
                  MO_TILE_Z <= 24,
              "a tile's sums fit their fields");

// one record: MORPH_WORDS u64 at rec[slot * MORPH_WORDS]
__device__ __forceinline__ void morph_put(uint64_t* __restrict__ rkey, uint64_t* __restrict__ rec, uint64_t slot,
                                          uint64_t key, uint64_t n, uint64_t sz, uint64_t sy, uint64_t sx,
                                          uint64_t z0, uint64_t y0, uint64_t x0, uint64_t z1, uint64_t y1,
                                          uint64_t x1) {
    rkey[slot] = key;
    uint64_t* q = rec + slot * MORPH_WORDS;
    q[0] = n;
    q[1] = sz;
    q[2] = sy;
    q[3] = sx;
    q[4] = z0;
    q[5] = y0;
    q[6] = x0;
    q[7] = z1;
    q[8] = y1;
    q[9] = x1;
}

// One workgroup per 64 x TILE_Y x 16 tile of the box, a wave per row, lane = x.
// Equal consecutive labels collapse to their head lane (run length from the
// ballot of heads); a head of the run [x0, x0 + run) of row (z, y) adds, in
// tile-local coordinates, run to cnt, (run * x0 + run (run - 1) / 2, run * y,
// run * z) to the packed sums, and ors the run's x bits and its y and z bits
// into the occupancy words.  The table is written out when more than half full
// after a z step and at tile end, one global reservation per flush, converted to
// array coordinates (sum z = sum z_local + n * z0, ...); a head that finds no
// slot within MO_PROBES writes its record directly.  Records past `cap` are
// dropped: n_records still counts them and the host runs again with room.
template <typename LabelT>
__global__ __launch_bounds__(MO_THREADS) void k_morph_scan(const LabelT* __restrict__ A, int64_t Y, int64_t X,
                                                            int64_t bz, int64_t by, int64_t bx, int64_t ez,
                                                            int64_t ey, int64_t ex, uint64_t* __restrict__ rkey,
                                                            uint64_t* __restrict__ rec, int64_t cap, Counters* C) {
    __shared__ uint64_t tsum[MO_CAP];
    __shared__ uint64_t txo[MO_CAP];
    __shared__ uint32_t tkey[MO_CAP];
    __shared__ uint32_t tcnt[MO_CAP];
    __shared__ uint32_t tyz[MO_CAP];
    __shared__ uint32_t used;
    __shared__ uint32_t wpos;
    __shared__ unsigned long long base;
    const int tid = threadIdx.x;
    for (int e = tid; e < MO_CAP; e += MO_THREADS) {
        tkey[e] = MO_EMPTY;
        tcnt[e] = 0;
        tsum[e] = 0;
        txo[e] = 0;
        tyz[e] = 0;
    }
    if (tid == 0) used = 0;
    __syncthreads();
    const int lane = tid & (WAVE - 1), wave = tid >> 6;
    const int64_t x0 = bx + (int64_t)blockIdx.x * WAVE;
    const int64_t x = x0 + lane;
    const int64_t y0 = by + (int64_t)blockIdx.y * TILE_Y;
    const int64_t z0 = bz + (int64_t)blockIdx.z * MO_TILE_Z;
    const bool in = x < ex;
    uint32_t over = 0;
    for (int zs = 0; zs < MO_TILE_Z; zs += MO_THREADS / WAVE) {
        const int lz = zs + wave;
        const int64_t z = z0 + lz;
        if (z < ez) {   // (wave-uniform, like the row bound below)
            for (int dy = 0; dy < TILE_Y; ++dy) {
                const int64_t y = y0 + dy;
                if (y >= ey) break;
                const uint64_t a = in ? (uint64_t)A[(z * Y + y) * X + x] : 0ull;
                if (in && (a >> 32)) over = 1u;
                const uint32_t key = (uint32_t)a;
                const uint32_t prev = __shfl_up(key, 1, WAVE);
                // (lanes below a lane inside the box are inside it too)
                const bool head = in && (lane == 0 || prev != key);
                const uint64_t bound = __ballot(head || !in);
                bool direct = false;
                uint32_t run = 0;
                if (head) {
                    const uint64_t above = lane == WAVE - 1 ? 0ull : bound >> (lane + 1);
                    run = above ? (uint32_t)__ffsll((unsigned long long)above) : (uint32_t)(WAVE - lane);
                    direct = true;
                    if (key != MO_EMPTY) {   // (the one key that looks like a free slot goes direct)
                        const uint64_t add = (uint64_t)(run * (uint32_t)lane + run * (run - 1u) / 2u) |
                                             (uint64_t)(run * (uint32_t)dy) << MO_SY |
                                             (uint64_t)(run * (uint32_t)lz) << MO_SZ;
                        const uint64_t xbits = (run == WAVE ? ~0ull : (1ull << run) - 1ull) << lane;
                        const uint32_t yzbits = (1u << dy) | (1u << (8 + lz));
                        uint32_t h = hash_key(key) & (MO_CAP - 1);
                        for (int q = 0; q < MO_PROBES; ++q) {
                            uint32_t cur = tkey[h];
                            if (cur == MO_EMPTY) {
                                cur = atomicCAS(&tkey[h], MO_EMPTY, key);
                                if (cur == MO_EMPTY) {
                                    atomicAdd(&used, 1u);
                                    cur = key;
                                }
                            }
                            if (cur == key) {
                                atomicAdd(&tcnt[h], run);
                                atomicAdd((unsigned long long*)&tsum[h], (unsigned long long)add);
                                atomicOr((unsigned long long*)&txo[h], (unsigned long long)xbits);
                                atomicOr(&tyz[h], yzbits);
                                direct = false;
                                break;
                            }
                            h = (h + 1) & (MO_CAP - 1);
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
                        const uint64_t r = run;
                        morph_put(rkey, rec, b0 + rank, key, r, r * (uint64_t)z, r * (uint64_t)y,
                                  r * (uint64_t)x + r * (r - 1) / 2, (uint64_t)z, (uint64_t)y, (uint64_t)x, (uint64_t)z,
                                  (uint64_t)y, (uint64_t)x + r - 1);
                    }
                }
            }
        }
        __syncthreads();
        if (used > MO_CAP / 2 || zs + MO_THREADS / WAVE >= MO_TILE_Z) {   // (uniform: read after the barrier)
            if (tid == 0) {
                base = used ? atomicAdd(&C->n_records, (unsigned long long)used) : 0ull;
                wpos = 0;
            }
            __syncthreads();
            // compaction order is irrelevant (sorted afterwards)
            for (int e = tid; e < MO_CAP; e += MO_THREADS) {
                const uint32_t k = tkey[e];
                const bool live = k != MO_EMPTY;
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
                            const uint64_t n = tcnt[e], sm = tsum[e], xo = txo[e];
                            const uint32_t yo = tyz[e] & 0xFFu, zo = tyz[e] >> 8;
                            morph_put(rkey, rec, slot, k, n, (sm >> MO_SZ) + n * (uint64_t)z0,
                                      ((sm >> MO_SY) & ((1ull << (MO_SZ - MO_SY)) - 1ull)) + n * (uint64_t)y0,
                                      (sm & ((1ull << MO_SY) - 1ull)) + n * (uint64_t)x0,
                                      (uint64_t)(z0 + __ffs((int)zo) - 1), (uint64_t)(y0 + __ffs((int)yo) - 1),
                                      (uint64_t)(x0 + __ffsll((unsigned long long)xo) - 1),
                                      (uint64_t)(z0 + 31 - __clz((int)zo)), (uint64_t)(y0 + 31 - __clz((int)yo)),
                                      (uint64_t)(x0 + 63 - __clzll((long long)xo)));
                        }
                        tkey[e] = MO_EMPTY;
                        tcnt[e] = 0;
                        tsum[e] = 0;
                        txo[e] = 0;
                        tyz[e] = 0;
                    }
                }
            }
            __syncthreads();
            if (tid == 0) used = 0;
            __syncthreads();
        }
    }
    over = (uint32_t)__any((int)over);
    if (lane == 0 && over) atomicOr(&C->label_overflow, 1ull);
}

template <typename LabelT>
static hipError_t launch_morph_scan_t(const void* A, const int64_t* shape, const int64_t* b, const int64_t* e,
                                      uint64_t* rkey, uint64_t* rec, int64_t cap, Counters* C, hipStream_t s) {
    const int64_t gx = (e[2] - b[2] + WAVE - 1) / WAVE, gy = (e[1] - b[1] + TILE_Y - 1) / TILE_Y,
                  gz = (e[0] - b[0] + MO_TILE_Z - 1) / MO_TILE_Z;
    if (gx > 0x7FFFFFFFll || gy > 65535 || gz > 65535) return hipErrorInvalidValue;
    hipLaunchKernelGGL((k_morph_scan<LabelT>), dim3((unsigned)gx, (unsigned)gy, (unsigned)gz), dim3(MO_THREADS), 0, s,
                       (const LabelT*)A, shape[1], shape[2], b[0], b[1], b[2], e[0], e[1], e[2], rkey, rec, cap, C);
    return hipGetLastError();
}

// row i of [id, size, com z y x, min z y x, max z y x] -> key i, record i.  The
// integer sum of a row is rint(com * size) (exact below 2^51: the header).
__global__ void k_morph_merge(int64_t n, const double* __restrict__ rows, uint64_t* __restrict__ key,
                              uint64_t* __restrict__ rec, unsigned long long* bad) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double* r = rows + i * CTG_MORPH_COLS;
    const double two53 = 9007199254740992.0, two63 = 9223372036854775808.0;
    const double id = r[0], size = r[1];
    bool ok = id >= 0.0 && id < two53 && id == rint(id) && size >= 0.0 && size < two53;
    uint64_t q[MORPH_WORDS];
    q[0] = ok ? (uint64_t)size : 0ull;
    for (int c = 0; c < 3; ++c) {
        const double sum = rint(r[2 + c] * size);
        ok = ok && sum >= 0.0 && sum < two63;
        q[1 + c] = ok ? (uint64_t)sum : 0ull;
    }
    for (int c = 0; c < 6; ++c) {
        const double v = r[5 + c];
        ok = ok && v >= 0.0 && v < two53;
        q[4 + c] = ok ? (uint64_t)v : 0ull;
    }
    if (ok && q[0] == 0) {   // a row without voxels (the zero row of an absent label) adds nothing
        for (int c = 1; c < 4; ++c) q[c] = 0;
        for (int c = 4; c < 7; ++c) q[c] = ~0ull;
        for (int c = 7; c < 10; ++c) q[c] = 0;
    }
    if (!ok) atomicOr(bad, 1ull);
    key[i] = ok ? (uint64_t)id : 0ull;
    for (int c = 0; c < MORPH_WORDS; ++c) rec[i * MORPH_WORDS + c] = q[c];
}

__global__ void k_morph_iota(int64_t n, uint32_t* __restrict__ idx) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) idx[i] = (uint32_t)i;
}

// the identity of k_morph_runs' folds: sums 0, min all ones, max 0
__global__ void k_morph_init(int64_t N, uint64_t* __restrict__ mom) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N * MORPH_WORDS) return;
    const int c = (int)(i % MORPH_WORDS);
    mom[i] = (c >= 4 && c < 7) ? ~0ull : 0ull;
}

// Sorted position i holds record slot[i] of label number scan[i].lo - 1.  A
// wave folds the records of its 64 positions per label (segmented suffix folds
// by shuffles: add for n and the sums, min / max for the box) and the first
// lane of every segment applies the fold to the label's row -- one atomic set
// per (wave, label), none contended unless a label spans waves.  mom is
// initialised by k_morph_init before the launch.
__global__ __launch_bounds__(256) void k_morph_runs(int64_t n, const uint64_t* __restrict__ key,
                                                    const uint32_t* __restrict__ slot,
                                                    const uint64_t* __restrict__ scan,
                                                    const uint64_t* __restrict__ rec, int64_t n_rec,
                                                    uint64_t* __restrict__ nodes,
                                                    unsigned long long* __restrict__ mom, int64_t N) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = threadIdx.x & (WAVE - 1);
    const bool in = i < n;
    const uint64_t sc = in ? scan[i] : 0ull, sp = (in && i) ? scan[i - 1] : 0ull;
    const uint32_t seg = in ? (uint32_t)sc - 1u : 0xFFFFFFFFu;   // (labels < 2^32 - 1: the record limit)
    uint64_t v[MORPH_WORDS];
    if (in) {
        const uint32_t j = slot[i];
        CTG_IDX(j, n_rec);
        for (int c = 0; c < MORPH_WORDS; ++c) v[c] = rec[(int64_t)j * MORPH_WORDS + c];
    } else {
        for (int c = 0; c < MORPH_WORDS; ++c) v[c] = (c >= 4 && c < 7) ? ~0ull : 0ull;
    }
    for (int o = 1; o < WAVE; o <<= 1) {
        const uint32_t so = __shfl_down(seg, o, WAVE);
        const bool take = lane + o < WAVE && so == seg;
#pragma unroll
        for (int c = 0; c < MORPH_WORDS; ++c) {
            const uint64_t vo = shfl_down_u64(v[c], o);
            if (take) v[c] = c < 4 ? v[c] + vo : c < 7 ? (vo < v[c] ? vo : v[c]) : (vo > v[c] ? vo : v[c]);
        }
    }
    const uint32_t sprev = __shfl_up(seg, 1, WAVE);
    if (!in) return;
    if (lane == 0 || sprev != seg) {
        CTG_IDX(seg, N);
        unsigned long long* m = mom + (int64_t)seg * MORPH_WORDS;
        for (int c = 0; c < 4; ++c) atomicAdd(&m[c], (unsigned long long)v[c]);
        for (int c = 4; c < 7; ++c) atomicMin(&m[c], (unsigned long long)v[c]);
        for (int c = 7; c < 10; ++c) atomicMax(&m[c], (unsigned long long)v[c]);
    }
    if ((uint32_t)sc != (uint32_t)sp) nodes[seg] = key[i];
}

// coordinates = array index + origin: sums += n * origin, box += origin; a
// label without voxels (merge rows of size 0 only) gets an empty box of zeros
__global__ void k_morph_finish(int64_t N, uint64_t* __restrict__ mom, uint64_t oz, uint64_t oy, uint64_t ox) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= N) return;
    uint64_t* m = mom + j * MORPH_WORDS;
    const uint64_t n = m[0], o[3] = {oz, oy, ox};
    for (int c = 0; c < 3; ++c) {
        m[1 + c] += n * o[c];
        m[4 + c] = n ? m[4 + c] + o[c] : 0ull;
        m[7 + c] = n ? m[7 + c] + o[c] : 0ull;
    }
}

// One thread per label: its float64 row [id, size, com z y x, min z y x,
// max z y x], com = (double)sum / (double)n, into rows[j] and, for labels in
// [lb, le), into out[label - lb] (zeroed before the launch).  A label without
// voxels keeps a zero row.
__global__ void k_morph_rows(int64_t N, const uint64_t* __restrict__ nodes, const uint64_t* __restrict__ mom,
                             uint64_t lb, uint64_t le, double* __restrict__ out, double* __restrict__ rows) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= N) return;
    const uint64_t a = nodes[j];
    const uint64_t* m = mom + j * MORPH_WORDS;
    const uint64_t n = m[0];
    double r[CTG_MORPH_COLS];
    r[0] = (double)a;
    r[1] = (double)n;
    for (int c = 0; c < 3; ++c) r[2 + c] = n ? (double)m[1 + c] / (double)n : 0.0;
    for (int c = 0; c < 6; ++c) r[5 + c] = (double)m[4 + c];
    if (rows)
        for (int c = 0; c < CTG_MORPH_COLS; ++c) rows[j * CTG_MORPH_COLS + c] = r[c];
    if (out && n && a >= lb && a < le)
        for (int c = 0; c < CTG_MORPH_COLS; ++c) out[(a - lb) * CTG_MORPH_COLS + c] = r[c];
}

static dim3 grid_for(int64_t n) { return dim3((unsigned)((n + 255) / 256)); }

// n (key, record) pairs -> r's nodes and moments (array coordinates + origin):
// sort the record slots by key, number the labels, fold.  n in (0, 2^32 - 1);
// keys compare in their low end_bit bits.
static hipError_t morph_reduce(Workspace& w, const uint64_t* key, const uint64_t* rec, int64_t n, unsigned end_bit,
                               const int64_t* origin, hipStream_t s, ctg_result* r) {
    Ev ev{w, s};
    DevBuf<uint64_t> ks((size_t)n * 8), flags((size_t)n * 8), scan((size_t)n * 8);
    DevBuf<uint32_t> idx((size_t)n * 4), is((size_t)n * 4);
    if (!ks || !flags || !scan || !idx || !is) return hipErrorOutOfMemory;
    hipLaunchKernelGGL(k_morph_iota, grid_for(n), dim3(256), 0, s, n, idx.p);
    CTG_TRY(hipGetLastError());
    CTG_TRY(with_temp(w.temp, [&](void* t, size_t& tb) {
        return rocprim::radix_sort_pairs(t, tb, key, ks.p, idx.p, is.p, (size_t)n, 0u, end_bit, s);
    }));
    ev.mark(3);
    CTG_TRY(launch_overlap_heads(n, ks, flags, s));
    CTG_TRY(with_temp(w.temp, [&](void* t, size_t& tb) {
        return rocprim::inclusive_scan(t, tb, flags.p, scan.p, (size_t)n, rocprim::plus<uint64_t>(), s);
    }));
    uint64_t last = 0;
    CTG_TRY(hipMemcpyAsync(&last, scan.p + (n - 1), 8, hipMemcpyDeviceToHost, s));
    CTG_TRY(hipStreamSynchronize(s));
    flags.reset();
    idx.reset();
    const int64_t N = (int64_t)(uint32_t)last;
    ev.mark(4);
    DevBuf<uint64_t> nodes((size_t)N * 8), mom((size_t)N * MORPH_WORDS * 8);
    if (!nodes || !mom) return hipErrorOutOfMemory;
    hipLaunchKernelGGL(k_morph_init, grid_for(N * MORPH_WORDS), dim3(256), 0, s, N, mom.p);
    CTG_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_morph_runs, grid_for(n), dim3(256), 0, s, n, ks.p, is.p, scan.p, rec, n, nodes.p,
                       (unsigned long long*)mom.p, N);
    CTG_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_morph_finish, grid_for(N), dim3(256), 0, s, N, mom.p, (uint64_t)origin[0],
                       (uint64_t)origin[1], (uint64_t)origin[2]);
    CTG_TRY(hipGetLastError());
    ev.mark(5);
    dev_free(r->nodes);
    dev_free(r->moments);
    r->nodes = nodes.release();
    r->moments = mom.release();
    r->n_nodes = N;
    return hipSuccess;
}

hipError_t morph_tables(Workspace& w, const void* A, int bits, const int64_t* shape, const int64_t* b,
                        const int64_t* e, const int64_t* origin, hipStream_t s, ctg_result* r, unsigned* overflow) {
    *overflow = 0;
    Ev ev{w, s};
    const int64_t nb = (e[0] - b[0]) * (e[1] - b[1]) * (e[2] - b[2]);
    // a record per voxel at most; coarse labellings need a small fraction of that
    int64_t cap = std::min<int64_t>(nb, std::max<int64_t>(1 << 12, nb / 16));
    for (int attempt = 0; attempt < 3; ++attempt) {
        DevBuf<uint64_t> rkey((size_t)cap * 8), rec((size_t)cap * MORPH_WORDS * 8);
        if (!rkey || !rec) return hipErrorOutOfMemory;
        CTG_TRY(hipMemsetAsync(w.counters, 0, sizeof(Counters), s));
        ev.mark(0);
        CTG_TRY(bits == 32 ? launch_morph_scan_t<uint32_t>(A, shape, b, e, rkey, rec, cap, w.counters, s)
                           : launch_morph_scan_t<uint64_t>(A, shape, b, e, rkey, rec, cap, w.counters, s));
        ev.mark(1);
        ev.mark(2);
        CTG_TRY(hipMemcpyAsync(w.counters_host, w.counters, sizeof(Counters), hipMemcpyDeviceToHost, s));
        CTG_TRY(hipStreamSynchronize(s));
        if (w.counters_host->label_overflow) {
            *overflow = 1;
            return hipSuccess;
        }
        const int64_t m = (int64_t)w.counters_host->n_records;
        if (m > cap) {
            // which heads miss the table depends on the order of arrival, so a
            // second run may count a few more: the third gets a slot per voxel
            cap = attempt == 0 ? std::min<int64_t>(nb, m + m / 8 + 1024) : nb;
            continue;
        }
        if (m <= 0 || m >= 0xFFFFFFFFll) return hipErrorInvalidValue;   // (the API refuses empty and 2^32-voxel boxes)
        r->n_records = m;
        r->n_direct = (int64_t)w.counters_host->n_direct;
        CTG_TRY(morph_reduce(w, rkey, rec, m, 32u, origin, s, r));
        ev.mark(6);
        return hipSuccess;
    }
    return hipErrorOutOfMemory;   // (unreachable: the third attempt holds every voxel)
}

hipError_t morph_merge(Workspace& w, const double* rows, int64_t n, hipStream_t s, ctg_result* r, int* bad) {
    *bad = 0;
    Ev ev{w, s};
    DevBuf<uint64_t> key((size_t)n * 8), rec((size_t)n * MORPH_WORDS * 8);
    if (!key || !rec) return hipErrorOutOfMemory;
    CTG_TRY(hipMemsetAsync(w.counters, 0, sizeof(Counters), s));
    ev.mark(0);
    hipLaunchKernelGGL(k_morph_merge, grid_for(n), dim3(256), 0, s, n, rows, key.p, rec.p,
                       &w.counters->label_overflow);
    CTG_TRY(hipGetLastError());
    ev.mark(1);
    ev.mark(2);
    CTG_TRY(hipMemcpyAsync(w.counters_host, w.counters, sizeof(Counters), hipMemcpyDeviceToHost, s));
    CTG_TRY(hipStreamSynchronize(s));
    if (w.counters_host->label_overflow) {
        *bad = 1;
        return hipSuccess;
    }
    const int64_t zero[3] = {0, 0, 0};
    CTG_TRY(morph_reduce(w, key, rec, n, 53u, zero, s, r));
    ev.mark(6);
    r->n_records = n;
    return hipSuccess;
}

hipError_t launch_morph_rows(const ctg_result* r, uint64_t lb, uint64_t le, double* out, double* rows, hipStream_t s) {
    if (r->n_nodes == 0) return hipSuccess;
    hipLaunchKernelGGL(k_morph_rows, grid_for(r->n_nodes), dim3(256), 0, s, r->n_nodes, r->nodes, r->moments, lb, le,
                       out, rows);
    return hipGetLastError();
}

CTG_BOUNDS_TAKE(morph)

}  // namespace ctg
