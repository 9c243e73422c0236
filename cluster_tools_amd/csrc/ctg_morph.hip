// Segment morphology (MorphologyWorkflow): per label the voxel count, the
// coordinate sums (centre of mass) and the bounding box.  Replaces the array
// work of ndist.computeAndSerializeMorphology (morphology/block_morphology.py:134)
// and ndist.mergeAndSerializeMorphology (morphology/merge_morphology.py:130).
//
//   k_morph_scan   box of labels -> (key = label, 10-word moments) records, one
//                  per (tile flush, label): a tile-table scan (ctg_tile_table.h)
//   k_morph_merge  float64 rows [id, size, com, min, max] -> the same records
//   sort_and_number   (key, record slot) sorted by key, the distinct labels numbered
//   k_morph_runs   per label: n and the three sums add in u64, the box folds: a
//                  run fold (ctg_run_fold.h)
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
#include <hip/hip_runtime.h>

#include "ctg_run_fold.h"

namespace ctg {

#ifndef CTG_MORPH_CAP
#define CTG_MORPH_CAP 512
#endif
constexpr int MO_CAP = CTG_MORPH_CAP;   // LDS table entries (A/B builds: make variant EXTRA=-DCTG_MORPH_CAP=...)
constexpr uint32_t MO_EMPTY = 0xFFFFFFFFu;
constexpr int MO_SY = 19, MO_SZ = 35;   // bit positions of sum y / sum z in the packed sums
static_assert(WAVE * TILE_Y * TT_TILE_Z * (WAVE - 1) < (1 << MO_SY) &&
                  WAVE * TILE_Y * TT_TILE_Z * (TILE_Y - 1) < (1 << (MO_SZ - MO_SY)) &&
                  (uint64_t)WAVE * TILE_Y * TT_TILE_Z * (TT_TILE_Z - 1) < (1ull << (64 - MO_SZ)) && TILE_Y <= 8 &&
                  TT_TILE_Z <= 24,
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

// The tile-table policy of the morphology (the entry's words: the header).  A
// head of the run [x0, x0 + run) of row (z, y) adds, in tile-local coordinates,
// run to cnt, (run * x0 + run (run - 1) / 2, run * y, run * z) to the packed
// sums, and ors the run's x bits and its y and z bits into the occupancy words;
// a flushed entry is converted to array coordinates (sum z = sum z_local +
// n * z0, ...).  A label >= 2^32 raises bit 0 of label_overflow.
template <typename LabelT>
struct MorphTable {
    using Key = uint32_t;
    static constexpr Key EMPTY = MO_EMPTY;
    static constexpr int CAP = MO_CAP;
    static constexpr bool SET = false, HOLES = false;
    struct Add {
        uint64_t sums, xbits;
        uint32_t run, yzbits;
    };
    const LabelT* __restrict__ A;
    uint32_t* keys;
    uint32_t* tcnt;
    uint64_t* tsum;
    uint64_t* txo;
    uint32_t* tyz;
    uint64_t* __restrict__ rkey;
    uint64_t* __restrict__ rec;
    unsigned long long* count;
    Counters* C;
    __device__ uint64_t load(int64_t p, bool in) const { return in ? (uint64_t)A[p] : 0ull; }
    __device__ bool valid(uint64_t, bool in) const { return in; }
    __device__ Key key(uint64_t a) const { return (uint32_t)a; }
    __device__ uint32_t overflow(uint64_t a) const { return (a >> 32) ? 1u : 0u; }
    __device__ NoFold fold(uint64_t, bool, uint64_t, int) const { return {}; }
    __device__ Add head(uint32_t run, int lane, int dy, int lz, NoFold) const {
        return Add{(uint64_t)(run * (uint32_t)lane + run * (run - 1u) / 2u) | (uint64_t)(run * (uint32_t)dy) << MO_SY |
                       (uint64_t)(run * (uint32_t)lz) << MO_SZ,
                   (run == WAVE ? ~0ull : (1ull << run) - 1ull) << lane, run, (1u << dy) | (1u << (8 + lz))};
    }
    __device__ void add(uint32_t h, const Add& a) const {
        atomicAdd(&tcnt[h], a.run);
        atomicAdd((unsigned long long*)&tsum[h], (unsigned long long)a.sums);
        atomicOr((unsigned long long*)&txo[h], (unsigned long long)a.xbits);
        atomicOr(&tyz[h], a.yzbits);
    }
    __device__ void put_direct(uint64_t slot, Key key, uint32_t run, int64_t z, int64_t y, int64_t x, NoFold) const {
        const uint64_t r = run;
        morph_put(rkey, rec, slot, key, r, r * (uint64_t)z, r * (uint64_t)y, r * (uint64_t)x + r * (r - 1) / 2,
                  (uint64_t)z, (uint64_t)y, (uint64_t)x, (uint64_t)z, (uint64_t)y, (uint64_t)x + r - 1);
    }
    __device__ void put_flush(uint64_t slot, int e, Key key, const TileBox& t) const {
        const uint64_t n = tcnt[e], sm = tsum[e], xo = txo[e];
        const uint32_t yo = tyz[e] & 0xFFu, zo = tyz[e] >> 8;
        morph_put(rkey, rec, slot, key, n, (sm >> MO_SZ) + n * (uint64_t)t.z0,
                  ((sm >> MO_SY) & ((1ull << (MO_SZ - MO_SY)) - 1ull)) + n * (uint64_t)t.y0,
                  (sm & ((1ull << MO_SY) - 1ull)) + n * (uint64_t)t.x0, (uint64_t)(t.z0 + __ffs((int)zo) - 1),
                  (uint64_t)(t.y0 + __ffs((int)yo) - 1), (uint64_t)(t.x0 + __ffsll((unsigned long long)xo) - 1),
                  (uint64_t)(t.z0 + 31 - __clz((int)zo)), (uint64_t)(t.y0 + 31 - __clz((int)yo)),
                  (uint64_t)(t.x0 + 63 - __clzll((long long)xo)));
    }
    __device__ void clear(int e) const {
        keys[e] = EMPTY;
        tcnt[e] = 0;
        tsum[e] = 0;
        txo[e] = 0;
        tyz[e] = 0;
    }
};

template <typename LabelT>
__global__ __launch_bounds__(TT_THREADS) void k_morph_scan(const LabelT* __restrict__ A, int64_t Y, int64_t X,
                                                            int64_t bz, int64_t by, int64_t bx, int64_t ez,
                                                            int64_t ey, int64_t ex, uint64_t* __restrict__ rkey,
                                                            uint64_t* __restrict__ rec, int64_t cap, Counters* C) {
    __shared__ uint64_t tsum[MO_CAP];
    __shared__ uint64_t txo[MO_CAP];
    __shared__ uint32_t tkey[MO_CAP];
    __shared__ uint32_t tcnt[MO_CAP];
    __shared__ uint32_t tyz[MO_CAP];
    const MorphTable<LabelT> pol{A, tkey, tcnt, tsum, txo, tyz, rkey, rec, &C->n_records, C};
    tile_table_scan(pol, tile_of_grid(Y, X, bz, by, bx, ez, ey, ex), cap);
}

template <typename LabelT>
static hipError_t launch_morph_scan_t(const void* A, const int64_t* shape, const int64_t* b, const int64_t* e,
                                      uint64_t* rkey, uint64_t* rec, int64_t cap, Counters* C, hipStream_t s) {
    dim3 grid;
    CTG_TRY(tile_grid(b, e, &grid));
    hipLaunchKernelGGL((k_morph_scan<LabelT>), grid, dim3(TT_THREADS), 0, s, (const LabelT*)A, shape[1], shape[2],
                       b[0], b[1], b[2], e[0], e[1], e[2], rkey, rec, cap, C);
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

// the identity of k_morph_runs' folds: sums 0, min all ones, max 0
__global__ void k_morph_init(int64_t N, uint64_t* __restrict__ mom) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N * MORPH_WORDS) return;
    const int c = (int)(i % MORPH_WORDS);
    mom[i] = (c >= 4 && c < 7) ? ~0ull : 0ull;
}

// The run-fold policy of the morphology (ctg_run_fold.h): sorted position i
// holds the 10-word record slot[i]; n and the three sums add, the box folds by
// min / max, all in u64, onto the label's row of mom (k_morph_init's identities
// before the launch).  A run head writes the label.
struct MorphRuns {
    using Value = uint64_t[MORPH_WORDS];
    const uint64_t *__restrict__ key, *__restrict__ rec;
    const uint32_t* __restrict__ slot;
    int64_t n_rec;
    uint64_t* __restrict__ nodes;
    unsigned long long* __restrict__ mom;
    __device__ __forceinline__ void load(Value& v, int64_t i, bool in) const {
        if (in) {
            const uint32_t j = slot[i];
            CTG_IDX(j, n_rec);
            for (int c = 0; c < MORPH_WORDS; ++c) v[c] = rec[(int64_t)j * MORPH_WORDS + c];
        } else {
            for (int c = 0; c < MORPH_WORDS; ++c) v[c] = (c >= 4 && c < 7) ? ~0ull : 0ull;
        }
    }
    __device__ __forceinline__ void combine(Value& v, int o, bool take) const {
#pragma unroll
        for (int c = 0; c < MORPH_WORDS; ++c) {
            const uint64_t vo = shfl_down_u64(v[c], o);
            if (take) v[c] = c < 4 ? v[c] + vo : c < 7 ? (vo < v[c] ? vo : v[c]) : (vo > v[c] ? vo : v[c]);
        }
    }
    __device__ __forceinline__ void apply(uint32_t seg, const Value& v) const {
        unsigned long long* m = mom + (int64_t)seg * MORPH_WORDS;
        for (int c = 0; c < 4; ++c) atomicAdd(&m[c], (unsigned long long)v[c]);
        for (int c = 4; c < 7; ++c) atomicMin(&m[c], (unsigned long long)v[c]);
        for (int c = 7; c < 10; ++c) atomicMax(&m[c], (unsigned long long)v[c]);
    }
    __device__ __forceinline__ void name(int64_t i, uint32_t seg, bool head, uint64_t, uint64_t) const {
        if (head) nodes[seg] = key[i];
    }
};

__global__ __launch_bounds__(256) void k_morph_runs(int64_t n, const uint64_t* __restrict__ key,
                                                    const uint32_t* __restrict__ slot,
                                                    const uint64_t* __restrict__ scan,
                                                    const uint64_t* __restrict__ rec, int64_t n_rec,
                                                    uint64_t* __restrict__ nodes,
                                                    unsigned long long* __restrict__ mom, int64_t N) {
    run_fold(MorphRuns{key, rec, slot, n_rec, nodes, mom}, n, scan, N);
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

// n (key, record) pairs -> r's nodes and moments (array coordinates + origin);
// keys compare in their low end_bit bits
static hipError_t morph_reduce(Workspace& w, const uint64_t* key, const uint64_t* rec, int64_t n, unsigned end_bit,
                               const int64_t* origin, hipStream_t s, ctg_result* r) {
    return fold_records<true, uint32_t>(
        w, key, nullptr, n, end_bit, s,
        [&](const uint64_t* ks, const uint32_t* is, const uint64_t* scan, int64_t N, int64_t) {
            DevBuf<uint64_t> nodes((size_t)N * 8), mom((size_t)N * MORPH_WORDS * 8);
            if (!nodes || !mom) return hipErrorOutOfMemory;
            hipLaunchKernelGGL(k_morph_init, grid_for(N * MORPH_WORDS), dim3(256), 0, s, N, mom.p);
            CTG_TRY(hipGetLastError());
            hipLaunchKernelGGL(k_morph_runs, grid_for(n), dim3(256), 0, s, n, ks, is, scan, rec, n, nodes.p,
                               (unsigned long long*)mom.p, N);
            CTG_TRY(hipGetLastError());
            hipLaunchKernelGGL(k_morph_finish, grid_for(N), dim3(256), 0, s, N, mom.p, (uint64_t)origin[0],
                               (uint64_t)origin[1], (uint64_t)origin[2]);
            CTG_TRY(hipGetLastError());
            swap_in(r->nodes, nodes);
            swap_in(r->moments, mom);
            r->n_nodes = N;
            return hipSuccess;
        });
}

hipError_t morph_tables(Workspace& w, const void* A, int bits, const int64_t* shape, const int64_t* b,
                        const int64_t* e, const int64_t* origin, hipStream_t s, ctg_result* r, unsigned* overflow) {
    return scan_tables<uint64_t>(
        w, (e[0] - b[0]) * (e[1] - b[1]) * (e[2] - b[2]), s, MORPH_WORDS,
        [&](uint64_t* rkey, uint64_t* rec, int64_t cap) {
            return bits == 32 ? launch_morph_scan_t<uint32_t>(A, shape, b, e, rkey, rec, cap, w.counters, s)
                              : launch_morph_scan_t<uint64_t>(A, shape, b, e, rkey, rec, cap, w.counters, s);
        },
        [&](const uint64_t* k, const uint64_t* q, int64_t m) { return morph_reduce(w, k, q, m, 32u, origin, s, r); },
        false, r, overflow);   // (no ignore label: a box without records is refused)
}

hipError_t morph_merge(Workspace& w, const double* rows, int64_t n, hipStream_t s, ctg_result* r, int* bad) {
    const int64_t zero[3] = {0, 0, 0};
    return merge_rows(
        w, rows, n, MORPH_WORDS, k_morph_merge,
        [&](const uint64_t* key, const uint64_t* rec) { return morph_reduce(w, key, rec, n, 53u, zero, s, r); }, s, r,
        bad);
}

hipError_t launch_morph_rows(const ctg_result* r, uint64_t lb, uint64_t le, double* out, double* rows, hipStream_t s) {
    if (r->n_nodes == 0) return hipSuccess;
    hipLaunchKernelGGL(k_morph_rows, grid_for(r->n_nodes), dim3(256), 0, s, r->n_nodes, r->nodes, r->moments, lb, le,
                       out, rows);
    return hipGetLastError();
}

CTG_BOUNDS_TAKE(morph)

}  // namespace ctg
