// Region features (RegionFeaturesWorkflow): per label the voxel count and the
// sum, minimum and maximum of an input map.  Replaces the array work of
// _block_features (features/region_features.py:159-185: np.unique, the dict
// relabelling, vigra.analysis.extractRegionFeatures) and of
// _extract_and_merge_region_features (features/merge_region_features.py:109-158).
//
//   k_region_scan   box of (labels, data) -> (key = label, n, sum, min, max)
//                   records, one per (tile flush, label): a tile-table scan
//                   (ctg_tile_table.h) whose heads carry their run's folded samples
//   k_region_merge  float64 rows [id, count, sum, min, max] -> the same records
//   sort_and_number   (key, record slot) sorted by key, the distinct labels numbered
//   k_region_runs   per label: n adds in u64, the sums in f64, min / max fold: a
//                   run fold (ctg_run_fold.h)
//   k_region_finish ordered min / max words -> f32; zeros for a label without voxels
//   k_region_rows   moments -> float64 rows of either form, compact and / or dense
//
// Sums stay sums until the one division of k_region_rows.  Every addend is an
// f32 sample (or a u8 value) widened to f64, hence exact; the adds happen in no
// fixed order (LDS and global atomics), so the result is the same bits in every
// run only where every partial sum is representable -- u8 data, f32 data on a
// grid such as k / 256 -- and within 2 (n - 1) 2^-53 sum|x| of any other order
// otherwise (ctg.h).
//
// The LDS table, per entry (24 B; 512 entries = 12 KiB a workgroup):
//   key  u32   the label's low half (CAS; labels >= 2^32: Counters::label_overflow)
//   cnt  u32   voxels (add; a tile holds 2^13)
//   sum  f64   sum of the samples (add)
//   mn   u32   f2ord(minimum) (min)
//   mx   u32   f2ord(maximum) (max)
// Four no-return LDS atomics per run head, after the segmented fold of the
// run's samples over the wave (RegionTable::fold).
#include <hip/hip_runtime.h>

#include "ctg_run_fold.h"

namespace ctg {

#ifndef CTG_REGION_CAP
#define CTG_REGION_CAP 512
#endif
constexpr int RG_CAP = CTG_REGION_CAP;   // LDS table entries (A/B builds: make variant EXTRA=-DCTG_REGION_CAP=...)
constexpr uint32_t RG_EMPTY = 0xFFFFFFFFu;

// one record: REGION_WORDS u64 at rec[slot * REGION_WORDS]: n, the sum's bits,
// f2ord(min) | f2ord(max) << 32
__device__ __forceinline__ void region_put(uint64_t* __restrict__ rkey, uint64_t* __restrict__ rec, uint64_t slot,
                                           uint64_t key, uint64_t n, double sum, uint32_t mn, uint32_t mx) {
    rkey[slot] = key;
    uint64_t* q = rec + slot * REGION_WORDS;
    q[0] = n;
    q[1] = (uint64_t)__double_as_longlong(sum);
    q[2] = (uint64_t)mn | (uint64_t)mx << 32;
}

// The tile-table policy of the region features (the entry's words: the
// header).  Voxels whose label equals `ignore` are skipped (HOLES).  fold gives
// every lane the sum, minimum and maximum of the samples from itself to the end
// of its run -- segmented suffix folds by shuffles: at distance o a lane takes
// its partner's fold if no head and no skipped lane lies in (lane, lane + o],
// so nothing crosses a hole or a head; skipped lanes hold the identities and
// are never taken from -- and a head adds its own, the whole run's.  A label
// >= 2^32 raises bit 0 of label_overflow.
template <typename LabelT, typename DataT, bool HOLES_>
struct RegionTable {
    using Key = uint32_t;
    static constexpr Key EMPTY = RG_EMPTY;
    static constexpr int CAP = RG_CAP;
    static constexpr bool SET = false, HOLES = HOLES_;
    struct Voxel {
        uint64_t a;
        float x;
    };
    struct Fold {
        double sum;
        float mn, mx;
    };
    struct Add {
        double sum;
        uint32_t run, mn, mx;
    };
    const LabelT* __restrict__ A;
    const DataT* __restrict__ D;
    uint64_t ignore;
    uint32_t* keys;
    uint32_t* tcnt;
    double* tsum;
    uint32_t* tmn;
    uint32_t* tmx;
    uint64_t* __restrict__ rkey;
    uint64_t* __restrict__ rec;
    unsigned long long* count;
    Counters* C;
    __device__ Voxel load(int64_t p, bool in) const { return Voxel{in ? (uint64_t)A[p] : 0ull, in ? (float)D[p] : 0.0f}; }
    __device__ bool valid(const Voxel& v, bool in) const { return in && !(HOLES && v.a == ignore); }
    __device__ Key key(const Voxel& v) const { return (uint32_t)v.a; }
    __device__ uint32_t overflow(const Voxel& v) const { return (v.a >> 32) ? 1u : 0u; }
    __device__ Fold fold(const Voxel& v, bool valid, uint64_t bound, int lane) const {
        Fold f{valid ? (double)v.x : 0.0, valid ? v.x : __builtin_inff(), valid ? v.x : -__builtin_inff()};
        // how many lanes follow this one in its run: up to the next head or skipped lane (a skipped
        // lane's follower is a head or skipped, so it takes nothing)
        const uint64_t above = lane == WAVE - 1 ? 0ull : bound >> (lane + 1);
        const int rem = above ? __ffsll((unsigned long long)above) - 1 : WAVE - 1 - lane;
        // distance 1: the partner's fold is still its sample -- one shuffle, not four
        if (!__ballot(rem >= 1)) return f;   // (wave-uniform: every lane a head or skipped)
        const float x1 = __shfl_down(v.x, 1, WAVE);
        if (rem >= 1) {
            f.sum += (double)x1;
            f.mn = x1 < f.mn ? x1 : f.mn;
            f.mx = x1 > f.mx ? x1 : f.mx;
        }
        for (int o = 2; o < WAVE; o <<= 1) {
            const bool take = rem >= o;
            if (!__ballot(take)) break;   // (wave-uniform: no run reaches o lanes, nor any longer distance)
            const double so = __longlong_as_double((long long)shfl_down_u64((uint64_t)__double_as_longlong(f.sum), o));
            const float no = __shfl_down(f.mn, o, WAVE), xo = __shfl_down(f.mx, o, WAVE);
            if (take) {
                f.sum += so;
                f.mn = no < f.mn ? no : f.mn;
                f.mx = xo > f.mx ? xo : f.mx;
            }
        }
        return f;
    }
    __device__ Add head(uint32_t run, int, int, int, const Fold& f) const {
        return Add{f.sum, run, f2ord(f.mn), f2ord(f.mx)};
    }
    __device__ void add(uint32_t h, const Add& a) const {
        atomicAdd(&tcnt[h], a.run);
        atomicAdd(&tsum[h], a.sum);
        atomicMin(&tmn[h], a.mn);
        atomicMax(&tmx[h], a.mx);
    }
    __device__ void put_direct(uint64_t slot, Key key, uint32_t run, int64_t, int64_t, int64_t, const Fold& f) const {
        region_put(rkey, rec, slot, key, run, f.sum, f2ord(f.mn), f2ord(f.mx));
    }
    __device__ void put_flush(uint64_t slot, int e, Key key, const TileBox&) const {
        region_put(rkey, rec, slot, key, tcnt[e], tsum[e], tmn[e], tmx[e]);
    }
    __device__ void clear(int e) const {
        keys[e] = EMPTY;
        tcnt[e] = 0;
        tsum[e] = 0.0;
        tmn[e] = 0xFFFFFFFFu;
        tmx[e] = 0u;
    }
};

template <typename LabelT, typename DataT, bool HOLES>
__global__ __launch_bounds__(TT_THREADS) void k_region_scan(const LabelT* __restrict__ A, const DataT* __restrict__ D,
                                                             int64_t Y, int64_t X, int64_t bz, int64_t by, int64_t bx,
                                                             int64_t ez, int64_t ey, int64_t ex, uint64_t ignore,
                                                             uint64_t* __restrict__ rkey, uint64_t* __restrict__ rec,
                                                             int64_t cap, Counters* C) {
    __shared__ double tsum[RG_CAP];
    __shared__ uint32_t tkey[RG_CAP];
    __shared__ uint32_t tcnt[RG_CAP];
    __shared__ uint32_t tmn[RG_CAP];
    __shared__ uint32_t tmx[RG_CAP];
    const RegionTable<LabelT, DataT, HOLES> pol{A, D, ignore, tkey, tcnt, tsum, tmn, tmx, rkey, rec, &C->n_records, C};
    tile_table_scan(pol, tile_of_grid(Y, X, bz, by, bx, ez, ey, ex), cap);
}

template <typename LabelT, typename DataT, bool HOLES>
static hipError_t launch_region_scan_t(const void* A, const void* D, const int64_t* shape, const int64_t* b,
                                       const int64_t* e, uint64_t ignore, uint64_t* rkey, uint64_t* rec, int64_t cap,
                                       Counters* C, hipStream_t s) {
    dim3 grid;
    CTG_TRY(tile_grid(b, e, &grid));
    hipLaunchKernelGGL((k_region_scan<LabelT, DataT, HOLES>), grid, dim3(TT_THREADS), 0, s, (const LabelT*)A,
                       (const DataT*)D, shape[1], shape[2], b[0], b[1], b[2], e[0], e[1], e[2], ignore, rkey, rec, cap,
                       C);
    return hipGetLastError();
}

template <typename LabelT, typename DataT>
static hipError_t launch_region_scan_h(const void* A, const void* D, const int64_t* shape, const int64_t* b,
                                       const int64_t* e, int has_ignore, uint64_t ignore, uint64_t* rkey,
                                       uint64_t* rec, int64_t cap, Counters* C, hipStream_t s) {
    return has_ignore ? launch_region_scan_t<LabelT, DataT, true>(A, D, shape, b, e, ignore, rkey, rec, cap, C, s)
                      : launch_region_scan_t<LabelT, DataT, false>(A, D, shape, b, e, ignore, rkey, rec, cap, C, s);
}

static hipError_t launch_region_scan(const void* A, int bits, const void* D, int kind, const int64_t* shape,
                                     const int64_t* b, const int64_t* e, int has_ignore, uint64_t ignore,
                                     uint64_t* rkey, uint64_t* rec, int64_t cap, Counters* C, hipStream_t s) {
    if (bits == 32)
        return kind == CTG_DATA_U8
                   ? launch_region_scan_h<uint32_t, uint8_t>(A, D, shape, b, e, has_ignore, ignore, rkey, rec, cap, C, s)
                   : launch_region_scan_h<uint32_t, float>(A, D, shape, b, e, has_ignore, ignore, rkey, rec, cap, C, s);
    return kind == CTG_DATA_U8
               ? launch_region_scan_h<uint64_t, uint8_t>(A, D, shape, b, e, has_ignore, ignore, rkey, rec, cap, C, s)
               : launch_region_scan_h<uint64_t, float>(A, D, shape, b, e, has_ignore, ignore, rkey, rec, cap, C, s);
}

// row i of [id, count, sum, min, max] -> key i, record i.  A row without voxels
// (the zero row of an absent label) adds nothing: the folds' identities.
__global__ void k_region_merge(int64_t n, const double* __restrict__ rows, uint64_t* __restrict__ key,
                               uint64_t* __restrict__ rec, unsigned long long* bad) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double* r = rows + i * CTG_REGION_COLS;
    const double two53 = 9007199254740992.0, two64 = 18446744073709551616.0;
    const double id = r[0], cnt = r[1];
    const bool ok = id >= 0.0 && id < two53 && id == rint(id) && cnt >= 0.0 && cnt < two64;
    const uint64_t c = ok ? (uint64_t)cnt : 0ull;
    if (!ok) atomicOr(bad, 1ull);
    region_put(key, rec, (uint64_t)i, ok ? (uint64_t)id : 0ull, c, c ? r[2] : 0.0,
               c ? f2ord((float)r[3]) : 0xFFFFFFFFu, c ? f2ord((float)r[4]) : 0u);
}

// the identity of k_region_runs' folds: n 0, sum 0, min all ones, max 0
__global__ void k_region_init(int64_t N, unsigned long long* __restrict__ cnt, double* __restrict__ sum,
                              uint32_t* __restrict__ mm) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= N) return;
    cnt[j] = 0ull;
    sum[j] = 0.0;
    mm[2 * j] = 0xFFFFFFFFu;
    mm[2 * j + 1] = 0u;
}

// The run-fold policy of the region features (ctg_run_fold.h): sorted position
// i holds the 3-word record slot[i]; n adds in u64, the sum in f64, the ordered
// min / max words fold, onto the label's row of cnt / sum / mm (k_region_init's
// identities before the launch).  A run head writes the label.
struct RegionRuns {
    struct Value {
        uint64_t n;
        double sum;
        uint32_t mn, mx;
    };
    const uint64_t *__restrict__ key, *__restrict__ rec;
    const uint32_t* __restrict__ slot;
    int64_t n_rec;
    uint64_t* __restrict__ nodes;
    unsigned long long* __restrict__ cnt;
    double* __restrict__ sum;
    uint32_t* __restrict__ mm;
    __device__ __forceinline__ void load(Value& v, int64_t i, bool in) const {
        v = Value{0ull, 0.0, 0xFFFFFFFFu, 0u};
        if (in) {
            const uint32_t j = slot[i];
            CTG_IDX(j, n_rec);
            const uint64_t* q = rec + (int64_t)j * REGION_WORDS;
            v.n = q[0];
            v.sum = __longlong_as_double((long long)q[1]);
            v.mn = (uint32_t)q[2];
            v.mx = (uint32_t)(q[2] >> 32);
        }
    }
    __device__ __forceinline__ void combine(Value& v, int o, bool take) const {
        const uint64_t no = shfl_down_u64(v.n, o);
        const double uo = __longlong_as_double((long long)shfl_down_u64((uint64_t)__double_as_longlong(v.sum), o));
        const uint32_t mo = __shfl_down(v.mn, o, WAVE), xo = __shfl_down(v.mx, o, WAVE);
        if (take) {
            v.n += no;
            v.sum += uo;
            v.mn = mo < v.mn ? mo : v.mn;
            v.mx = xo > v.mx ? xo : v.mx;
        }
    }
    __device__ __forceinline__ void apply(uint32_t seg, const Value& v) const {
        atomicAdd(&cnt[seg], (unsigned long long)v.n);
        atomicAdd(&sum[seg], v.sum);
        atomicMin(&mm[2 * (int64_t)seg], v.mn);
        atomicMax(&mm[2 * (int64_t)seg + 1], v.mx);
    }
    __device__ __forceinline__ void name(int64_t i, uint32_t seg, bool head, uint64_t, uint64_t) const {
        if (head) nodes[seg] = key[i];
    }
};

__global__ __launch_bounds__(256) void k_region_runs(int64_t n, const uint64_t* __restrict__ key,
                                                     const uint32_t* __restrict__ slot,
                                                     const uint64_t* __restrict__ scan,
                                                     const uint64_t* __restrict__ rec, int64_t n_rec,
                                                     uint64_t* __restrict__ nodes,
                                                     unsigned long long* __restrict__ cnt, double* __restrict__ sum,
                                                     uint32_t* __restrict__ mm, int64_t N) {
    run_fold(RegionRuns{key, rec, slot, n_rec, nodes, cnt, sum, mm}, n, scan, N);
}

// ordered words -> the f32 they stand for, in place; a label without voxels
// (merge rows of count 0 only) gets zeros
__global__ void k_region_finish(int64_t N, const uint64_t* __restrict__ cnt, uint32_t* __restrict__ mm) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= N) return;
    const bool any = cnt[j] != 0ull;
    for (int c = 0; c < 2; ++c) {
        const float f = any ? ord2f(mm[2 * j + c]) : 0.0f;
        uint32_t b;
        __builtin_memcpy(&b, &f, 4);
        mm[2 * j + c] = b;
    }
}

// One thread per label: its float64 row -- form CTG_REGION_SUMS
// [id, count, sum, min, max], form CTG_REGION_FEATURES [id, count,
// (sum / count) / norm, min / norm, max / norm] -- into rows[j] and, for labels
// in [lb, le), into out[label - lb] (zeroed before the launch).  A label
// without voxels keeps a zero row.
__global__ void k_region_rows(int64_t N, const uint64_t* __restrict__ nodes, const uint64_t* __restrict__ cnt,
                              const double* __restrict__ sum, const float* __restrict__ mm, uint64_t lb, uint64_t le,
                              int form, double norm, double* __restrict__ out, double* __restrict__ rows) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= N) return;
    const uint64_t a = nodes[j], n = cnt[j];
    double r[CTG_REGION_COLS];
    r[0] = (double)a;
    r[1] = (double)n;
    if (form == CTG_REGION_FEATURES) {
        r[2] = n ? (sum[j] / (double)n) / norm : 0.0;
        r[3] = (double)mm[2 * j] / norm;
        r[4] = (double)mm[2 * j + 1] / norm;
    } else {
        r[2] = sum[j];
        r[3] = (double)mm[2 * j];
        r[4] = (double)mm[2 * j + 1];
    }
    if (rows)
        for (int c = 0; c < CTG_REGION_COLS; ++c) rows[j * CTG_REGION_COLS + c] = r[c];
    if (out && n && a >= lb && a < le)
        for (int c = 0; c < CTG_REGION_COLS; ++c) out[(a - lb) * CTG_REGION_COLS + c] = r[c];
}

// n (key, record) pairs -> r's nodes and region moments; keys compare in their
// low end_bit bits
static hipError_t region_reduce(Workspace& w, const uint64_t* key, const uint64_t* rec, int64_t n, unsigned end_bit,
                                hipStream_t s, ctg_result* r) {
    return fold_records<true, uint32_t>(
        w, key, nullptr, n, end_bit, s,
        [&](const uint64_t* ks, const uint32_t* is, const uint64_t* scan, int64_t N, int64_t) {
            DevBuf<uint64_t> nodes((size_t)N * 8), cnt((size_t)N * 8);
            DevBuf<double> sum((size_t)N * 8);
            DevBuf<float> mm((size_t)N * 8);
            if (!nodes || !cnt || !sum || !mm) return hipErrorOutOfMemory;
            hipLaunchKernelGGL(k_region_init, grid_for(N), dim3(256), 0, s, N, (unsigned long long*)cnt.p, sum.p,
                               (uint32_t*)mm.p);
            CTG_TRY(hipGetLastError());
            hipLaunchKernelGGL(k_region_runs, grid_for(n), dim3(256), 0, s, n, ks, is, scan, rec, n, nodes.p,
                               (unsigned long long*)cnt.p, sum.p, (uint32_t*)mm.p, N);
            CTG_TRY(hipGetLastError());
            hipLaunchKernelGGL(k_region_finish, grid_for(N), dim3(256), 0, s, N, cnt.p, (uint32_t*)mm.p);
            CTG_TRY(hipGetLastError());
            swap_in(r->nodes, nodes);
            swap_in(r->reg_count, cnt);
            swap_in(r->reg_sum, sum);
            swap_in(r->reg_minmax, mm);
            r->n_nodes = N;
            return hipSuccess;
        });
}

hipError_t region_tables(Workspace& w, const void* A, int bits, const void* D, int kind, const int64_t* shape,
                         const int64_t* b, const int64_t* e, int has_ignore, uint64_t ignore, hipStream_t s,
                         ctg_result* r, unsigned* overflow) {
    return scan_tables<uint64_t>(
        w, (e[0] - b[0]) * (e[1] - b[1]) * (e[2] - b[2]), s, REGION_WORDS,
        [&](uint64_t* rkey, uint64_t* rec, int64_t cap) {
            return launch_region_scan(A, bits, D, kind, shape, b, e, has_ignore, ignore, rkey, rec, cap, w.counters,
                                      s);
        },
        [&](const uint64_t* rkey, const uint64_t* rec, int64_t m) { return region_reduce(w, rkey, rec, m, 32u, s, r); },
        true, r, overflow);
}

hipError_t region_merge(Workspace& w, const double* rows, int64_t n, hipStream_t s, ctg_result* r, int* bad) {
    return merge_rows(
        w, rows, n, REGION_WORDS, k_region_merge,
        [&](const uint64_t* key, const uint64_t* rec) { return region_reduce(w, key, rec, n, 53u, s, r); }, s, r, bad);
}

hipError_t launch_region_rows(const ctg_result* r, uint64_t lb, uint64_t le, int form, double norm, double* out,
                              double* rows, hipStream_t s) {
    if (r->n_nodes == 0) return hipSuccess;
    hipLaunchKernelGGL(k_region_rows, grid_for(r->n_nodes), dim3(256), 0, s, r->n_nodes, r->nodes, r->reg_count,
                       r->reg_sum, r->reg_minmax, lb, le, form, norm, out, rows);
    return hipGetLastError();
}

CTG_BOUNDS_TAKE(region)

}  // namespace ctg
