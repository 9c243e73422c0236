// Internal definitions shared by the ctg (cluster-tools graph) HIP sources.
// gfx950 / CDNA4 only.  See DESIGN.md for the data layout and the pipeline.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstddef>
#include <memory>
#include <atomic>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "../../include/ctg.h"
#include "ctg_buffers.h"
#include "ctg_plan.h"

namespace ctg {

// ---------------------------------------------------------------------------
// CTG_DIAG builds: bounds checks on the indices into call-sized workspace
// buffers (records, sorted positions, run tables, permutations, bitmaps).
// The buffers are sized by the largest call so far, so a read past the
// current call's count stays inside the allocation and returns stale data
// instead of faulting (round 5's k_mark_nodes_win bug).  CTG_IDX(i, n) notes
// the first i >= n of a source file in that file's device word block --
// (line, index, bound), no trap, the access itself unchanged -- and
// ctg_diag_bounds() hands it to the host.  Product builds compile it out.
// ---------------------------------------------------------------------------
#ifdef CTG_DIAG
static __device__ unsigned long long ctg_oob[4];   // per translation unit (static): line, index, bound
__device__ __forceinline__ void oob_note(unsigned long long* d, uint64_t i, uint64_t n, int line) {
    if (i >= n && atomicCAS(d, 0ull, (unsigned long long)line) == 0ull) {
        d[1] = i;
        d[2] = n;
    }
}
#define CTG_IDX(i, n) ::ctg::oob_note(::ctg::ctg_oob, (uint64_t)(i), (uint64_t)(n), __LINE__)
// the host side of one file's block: copy it out (3 words) and clear it
#define CTG_BOUNDS_TAKE(tag)                                                      \
    hipError_t bounds_take_##tag(unsigned long long* h) {                       \
        hipError_t e_ = hipMemcpyFromSymbol(h, HIP_SYMBOL(ctg_oob), 24);          \
        if (e_ != hipSuccess || h[0] == 0) return e_;                             \
        const unsigned long long z_[4] = {0, 0, 0, 0};                            \
        return hipMemcpyToSymbol(HIP_SYMBOL(ctg_oob), z_, 32);                    \
    }
#else
#define CTG_IDX(i, n) ((void)0)
#define CTG_BOUNDS_TAKE(tag)
#endif

// ---------------------------------------------------------------------------
// fixed geometry of the face-scan tiles and the LDS edge table
// ---------------------------------------------------------------------------
constexpr int WAVE = 64;
#ifndef CTG_SCAN_THREADS
#define CTG_SCAN_THREADS 512
#endif
constexpr int SCAN_THREADS = CTG_SCAN_THREADS;   // 8 waves per workgroup (1024: 16 waves, one per CU)
constexpr int TILE_Y = 8;              // (TILE_X, one wave row: ctg_plan.h)
// LDS edge-table entries: a multiple of 4 (4-slot buckets), at most one per
// thread in a flush; a power of two or not (the home bucket is a multiply-high)
#ifndef CTG_TABLE_CAP
#define CTG_TABLE_CAP SCAN_THREADS
#endif
constexpr int TABLE_CAP = CTG_TABLE_CAP;
static_assert(TABLE_CAP % 4 == 0 && TABLE_CAP <= SCAN_THREADS, "table capacity");
constexpr int NBINS = 40;              // vigra UserRangeHistogram<40> (nifty default)
constexpr int NSLOTS = NBINS + 2;      // left outliers, 40 bins, right outliers
constexpr int HWORDS = 21;             // 42 u16 slots packed in 21 u32 words
constexpr int NREC_WORDS = 24;         // narrow record: 21 hist words + cnt + min + max
// narrow records live in 128-byte bodies (one cache line each, so the
// reduction's gather touches exactly one line per record):
//   words 0..3 (sum f64, sum of squares f64), 4..27 the NREC_WORDS, 28..31 zero
constexpr int NREC_STRIDE = 32;
constexpr int NREC_OFF = 4;
constexpr int NREC_PIV = 28;           // word 28: the pivot (f32 bits) the two sums are taken about
constexpr int WREC_WORDS = 48;         // wide record: 42 u32 slots + cnt + min + max + pivot + pad
constexpr int WREC_PIV = 45;
// Statistics are kept as shifted sums about a per-entry pivot p (the entry's
// first sample): S1 = sum(x - p), S2 = sum((x - p)^2).  The variance
// (S2 - S1^2/n)/n then cancels only the spread of the samples, not their
// magnitude, and records / partial tables combine by re-pivoting
// (Moments::add, ctg_reduce.hip).  A pivot word of 0 is the plain power sums.
constexpr uint32_t PIV_EMPTY = 0xFFFFFFFFu;   // table entry without a pivot yet (a NaN no sample carries)
constexpr uint32_t ADJ_FLAG = 0x80000000u;  // record/edge came from a nearest-neighbour face
constexpr uint64_t EMPTY_KEY = ~0ull;
constexpr int N_FEATURES = 10;
// The label-table calls (overlaps, morphology, region features) take fewer
// voxels, rows and records than this in one call: a record per voxel at most,
// and the run fold numbers records and rows in 32 bits, all ones being no row
// (ctg_run_fold.h)
constexpr int64_t RECORD_LIMIT = 0xFFFFFFFFll;

// order-preserving float <-> u32 mapping for LDS/global atomicMin/Max
__host__ __device__ inline uint32_t f2ord(float f) {
    uint32_t b;
    __builtin_memcpy(&b, &f, 4);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__host__ __device__ inline float ord2f(uint32_t o) {
    uint32_t b = (o & 0x80000000u) ? (o & 0x7FFFFFFFu) : ~o;
    float f;
    __builtin_memcpy(&f, &b, 4);
    return f;
}
constexpr uint32_t ORD_POS_INF = 0xFF800000u;  // f2ord(+inf)
constexpr uint32_t ORD_NEG_INF = 0x007FFFFFu;  // f2ord(-inf)

// vigra RangeHistogramBase::update binning -> slot in [0, NSLOTS)
__host__ __device__ inline int hist_slot(double x, double scale, double offset) {
    double m = scale * (x - offset);
    if (m == (double)NBINS) return NBINS;          // index nbins-1 -> slot nbins
    if (!(m < (double)NBINS)) return (m != m) ? 0 : NBINS + 1;  // right outlier (NaN -> left)
    if (m <= -1.0) return 0;                          // (int)m < 0 -> left outlier
    return (int)m + 1;                                // trunc toward zero, as (int)m
}

__host__ __device__ inline uint32_t hash_key(uint64_t k) {
    k ^= k >> 33;
    k *= 0xff51afd7ed558ccdull;
    k ^= k >> 33;
    return (uint32_t)k;
}

// 64-bit wave shuffles as two 32-bit ones (device code only)
#ifdef __HIPCC__
__device__ __forceinline__ uint64_t shfl_up_u64(uint64_t v) {
    const uint32_t lo = __shfl_up((uint32_t)v, 1, WAVE), hi = __shfl_up((uint32_t)(v >> 32), 1, WAVE);
    return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ uint64_t shfl_down_u64(uint64_t v, int o) {
    const uint32_t lo = __shfl_down((uint32_t)v, o, WAVE), hi = __shfl_down((uint32_t)(v >> 32), o, WAVE);
    return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ uint64_t bcast0_u64(uint64_t v) {
    const uint32_t lo = __shfl((uint32_t)v, 0, WAVE), hi = __shfl((uint32_t)(v >> 32), 0, WAVE);
    return ((uint64_t)hi << 32) | lo;
}
#endif

// Blocked Bloom filter of RAG edge keys (the long-range affinity prefilter),
// blocked by OWNER label: an edge (u, v) is stored twice, as u -> v in the
// 64-B block of u and as v -> u in the block of v; a probe from a voxel of
// label a for partner b tests a -> b: 4 bits of ONE 64-bit word of a's block.
// A wave's probes then touch one cache line per distinct own label (a few per
// row) instead of one per distinct pair, and the line of a label stays hot in
// L2 over every channel and plane that label's cell spans.
__host__ __device__ inline uint64_t bloom_hash(uint64_t k) {
    k ^= k >> 33;
    k *= 0xff51afd7ed558ccdull;
    k ^= k >> 29;
    k *= 0xc4ceb9fe1a85ec53ull;
    return k ^ (k >> 32);
}
// h: bloom_hash((owner << 32) | other)
__host__ __device__ inline uint64_t bloom_bits(uint64_t h) {
    return (1ull << (h & 63)) | (1ull << ((h >> 6) & 63)) | (1ull << ((h >> 12) & 63)) | (1ull << ((h >> 18) & 63));
}
// word of the owner's block (block_mask = blocks - 1, 8 words per block)
__host__ __device__ inline uint32_t bloom_block(uint32_t owner, uint32_t block_mask) {
    return ((uint32_t)(bloom_hash(owner) >> 24) & block_mask) * 8u;
}
__host__ __device__ inline uint32_t bloom_word(uint32_t block, uint64_t h) { return block + ((uint32_t)(h >> 40) & 7u); }

// ---------------------------------------------------------------------------
// records: the face scan flushes one record per (tile, edge), into the NREG
// regions of the record buffer (NREG, RegionPrefix: ctg_plan.h)
// ---------------------------------------------------------------------------
struct RecordBuf {
    uint64_t* key = nullptr;      // (u << 32) | v
    double2* sums = nullptr;      // wide records: (sum, sum of squares); compact: unused (in the body)
    uint32_t* hist = nullptr;     // narrow: NREC_STRIDE-word bodies; wide: WREC_WORDS per record
    int64_t cap = 0;
    int64_t rcap = 0;             // slots per region (cap / NREG)
};

// (BlockGeom, one array of a batched call: ctg_plan.h)
struct ScanParams {
    const void* labels;
    const void* data;          // boundary (Z,Y,X) or affinities (C,Z,Y,X); may be null
    int label_bits;            // 64 or 32
    int data_kind;             // CTG_DATA_*
    int n_channels;            // 0 -> boundary map
    int offsets[CTG_MAX_CHANNELS][3];
    int64_t shape[3];
    int64_t own_begin[3];
    int64_t own_end[3];
    double scale, offset;      // histogram mapping
    double u8_scale;           // uint8 -> float factor (1/255)
    int tile_z;                // z-planes per workgroup
    int tile_z_narrow;         // z-planes per workgroup of the narrow-tile launch (0: tile_z)
    int check_planes;          // planes between flush decisions
    int fast40;                // histogram range [0,1) x 40 bins: exact f32 binning
    int ablate;                // diagnostic: 8 loads only, 32 staging without fold
    // long-range affinity channels: samples whose (u,v) fails this blocked
    // Bloom filter of the RAG edge keys ((u << 32) | v) are dropped in the scan
    // (bloom_mask = blocks - 1, 8 words a block); the reduce drops the false positives, keeping
    // only keys that nearest-neighbour samples (MARK_ONE_ADJ) flagged
    const unsigned long long* bloom;
    uint32_t bloom_mask;
    int64_t ntiles[3];         // tiles along x, y, z (set by the launcher)
    int xcd_remap;             // 1: XCD-contiguous tile order (see k_face_scan)
    // affinities: the three nearest-neighbour channels are present, so every
    // RAG edge gets a sample of one of them and the scan pushes no adjacency
    // markers (with a Bloom filter those samples carry the flag instead)
    int skip_adj_marks;
    // the three nearest-neighbour channels alone (whole array, no long-range
    // channel, adjacency proven by every sample): scanned as faces, like a
    // boundary map, the sample of face (p - e_a, p) being aff[nn_ch[a], p]
    int nn3;
    int nn_ch[3];              // channel of the offset -e_a, a = z, y, x
    // long-range calls (Bloom-filtered): the three nearest-neighbour channels
    // as faces (their samples are the adjacency proofs), the other channels
    // loop_ch[0 .. n_loop) in the channel loop
    int nn_mix;
    int n_loop;
    int loop_ch[CTG_MAX_CHANNELS];
    uint32_t lr_mask;          // bit c: channel c is long-range (|offset|_1 > 1)
    int narrow_rows;           // boundary maps: 1 2-row waves (fragmented volumes, see ctg_scan.hip),
                               // 2 decided on the device from density[] (no host round trip)
    const uint32_t* density;   // sampled x-face changes / pairs (k_density), for narrow_rows == 2
    // batched blocks (ctg_rag_blocks): workgroup w scans a tile of array b with
    // tile_prefix[b] <= w < tile_prefix[b+1]; keys carry b in the bits of u
    // from tag_shift up, so labels must stay below 2^tag_shift (else the label
    // overflow flag is raised and the host relabels densely)
    const BlockGeom* blocks;
    const uint32_t* tile_prefix;
    int n_blocks;
    int64_t batch_tiles;       // tile_prefix[n_blocks]: the launch's workgroups
    int tag_shift;             // 32: no tag (n_blocks == 1)
    uint32_t label_hi_mask;    // bits a narrowed label must not have (overflow flag)
    unsigned long long* wg_times;   // CTG_DIAG (CTG_WG_TIMES): per workgroup (start, end) s_memrealtime, or null
    // tail tiles (whole arrays): workgroups [0, main_tiles) take tile_z-deep
    // tiles of planes [0, tail_z0), the rest tile_z_tail-deep tiles of
    // [tail_z0, Z) -- dispatched last on every XCD, so the launch's drain waits
    // for short tiles (set by the launcher; main_tiles = all: none)
    int tail_tiles;            // host switch (CTG_TAIL_TILES)
    int64_t main_tiles;
    int tail_z0, tile_z_tail;
    // host switch (CTG_SCAN_INTERIOR, whole arrays): the face kernels' interior
    // waves (scan_wave_interior, ctg_plan.h) walk their planes without ownership
    // masks; 0: every wave takes the general plane loop
    int interior;
};

struct Counters {               // device-side counters, zeroed per call
    unsigned long long n_records;
    unsigned long long n_direct;     // faces emitted past a full LDS table
    unsigned long long label_overflow;  // labels >= 2^32 seen by the 32-bit key path
    unsigned long long max_v;        // largest label in any key
    // largest ~u (32 bits) of any key: the smallest u is ~max_nu (0: no key).  It is a lower bound the back half
    // relies on: min_u <= u of every sorted key -- the group sort's buckets start at min_u << nb, and the node
    // bitmap of collect_nodes starts at word min_u >> 5, so a key whose u came out below min_u (a wrong bucket
    // base, say) would index in front of the bitmap.  The host keeps the bound (plan_group_sort, tests/test_plan.py);
    // the device does not check it.
    unsigned long long max_nu;
    unsigned long long pad[8];      // diagnostics (ablation checks, s_memtime stamps)
    unsigned long long rcount[NREG];  // records reserved per region (may exceed rcap: overflow)
};

// record slot of sorted position r: a u32 index array, or the low ib bits of
// the packed sort keys (keys-only record sort, no unpack pass)
struct Perm {
    const uint32_t* p32;
    const uint64_t* p64;
    int ib;
    __device__ __forceinline__ uint32_t operator()(uint32_t r) const {
        return p64 ? (uint32_t)(p64[r] & ((1ull << ib) - 1ull)) : p32[r];
    }
};

// CTG_DEFER_STATS: what a result needs to rebuild an edge's mergeable
// statistics from its records -- run e of the sorted records is slots
// perm(offs[e] .. offs[e] + runs[e]) of the narrow record bodies `hist` --
// valid while the workspace's generation is still `gen`
struct DeferredStats {
    int on = 0;
    const uint32_t* offs = nullptr;
    const uint32_t* runs = nullptr;
    Perm perm{nullptr, nullptr, 0};
    const uint32_t* hist = nullptr;
    uint64_t gen = 0;
    int64_t n_runs = 0, n_rec = 0, rec_cap = 0;   // bounds of offs / runs, sorted positions, slots (CTG_DIAG checks)
};

struct ReduceOut {
    uint64_t* edges;      // 2E
    double* feats;        // 10E or null
    uint32_t* keep;       // E or null
    uint32_t* wstats;     // WREC_WORDS*E or null
    double2* wsums;       // E or null
    uint32_t* count_out;  // null, or receives the edge count (no compaction follows)
    int ablate;           // diagnostics (CTG_REDUCE_ABLATE): 1 no quantiles, 2 no record loads, 4 no feature stores
    int64_t n_rec;        // sorted record positions of the call (CTG_DIAG bounds checks)
};

constexpr int BK_SMALL_WORDS = 5 * 4096 + 16;   // bucket sort: counts, offsets, cursors, run heads
constexpr int GS_SMALL_WORDS = 5 * 65536 + 16;   // group sort: counts, offsets, cursors, misc, run counts / offsets (5M + 9)

// The scalar words of Workspace::small (device) and, at the same index,
// Workspace::small_host (pinned): who owns which.
enum SmallSlot : int {
    SLOT_RUNS = 0,         // reduce_records: runs, kept edges, nodes -- read back together
    SLOT_EDGES = 1,
    SLOT_NODES = 2,        // (also the count of the unique-label entry points)
    SLOT_BAD_ID = 3,       // ctg_merge_feature_rows: an id outside the block
    SLOT_DENSITY = 4,      // 2 words: the density probe's changes / pairs
    SLOT_GROUP_SORT = 16,  // host word of the group sort
    SLOT_MERGE = 20,       // 2 words: MergeCounts (ctg_mgpu.hip)
    SLOT_HEAVY = 40,       // edges listed for the wide-histogram kernel
    SMALL_WORDS = 64
};
struct MergeCounts {       // the multi-GPU merge's pair at SLOT_MERGE, cleared as one
    uint32_t keys;         // distinct received keys
    uint32_t rows;         // rows of the shard
};
// each slot ends where the next begins or before it, the last one below SMALL_WORDS: disjoint and in range
static_assert(SLOT_RUNS >= 0 && SLOT_RUNS + 1 <= SLOT_EDGES && SLOT_EDGES + 1 <= SLOT_NODES &&
                  SLOT_NODES + 1 <= SLOT_BAD_ID && SLOT_BAD_ID + 1 <= SLOT_DENSITY &&
                  SLOT_DENSITY + 2 <= SLOT_GROUP_SORT && SLOT_GROUP_SORT + 1 <= SLOT_MERGE &&
                  SLOT_MERGE + (int)(sizeof(MergeCounts) / 4) <= SLOT_HEAVY && SLOT_HEAVY + 1 <= SMALL_WORDS,
              "the scalar slots overlap or pass SMALL_WORDS");

struct Workspace {
    std::atomic<bool> ready{false};   // (read without the device lock by the accessors' copy) ws_init made every fixed member (counters .. mgpu_spl, ev); set last
    int device = -1;
    // bumped by every call that overwrites the records or the sort / run
    // buffers (a CTG_DEFER_STATS handle compares it)
    uint64_t gen = 1;
    RecordBuf rec;
    SortScratch sort;   // sort / reduce scratch
    GrowBuf temp;       // rocPRIM's temporary storage (with_temp)
    Counters* counters = nullptr;        // device
    Counters* counters_host = nullptr;   // pinned
    unsigned int* small = nullptr;       // device scalars, SMALL_WORDS of them (SmallSlot)
    unsigned int* small_host = nullptr;
    uint32_t* bsort = nullptr;           // device: bucket-sort scratch, BK_SMALL_WORDS u32 (ctg_sort.hip)
    uint32_t* gsort = nullptr;           // device: group-sort scratch, GS_SMALL_WORDS u32 (ctg_sort.hip)
    uint64_t* mgpu_spl = nullptr;        // device: the exchange's splitters, CTG_MGPU_MAX_WORLD u64
    hipEvent_t mgpu_spl_ev = nullptr;    // recorded after the last split read mgpu_spl (a split on another
                                         // stream waits for it before overwriting the splitters)
    GrowBuf stage[2];   // host->device staging of volumes
    // the result accessors' copies (ctg_result_copy_*): a non-blocking stream
    // of the library's own, so they neither run on the null stream nor wait for it
    hipStream_t copy_stream = nullptr;
    // timing
    hipEvent_t ev[7] = {};   // 0..6: the phase marks of a call
    double last_ms[8] = {0};   // scan, pack, sort, segment, reduce, nodes, total, narrow (always 0: no such pass)
    int64_t last_records = 0, last_direct = 0;
    SortReport last_sort;   // the last record sort (ctg_last_sort); host values, a few stores per call
    ScanReport last_scan;   // the last whole-array face scan (ctg_last_scan); host values
    int profiling = 0;
};

// ---------------------------------------------------------------------------
// workspace, allocator and error state (ctg_workspace.hip, ctg_api.hip)
// ---------------------------------------------------------------------------
Workspace& ws(int device);
hipError_t ws_init(Workspace& w);
int current_device();
void set_error(const std::string& msg);
void free_records(Workspace& w);
hipError_t ensure_records(Workspace& w, int64_t need, int wide);

// One workspace per device: calls that use it are serialised per device, so
// job threads may call the library concurrently (ctypes drops the GIL) --
// their N5 decode overlaps, their GPU work queues.  Recursive: the dense
// relabel and adjacency paths re-enter the C ABI.
std::recursive_mutex& device_mutex(int device);
struct DevLock {
    std::lock_guard<std::recursive_mutex> g;
    DevLock() : g(device_mutex(current_device())) {}
};

// rocPRIM call with a growable temp buffer: size query (null temp), grow, run.
// call: (void* temp, size_t& bytes) -> hipError_t
template <class F>
hipError_t with_temp(GrowBuf& temp, F&& call) {
    size_t bytes = 0;
    hipError_t e = call(nullptr, bytes);
    if (e != hipSuccess) return e;
    if (!temp.reserve(bytes + 256)) return hipErrorOutOfMemory;
    bytes = temp.bytes;
    return call(temp.p, bytes);
}

struct Ev {   // phase marks of a profiled call
    Workspace& w;
    hipStream_t s;
    void mark(int i) {
        if (w.profiling) hipEventRecord(w.ev[i], s);
    }
};

// ---------------------------------------------------------------------------
// launchers (one declaration each; the definitions name their file)
// ---------------------------------------------------------------------------
// ctg_scan.hip
// rep: null, or receives the waves of the launch(es) and how many are interior
hipError_t launch_face_scan(const ScanParams& P, const RecordBuf& R, Counters* C, hipStream_t s,
                            ScanReport* rep = nullptr);
int64_t scan_max_x();   // widest array (along x) the face scan takes
int scan_tile_rows();
int scan_tile_rows_narrow();
hipError_t launch_density(const void* L, int label_bits, const int64_t* shape, int n_rows, uint32_t* out,
                          hipStream_t s);
hipError_t launch_unique_tiles(const uint64_t* L, const int64_t* shape, const int64_t* b, const int64_t* e,
                               uint64_t* out, unsigned long long* count, int64_t cap, hipStream_t s);
hipError_t launch_unique_blocks(const void* L, int label_bits, const BlockGeom* blocks, const uint32_t* tile_prefix,
                                int n_blocks, int64_t n_tiles, uint64_t* out, unsigned long long* count, int64_t cap,
                                hipStream_t s);
int unique_tile_y();
// ctg_sort.hip
hipError_t bucket_sort_keys(const uint64_t* keys, uint64_t* tmp, uint64_t* out, int64_t n, int lo_bit, int hi_bit,
                            uint64_t kmin, uint64_t kmax, uint32_t* small, GrowBuf& temp, uint32_t* nbk_out,
                            hipStream_t s);
hipError_t bucket_runs(const uint64_t* sorted, int64_t n, int lo_bit, uint32_t nbk, uint32_t* small, uint64_t* uniq,
                       uint32_t* runs, uint32_t* roffs, uint32_t* dE, hipStream_t s);
hipError_t bucket_sort_pairs(const uint64_t* keys, const uint32_t* vals, uint64_t* ktmp, uint32_t* vtmp,
                             uint64_t* kout, uint32_t* vout, int64_t n, int hi_bit, uint32_t* small, GrowBuf& temp,
                             uint32_t* nbk_out, hipStream_t s);
hipError_t group_sort_runs(const uint64_t* key, int64_t rcap, const RegionPrefix& pre, int64_t n, int nb, int ub,
                           int ib, uint64_t min_label, uint64_t max_label, uint32_t* small, uint32_t* host_word,
                           uint64_t* items, uint32_t* perm, uint64_t* uniq, uint32_t* runs, uint32_t* roffs,
                           uint32_t* dE, bool* done, SortReport* rep, hipStream_t s);
// ctg_reduce.hip
hipError_t launch_pack_keys(int64_t n, const uint64_t* key, int nb, uint64_t* sk, uint32_t* idx, hipStream_t s);
hipError_t launch_pack_regions(const uint64_t* key, int64_t rcap, const RegionPrefix& pre, int nb, int ib, uint64_t* sk,
                               uint32_t* idx, hipStream_t s);
hipError_t launch_pack_pairs(int64_t n, const uint64_t* uv, int nb, uint64_t* sk, uint32_t* idx, hipStream_t s);
hipError_t launch_max_pairs(int64_t n, const uint64_t* uv, unsigned long long* out, hipStream_t s);
hipError_t launch_reduce(int64_t E, const uint32_t* dE, const uint64_t* uniq, const uint32_t* runs,
                         const uint32_t* offs, const uint32_t* perm32, const uint64_t* perm64, int ib,
                         const RecordBuf& R, int wide, int stats, int nb, uint64_t umask, int need_adj,
                         int ignore_label, double scale, double offset, const ReduceOut& O, hipStream_t s,
                         uint32_t* heavy = nullptr, uint32_t* n_heavy = nullptr);
hipError_t launch_block_bounds(int64_t n, const uint64_t* col, int stride, int n_blocks, int shift, int64_t* bounds,
                               hipStream_t s);
hipError_t launch_clear_bits(int64_t n, uint64_t* col, int stride, uint64_t mask, hipStream_t s);
hipError_t launch_compact(int64_t E, const uint32_t* dE, const uint32_t* keep, const uint32_t* pos,
                          const ReduceOut& in, const ReduceOut& out, uint32_t* dkept, hipStream_t s);
hipError_t launch_endpoints(int64_t E, const uint64_t* uniq, int nb, uint32_t* out, hipStream_t s);
hipError_t launch_u32_to_u64(int64_t n, const uint32_t* in, uint64_t* out, hipStream_t s);
hipError_t launch_mark_nodes(int64_t E, const uint32_t* dE, const uint64_t* uniq, int nb, uint32_t* bits,
                             int64_t W, uint32_t wbase, hipStream_t s);
hipError_t launch_bits_to_nodes(int64_t W, const uint32_t* bits, const uint32_t* off, uint64_t* nodes, uint32_t* dN,
                                int64_t cap, uint32_t wbase, hipStream_t s);
hipError_t launch_build_bloom(const uint64_t* edges, int64_t E, unsigned long long* words, uint32_t mask,
                              hipStream_t s);
hipError_t launch_find_edges(const uint64_t* ge, int64_t n, const uint64_t* q, int64_t m, int64_t* out,
                             hipStream_t s);
hipError_t launch_remap_dense(const uint64_t* L, int64_t V, const uint64_t* U, int64_t n, uint32_t* out,
                              hipStream_t s);
hipError_t launch_gather_labels(const uint64_t* U, uint64_t* x, int64_t n, hipStream_t s);
hipError_t launch_remap_dense64(const uint64_t* L, int64_t V, const uint64_t* U, int64_t n, uint64_t* out,
                                hipStream_t s);
hipError_t launch_row_keys(int64_t n, const uint64_t* ids, uint64_t begin, uint64_t end, uint32_t* key,
                           uint32_t* idx, uint32_t* bad, hipStream_t s);
hipError_t launch_merge_feature_rows(int64_t n, const uint32_t* key, const uint32_t* idx, const double* rows,
                                     double* out, hipStream_t s);
// ctg_synth.hip
hipError_t launch_synth(uint64_t* labels, float* boundary, const int64_t* shape, int64_t z_offset,
                        const int64_t* gshape, int cell, uint64_t seed, uint64_t label_offset, double noise_amp,
                        hipStream_t s);
hipError_t launch_synth_aff(const float* b, float* out, const int64_t* shape, int n_channels, const int32_t* off,
                            hipStream_t s);
#ifdef CTG_DIAG   // the per-file bounds-check blocks (CTG_BOUNDS_TAKE above)
hipError_t bounds_take_api(unsigned long long* h);
hipError_t bounds_take_reduce(unsigned long long* h);
hipError_t bounds_take_sort(unsigned long long* h);
hipError_t bounds_take_mgpu(unsigned long long* h);
hipError_t bounds_take_scan(unsigned long long* h);
hipError_t bounds_take_overlap(unsigned long long* h);
hipError_t bounds_take_morph(unsigned long long* h);
hipError_t bounds_take_region(unsigned long long* h);
#endif

}  // namespace ctg

// result handle (opaque in the C ABI)
struct ctg_result {
    int device = -1;
    // batched blocks (ctg_rag_blocks): rows [edge_off[b], edge_off[b+1]) of the
    // edge / feature tables and [node_off[b], node_off[b+1]) of the node table
    // belong to block b
    std::vector<int64_t> edge_off, node_off;
    int64_t n_edges = 0;
    int64_t n_nodes = 0;
    uint64_t* edges = nullptr;      // device (E,2)
    uint64_t* nodes = nullptr;      // device (N,)
    double* features = nullptr;     // device (E,10) or null
    uint32_t* stats = nullptr;      // device wide records (E, WREC_WORDS) or null
    double2* stat_sums = nullptr;   // device (E,) (sum, sumsq) or null
    // label-overlap tables (ctg_label_overlaps, ctg_merge_overlaps): edges holds
    // the sorted (a, b) pairs, nodes the distinct a
    uint64_t* counts = nullptr;     // device (E,) voxels of each pair, or null
    int64_t* row_off = nullptr;     // device (N+1,) rows [row_off[j], row_off[j+1]) belong to nodes[j], or null
    // segment morphology (ctg_morphology, ctg_merge_morphology): nodes holds the
    // distinct labels, ascending
    uint64_t* moments = nullptr;    // device (N, MORPH_WORDS): n, sum z y x, min z y x, max z y x (inclusive), or null
    // region features (ctg_region_features, ctg_merge_region_features): nodes
    // holds the distinct counted labels, ascending; all three or none
    uint64_t* reg_count = nullptr;  // device (N,) voxels, or null
    double* reg_sum = nullptr;      // device (N,) sum of the samples
    float* reg_minmax = nullptr;    // device (N,2) smallest and largest sample
    int64_t n_records = 0;
    int64_t n_direct = 0;
    // affinity partial table (CTG_NO_ADJ_FILTER): a key is an edge only where
    // some record carries the ADJ bit (decided after a merge)
    int partial_adj = 0;
    // CTG_DEFER_STATS: statistics rows rebuilt from the records on demand
    ctg::DeferredStats defer;
    // allocations this handle frees instead of the five pointers above, which
    // then point into them (a multi-GPU shard that is a range of its rank's
    // local table: ctg_mgpu_merge)
    std::vector<void*> owned;
};

// assignment handle (opaque in the C ABI): a dense table or the hash table of
// ctg_take.h, in device memory the handle owns
struct ctg_assignment {
    int device = -1;
    int kind = CTG_ASSIGN_DENSE;
    int64_t n = 0;               // dense: entries; sparse: pairs
    uint64_t max_value = 0;      // the largest value (0: no entry)
    uint64_t* table = nullptr;   // device
    uint64_t size = 0;           // dense: n; sparse: slots
};

namespace ctg {

// a result under construction: freed (ctg_free) unless release()d to the caller
struct ResultFree {
    void operator()(ctg_result* r) const { ctg_free(r); }
};
using ResultPtr = std::unique_ptr<ctg_result, ResultFree>;
ResultPtr new_result(int device);     // the one place a handle is made
ResultPtr empty_result(int device);   // no edges, no nodes: the 16- and 8-byte placeholders

// ---------------------------------------------------------------------------
// shared back half (ctg_records.hip): records (n, with keys (u<<32|v) or
// (u,v) pairs) -> result
// ---------------------------------------------------------------------------
struct ReduceJob {
    int64_t n;                 // records
    const uint64_t* keys;      // packed (u<<32)|v, or null if pairs given
    const uint64_t* pairs;     // (u,v) pairs
    RecordBuf R;
    int wide, stats, need_adj, ignore_label, keep_stats;
    uint64_t max_v;
    uint64_t min_u = 0;        // smallest u of any key (scan records; 0: unknown)
    double scale, offset;
    const uint64_t* single_label_ptr;  // device pointer to a label to use if E == 0
    const RegionPrefix* regions;       // keys in NREG regions of R (scan records), or null: dense
    int ub = 0;                        // bits of the key's u field (0: = bits of the largest label)
    uint64_t umask = ~0ull;            // label bits of u (batched blocks: below the block tag)
    int skip_nodes = 0;                // batched blocks: nodes come from the per-block unique pass
    int defer_stats = 0;               // CTG_DEFER_STATS (with keep_stats)
};
hipError_t reduce_records(Workspace& w, const ReduceJob& J, hipStream_t s, ctg_result* res);

// ---------------------------------------------------------------------------
// label overlaps (ctg_overlap.hip).  Call-sized pool buffers only: the
// workspace's records, sort scratch and generation stay as they are.
// ---------------------------------------------------------------------------
// The table of the box [b, e) of two volumes (abits / bbits: 32 or 64) into r
// (edges, counts, nodes, row_off; nothing where every voxel is ignored).
// *overflow: bit 0 a label, bit 1 a value >= 2^32 was met -- r is untouched and
// the caller relabels that side densely.
hipError_t overlap_tables(Workspace& w, const void* A, int abits, const void* B, int bbits, const int64_t* shape,
                          const int64_t* b, const int64_t* e, int with_ignore, uint64_t ignore, hipStream_t s,
                          ctg_result* r, unsigned* overflow);
// n > 0 (key = a << 32 | b, count) records -> r: equal keys add their counts
hipError_t overlap_reduce(Workspace& w, const uint64_t* key, const uint64_t* cnt, int64_t n, hipStream_t s,
                          ctg_result* r);
// The front half of a record reduce, shared with the morphology (ValueT: u32
// or u64): n > 0 (key, value) pairs sorted by the keys' low end_bit bits into
// (ks, vs), the runs numbered -- scan[i] counts the distinct keys (low word)
// and distinct high key halves (high word) up to and including sorted position
// i, *last = scan[n - 1], read back after a stream synchronise.
template <typename ValueT>
hipError_t sort_and_number(Workspace& w, const uint64_t* key, const ValueT* val, int64_t n, unsigned end_bit,
                           hipStream_t s, uint64_t* ks, ValueT* vs, uint64_t* scan, uint64_t* last);
hipError_t launch_overlap_pack(int64_t n, const uint64_t* pairs, uint64_t* key, hipStream_t s);
hipError_t launch_overlap_map_back(int64_t E, uint64_t* pairs, const uint64_t* Ua, int64_t na, const uint64_t* Ub,
                                   int64_t nb, hipStream_t s);
hipError_t launch_overlap_find(const uint64_t* U, int64_t n, uint64_t x, uint32_t* out, hipStream_t s);
hipError_t launch_overlap_argmax(const ctg_result* r, uint64_t lb, uint64_t le, uint64_t* out_l, uint64_t* out_c,
                                 hipStream_t s);

// ---------------------------------------------------------------------------
// segment morphology (ctg_morph.hip).  Call-sized pool buffers only, as the
// label overlaps.
// ---------------------------------------------------------------------------
constexpr int MORPH_WORDS = 10;   // u64 words of a moments row: n, sum z y x, min z y x, max z y x
// The moments of the box [b, e) of a label volume (bits: 32 or 64) into r
// (nodes, moments), coordinates = array index + origin.  *overflow: a label
// >= 2^32 was met -- r is untouched and the caller relabels densely.
hipError_t morph_tables(Workspace& w, const void* A, int bits, const int64_t* shape, const int64_t* b,
                        const int64_t* e, const int64_t* origin, hipStream_t s, ctg_result* r, unsigned* overflow);
// n > 0 rows of CTG_MORPH_COLS float64 (device), in any order -> r: rows of one
// id combine.  *bad: some id was not an integer in [0, 2^53), or a size / box
// entry was negative or not finite (r is untouched).
hipError_t morph_merge(Workspace& w, const double* rows, int64_t n, hipStream_t s, ctg_result* r, int* bad);
// moments -> float64 rows: compact into rows (N x CTG_MORPH_COLS) and / or
// scattered into the zeroed dense table out over the labels [lb, le); either
// may be null
hipError_t launch_morph_rows(const ctg_result* r, uint64_t lb, uint64_t le, double* out, double* rows, hipStream_t s);

// ---------------------------------------------------------------------------
// region features (ctg_region.hip).  Call-sized pool buffers only, as the
// label overlaps.
// ---------------------------------------------------------------------------
constexpr int REGION_WORDS = 3;   // u64 words of a record: n, the f64 sum's bits, f2ord(min) | f2ord(max) << 32
// The count, sum, min and max of D (kind: CTG_DATA_F32 / CTG_DATA_U8) per label
// of the box [b, e) of A (bits: 32 or 64) into r (nodes, reg_*; nothing where
// every voxel is ignored); voxels whose label equals `ignore` are skipped
// (has_ignore).  *overflow: a counted label >= 2^32 was met -- r is untouched
// and the caller relabels densely.
hipError_t region_tables(Workspace& w, const void* A, int bits, const void* D, int kind, const int64_t* shape,
                         const int64_t* b, const int64_t* e, int has_ignore, uint64_t ignore, hipStream_t s,
                         ctg_result* r, unsigned* overflow);
// n > 0 rows of CTG_REGION_COLS float64 in the sum form (device), in any order
// -> r: rows of one id combine.  *bad: some id was not an integer in [0, 2^53),
// or a count was negative or not finite (r is untouched).
hipError_t region_merge(Workspace& w, const double* rows, int64_t n, hipStream_t s, ctg_result* r, int* bad);
// region moments -> float64 rows of `form`: compact into rows (N x
// CTG_REGION_COLS) and / or scattered into the zeroed dense table out over the
// labels [lb, le); either may be null
hipError_t launch_region_rows(const ctg_result* r, uint64_t lb, uint64_t le, int form, double norm, double* out,
                              double* rows, hipStream_t s);

// ---------------------------------------------------------------------------
// applying an assignment (ctg_take.hip).  Call-sized pool buffers only, as the
// label overlaps.
// ---------------------------------------------------------------------------
struct TakeArgs {               // one launch of k_take
    const void* labels;         // n labels of the launch's width
    uint64_t* out;              // n values, or null: check only
    const int64_t* seg_begin;   // device: n_seg + 1 entries, ascending from 0 to n
    const uint64_t* seg_off;    // device: the label offset of each segment
    const uint32_t* prefix;     // device: workgroups before each segment (ctg_plan.h: take_chunk_prefix)
    int n_seg;
    const uint64_t* table;      // dense: the table; sparse: the hash table of ctg_take.h
    uint64_t size;              // dense: its entries; sparse: its slots
    unsigned long long* seg_nonzero;   // device, zeroed: nonzero input voxels, nz_slots partial counts per segment
    int nz_slots;               // a power of two (ctg_plan.h: take_count_slots); workgroup w adds to slot w mod nz_slots
    unsigned long long* missing;       // device: [0] missing voxels (zeroed), [1] the smallest missing label (all ones)
    int par;                    // parity of the labels' address in elements: pairs start where index + par is even
    int wide_store;             // such pairs are 16-byte aligned in out, too
};
// n (key, value) pairs into the zeroed-to-free table of cap slots; stat[0]
// counts the duplicates, stat[1] folds the largest value (both zeroed before)
hipError_t launch_take_build(const uint64_t* keys, const uint64_t* vals, int64_t n, uint64_t* table, uint64_t cap,
                             unsigned long long* stat, hipStream_t s);
hipError_t launch_take_max(const uint64_t* table, int64_t n, unsigned long long* stat, hipStream_t s);
// chunks: prefix[n_seg], the launch's workgroups
hipError_t launch_take(const TakeArgs& A, int label_bits, bool dense, uint32_t chunks, hipStream_t s);

// ---------------------------------------------------------------------------
// thresholded components (ctg_cc.hip).  Call-sized pool buffers only, as the
// label overlaps.
// ---------------------------------------------------------------------------
// The words of a call's small device block: the box's value range as f2ord
// words and its NaN flag, the error word (bit 0: a find or union passed its
// step cap; bit 1: a pair member that is 0 or not below n_labels), the number
// of sets
enum CcWord : int { CC_W_MIN = 0, CC_W_MAX = 1, CC_W_NAN = 2, CC_W_ERR = 3, CC_W_TOTAL = 4, CC_WORDS = 8 };
constexpr uint32_t CC_ERR_CAP = 1u, CC_ERR_PAIR = 2u;
struct CcArgs {                 // the box of a labelling call
    const void* data;           // the array's samples (float32 or uint8)
    const uint8_t* mask;        // the array's mask, or null
    VolBox box;                 // the box in the array (ctg_plan.h: vol_box)
    uint32_t nt[3];             // its tiles (ctg_plan.h: cc_grid)
    float threshold;
    int mode;                   // CTG_CC_*
    uint32_t* words;            // device: CcWord
    uint32_t* parent;           // device: one entry per voxel of the box, box-linear
};
// the smallest and largest sample of the box and whether it holds a NaN
hipError_t launch_cc_range(const CcArgs& A, int data_kind, hipStream_t s);
// per tile: threshold, label in LDS, each foreground voxel's tile root into parent (background: UF_NONE)
hipError_t launch_cc_tile(const CcArgs& A, const CcGrid& G, int data_kind, int normalize, int conn, hipStream_t s);
// the unions across tile borders
hipError_t launch_cc_seams(const CcArgs& A, const CcGrid& G, int conn, hipStream_t s);
// n parent entries = their own index
hipError_t launch_uf_init(uint32_t* parent, int64_t n, hipStream_t s);
// one union per (a, b) pair; a member that is 0 or >= n_labels raises CC_ERR_PAIR instead
hipError_t launch_uf_pairs(const uint64_t* pairs, int64_t n, uint32_t* parent, uint32_t n_labels, uint32_t* words,
                           hipStream_t s);
// every node's root into parent; each root's rank within its CC_SEG-node segment into rank, the roots of
// each segment into seg
hipError_t launch_uf_flatten(uint32_t* parent, int64_t n, uint32_t* rank, uint32_t* seg, uint32_t* words,
                             hipStream_t s);
// seg -> its exclusive prefix, the sum into words[CC_W_TOTAL]
hipError_t launch_uf_scan(uint32_t* seg, int64_t n_seg, uint32_t* words, hipStream_t s);
// out[i] = rank of i's root among all roots + plus; 0 where parent[i] is UF_NONE
hipError_t launch_uf_write(const uint32_t* parent, const uint32_t* rank, const uint32_t* seg, int64_t n,
                           uint64_t plus, uint64_t* out, hipStream_t s);

// ---------------------------------------------------------------------------
// exact Euclidean distance transform (ctg_edt.hip).  Call-sized pool buffers
// only, as the label overlaps.
// ---------------------------------------------------------------------------
struct EdtSrc {                 // the box of a call and its seed predicate
    const void* src;            // the array (uint8, float32, uint32 or uint64)
    VolBox box;                 // the box in the array (ctg_plan.h: vol_box)
    float threshold;            // CTG_EDT_SRC_GREATER
    uint64_t label;             // CTG_EDT_SRC_EQUAL
    int invert;                 // CTG_EDT_TO_BACKGROUND: the seeds are where the predicate fails
};
constexpr int EDT_PART_WORDS = 3;   // a workgroup's partial of the last pass: D2 bits, its first index, voxels without a seed
struct EdtLineArgs {            // one envelope pass (y or z)
    const void* in;             // box-shaped u16 |dx| (x pass) or u32 (|dy|, |dx| << 16) (y pass)
    void* out;                  // box-shaped u32 pairs, or with final_pass the float32 result (out_d2: float64 D2)
    int in32, final_pass, out_d2;
    int axis;                   // the line's axis: 1 y, 0 z
    uint32_t n[3];
    double p[3];                // the pitch (z, y, x)
    double diag2;               // edt_diag2: D2 of a voxel without a seed in its domain
    uint64_t* stack;            // the stack buffer of edt_line_plan, or null (LDS)
    unsigned long long* part;   // final_pass: EDT_PART_WORDS words per workgroup
};
// kind: 0 uint8 != 0, 1 float32 > threshold, 2 uint32 == label, 3 uint64 == label; |dx| of every voxel into out,
// the seeds added to *info (zeroed before)
hipError_t launch_edt_x(const EdtSrc& A, int kind, uint16_t* out, unsigned long long* info, hipStream_t s);
hipError_t launch_edt_line(const EdtLineArgs& A, const EdtLinePlan& P, hipStream_t s);
// n partials -> info[1 .. 3]
hipError_t launch_edt_fold(const unsigned long long* part, int64_t n, unsigned long long* info, hipStream_t s);

// ---------------------------------------------------------------------------
// seeded watershed (ctg_ws.hip).  Call-sized pool buffers only, as the label
// overlaps.
// ---------------------------------------------------------------------------
// The u64 words of a call's small device block: the NaN flag and the seeded
// voxels of the box, a round's hooks, whether a chase stopped short, the error
// word (never raised by a sound launch: a pick without an edge), and the
// result's largest label, its voxels left 0 and the labels the filter dropped
enum WsWord : int {
    WS_W_NAN = 0, WS_W_SEEDED = 1, WS_W_HOOKS = 2, WS_W_SHORT = 3, WS_W_ERR = 4, WS_W_MAX = 5, WS_W_ZERO = 6,
    WS_W_DROPPED = 7, WS_WORDS = 8
};
struct WsArgs {                 // one flood
    const float* hmap;          // the array's heights
    const void* seeds;          // the array's seeds (seed_bits 32 or 64)
    int seed_bits;
    VolBox box;                 // the box in both arrays (ctg_plan.h: vol_box)
    int two_d;
    uint32_t* parent;           // box-linear, as the three below (ctg_plan.h: ws_plan)
    uint32_t* key;
    unsigned long long* best;
    uint32_t* pick;
    unsigned long long* words;  // device: WsWord
};
// with_keys: the heights' keys and the NaN flag as well (a second flood of the same heights keeps them);
// every voxel its own root, flagged where seeded; the seeded voxels counted
hipError_t launch_ws_init(const WsArgs& A, int with_keys, hipStream_t s);
// one round up to the hooks: both minima, then what every picking root hangs below, counted in WS_W_HOOKS
hipError_t launch_ws_pick(const WsArgs& A, hipStream_t s);
// the hooks into parent
hipError_t launch_ws_apply(const WsArgs& A, hipStream_t s);
// one chase launch; WS_W_SHORT is raised where an entry is not yet its root
hipError_t launch_ws_chase(const WsArgs& A, hipStream_t s);
// out[i] = the seed of i's root, 0 without one; the largest label and the voxels left 0 folded into words
hipError_t launch_ws_write(const WsArgs& A, uint64_t* out, hipStream_t s);
// The size filter over the slab [v0, v0 + n) of out, whose labels and voxel counts are (nodes, moments) of a
// morphology table: labels with fewer than `size` voxels there become 0; the dropped labels added to WS_W_DROPPED
hipError_t launch_ws_filter(uint64_t* out, int64_t n, const uint64_t* nodes, const uint64_t* moments, int64_t n_nodes,
                            uint64_t size, unsigned long long* words, hipStream_t s);

hipError_t mgpu_sample(const uint64_t* edges, int64_t E, int64_t* meta, hipStream_t s);
hipError_t mgpu_split(const uint64_t* edges, int64_t E, const uint64_t* nodes, int64_t N, const int64_t* meta_all,
                      int world, uint64_t* spl, int64_t* counts, hipStream_t s);
// the rows and node ids of every send segment (ctg_plan.h: exchange_plan) into send
hipError_t mgpu_pack(const ctg_result* r, const ExchangeSegs& S, int64_t* send, hipStream_t s);

// What the merge kernels read and write: the own range of the local table,
// the received rows, and one entry per distinct received key.
struct MergeIO {
    // own range of the local table (rows [0, n_own) after offsetting)
    const uint64_t* own_edges;
    const double* own_feats;
    const uint32_t* own_wide;
    const double2* own_sums;
    DeferredStats defer;  // on: own rows' statistics from the records (own row i = run own_row0 + i)
    int64_t own_row0;
    int64_t n_own;
    // received rows, sorted order and runs
    const uint64_t* recv;
    const uint32_t* order;
    const uint64_t* skeys;
    const uint32_t* run0;
    const uint32_t* nK;
    // per unique received key k
    uint64_t* mkeys;      // (K,2)
    double* mfeats;       // (K,10)
    uint32_t* mkeep;      // keep (ADJ proved, or every key for boundary maps)
    uint32_t* mnew;       // key absent from the own range
    int64_t* mins;        // own rows with a smaller key
    uint32_t* touched;    // (n_own) 1 + k of the received key that matches own row i, 0 none
    int partial_adj;      // keys need the ADJ bit (affinity partials)
    double scale, offset;
};
// The merge's launches over the receive segments S, in the order of the steps
// of ctg_mgpu_merge (ctg_api_mgpu.hip).  own[0, n_own) and the node ids of
// every received segment -> out:
hipError_t mgpu_node_list(const ExchangeSegs& S, const int64_t* recv, const uint64_t* own, int64_t n_own,
                          uint64_t* out, hipStream_t s);
// the received rows in key order: order[pos] = received row, skeys[pos] = its (u,v)
hipError_t mgpu_order(const ExchangeSegs& S, const int64_t* recv, uint32_t* order, uint64_t* skeys, hipStream_t s);
// runs of equal keys among the M sorted keys: run0[k] = first position of run
// k, run0[K] = M, K in *nK (head, rid: M words of scratch each)
hipError_t mgpu_runs(Workspace& w, int64_t M, const uint64_t* skeys, uint32_t* head, uint32_t* rid, uint32_t* run0,
                     uint32_t* nK, hipStream_t s);
// every run combined with the own row of its key; nrank = exclusive scan of io.mnew
hipError_t mgpu_combine(Workspace& w, const ExchangeSegs& S, const MergeIO& io, uint32_t* nrank, hipStream_t s);
// the keep flag of every merged-order slot; fpos = its exclusive scan
hipError_t mgpu_slots(Workspace& w, const MergeIO& io, const uint32_t* nrank, int64_t n_slots, uint32_t* keep,
                      uint32_t* fpos, hipStream_t s);
// the kept rows to out_e / out_f, their number to *n_out
hipError_t mgpu_scatter(const MergeIO& io, const uint32_t* nrank, const uint32_t* keep, const uint32_t* fpos,
                        int64_t n_slots, uint64_t* out_e, double* out_f, uint32_t* n_out, hipStream_t s);
}  // namespace ctg

// in functions that return hipError_t: pass a failure up
#define CTG_TRY(expr)                        \
    do {                                     \
        hipError_t e_ = (expr);              \
        if (e_ != hipSuccess) return e_;     \
    } while (0)

#define CTG_CHECK(expr)                                                        \
    do {                                                                       \
        hipError_t e_ = (expr);                                                \
        if (e_ != hipSuccess) {                                                \
            ctg::set_error(std::string(#expr) + ": " + hipGetErrorString(e_)); \
            return CTG_ERR_HIP;                                                \
        }                                                                      \
    } while (0)
