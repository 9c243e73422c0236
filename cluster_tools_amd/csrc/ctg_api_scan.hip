// C ABI of libctg.so (include/ctg.h): the face scan -- ctg_rag_features on a
// whole array, ctg_rag_blocks on a batch of arrays.  Each entry point is a
// sequence of the steps below; what a step decides on the host is a pure
// function of ctg_plan.h, and the environment switches are read once per call
// (scan_switches).  The record back half is ctg_records.hip.
//
// Lifetime rule, for every buffer a queued kernel reads (the Bloom filter and
// its graph, the block tables, dense or widened labels): it is freed only
// after the stream is synchronised (AdjFilter, BlockTables: their destructors
// synchronise first, on every return path), or it goes back to the pool while
// still in use and the pool's stream-ordered reuse keeps a later user behind
// the kernel (ctg_buffers.h) -- a later user of this call, on this stream: both
// entry points wait for the stream before they return, so no call on another
// stream meets such a block (include/ctg.h, "Streams").
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "ctg_api.h"

using namespace ctg;

// ---------------------------------------------------------------------------
// switches
// ---------------------------------------------------------------------------
// The environment switches of a face scan, read once per call (tests toggle
// them between calls).  A batched call has the first two only.
struct ScanSwitches {
    int tile_z = 0;          // CTG_TILE_Z (tests): planes per workgroup, of both widths for a whole array; 0: unset
    bool rec_fresh = false;  // CTG_REC_FRESH (test hook): start from the smallest record buffer
    int tile_z_narrow = 0;   // CTG_TILE_Z_NARROW (A/B): planes of the narrow-tile launch; 0: unset
    bool tail_tiles = true;  // CTG_TAIL_TILES=0: no tail tiles (ctg_scan.hip)
    int narrow_rows = -1;    // CTG_NARROW_ROWS=0/1 forces a tile width (boundary maps); -1: unset
    bool skip_adj = true;    // CTG_SKIP_ADJ=0 keeps the adjacency markers
    bool nn3 = true;         // CTG_NN3=0 keeps the channel loop
    bool interior = true;    // CTG_SCAN_INTERIOR=0: every wave takes the general plane loop (A/B, tests)
    int ablate = 0;          // CTG_ABLATE: scan ablations (CTG_DIAG builds only)
};

static ScanSwitches scan_switches(bool whole_array, bool boundary_map) {
    ScanSwitches sw;
    if (const char* t = getenv("CTG_TILE_Z")) sw.tile_z = std::max(1, atoi(t));
    sw.rec_fresh = getenv("CTG_REC_FRESH") != nullptr;
    if (!whole_array) return sw;
    if (const char* t = getenv("CTG_TILE_Z_NARROW")) sw.tile_z_narrow = std::max(1, atoi(t));
    if (const char* t = getenv("CTG_TAIL_TILES")) sw.tail_tiles = t[0] != '0';
    if (boundary_map)
        if (const char* t = getenv("CTG_NARROW_ROWS")) sw.narrow_rows = atoi(t) ? 1 : 0;
    if (const char* t = getenv("CTG_SKIP_ADJ")) sw.skip_adj = atoi(t) != 0;
    if (const char* t = getenv("CTG_NN3")) sw.nn3 = t[0] != '0';
    if (const char* t = getenv("CTG_SCAN_INTERIOR")) sw.interior = t[0] != '0';
#ifdef CTG_DIAG
    if (const char* t = getenv("CTG_ABLATE")) sw.ablate = atoi(t);
#endif
    return sw;
}

// ---------------------------------------------------------------------------
// steps both entry points take
// ---------------------------------------------------------------------------
// stage: the label and the data volume (or arena) on the device
static int stage_volumes(Workspace& w, const void* labels, size_t lbytes, const void* data, size_t dbytes, int mem,
                         hipStream_t s, const void** dl, const void** dd) {
    const int rc = stage_in(w.stage[0], labels, lbytes, mem, s, dl);
    return rc ? rc : stage_in(w.stage[1], data, dbytes, mem, s, dd);
}

// The ScanParams fields common to the whole-array and the batched scan:
// pointers, kinds, channel offsets (and their classes), histogram mapping.
static ChannelClass scan_common(ScanParams& P, const void* dl, const void* dd, int label_bits, int data_kind,
                                int n_channels, const int32_t* offsets, double hist_lo, double hist_hi) {
    std::memset(&P, 0, sizeof(P));
    P.labels = dl;
    P.data = dd;
    P.label_bits = label_bits;
    P.data_kind = dd ? data_kind : CTG_DATA_NONE;
    P.n_channels = dd ? n_channels : 0;
    for (int c = 0; c < P.n_channels; ++c)
        for (int k = 0; k < 3; ++k) P.offsets[c][k] = offsets[3 * c + k];
    const ChannelClass cc = classify_channels(P.offsets, P.n_channels);
    P.lr_mask = cc.lr_mask;
    P.scale = (double)NBINS / (hist_hi - hist_lo);
    P.offset = hist_lo;
    P.fast40 = (hist_lo == 0.0 && P.scale == 40.0) ? 1 : 0;
    // flush decisions every check_planes planes (overflow safety does not
    // depend on it: ctg_scan.hip's per-wave sample budget bounds every count)
    P.check_planes = 8;
    P.xcd_remap = 1;
    return cc;
}

// scan with records: one face scan with its record bookkeeping -- the record
// buffer grows and the scan re-runs when a region overflowed.  *overflow =
// labels that do not fit the key's u / v fields (the caller relabels densely).
static int scan_records(Workspace& w, const ScanParams& P, int64_t V, hipStream_t s, const ScanSwitches& sw, Ev& ev,
                        RegionPrefix& pre, bool* overflow, const char* who) {
    *overflow = false;
    if (sw.rec_fresh) {
        CTG_CHECK(hipStreamSynchronize(s));
        free_records(w);
    }
    int64_t need = record_slots_first(w.rec.cap, V);
#ifdef CTG_DIAG   // CTG_WG_TIMES=<file>: per-workgroup (start, end) clock of the (last) scan launch
    static const char* wg_path = getenv("CTG_WG_TIMES");
    ScanParams PW = P;
    size_t wg_n = 0;
    if (wg_path && !P.blocks) {
        const int64_t rows = std::min(scan_tile_rows(), scan_tile_rows_narrow());
        const int64_t tz = std::max(1, std::min(std::min(P.tile_z, P.tile_z_narrow > 0 ? P.tile_z_narrow : P.tile_z),
                                                std::max(8, P.tile_z / 4)));   // (tail tiles)
        wg_n = (size_t)((P.shape[2] + 63) / 64) * (size_t)((P.shape[1] + rows - 1) / rows) *
               (size_t)((P.shape[0] + tz - 1) / tz);   // >= the tile count of either width
        CTG_CHECK(hipMalloc(&PW.wg_times, wg_n * 16));
        CTG_CHECK(hipMemsetAsync(PW.wg_times, 0, wg_n * 16, s));
    }
#else
    const ScanParams& PW = P;
#endif
    for (int attempt = 0; attempt < 4; ++attempt) {
        CTG_CHECK(ensure_records(w, need, 0));
        CTG_CHECK(hipMemsetAsync(w.counters, 0, sizeof(Counters), s));
        ev.mark(0);   // (re-recorded here: the scan phase brackets the scan launch alone)
        CTG_CHECK(launch_face_scan(PW, w.rec, w.counters, s, &w.last_scan));
        ev.mark(1);
        CTG_CHECK(hipMemcpyAsync(w.counters_host, w.counters, sizeof(Counters), hipMemcpyDeviceToHost, s));
        CTG_CHECK(hipStreamSynchronize(s));
        if (w.counters_host->label_overflow) {
            *overflow = true;
            return CTG_OK;
        }
        const RegionFold f = fold_regions(w.counters_host->rcount);
        pre = f.pre;
        w.counters_host->n_records = f.total;
        if (f.total >= (1ull << 32)) {
            set_error(std::string(who) + ": more than 2^32 records");
            return CTG_ERR_NOMEM;
        }
        if ((int64_t)f.fullest <= w.rec.rcap) break;
        need = record_slots_regrow(f.fullest);
        if (attempt == 3) {
            set_error(std::string(who) + ": record buffer overflow");
            return CTG_ERR_NOMEM;
        }
    }
    if (P.ablate & 256)   // diagnostic s_memtime stamps, summed over waves
        fprintf(stderr, "stamps total %llu fold %llu flush %llu wait %llu drain %llu floor %llu\n",
                w.counters_host->pad[2], w.counters_host->pad[3], w.counters_host->pad[4], w.counters_host->pad[5],
                w.counters_host->pad[7], w.counters_host->pad[0]);
#ifdef CTG_DIAG
    if (PW.wg_times) {   // raw (start, end) pairs; unused slots stay 0; then the flush count
        std::vector<unsigned long long> h(wg_n * 2);
        CTG_CHECK(hipMemcpy(h.data(), PW.wg_times, wg_n * 16, hipMemcpyDeviceToHost));
        CTG_CHECK(hipFree(PW.wg_times));
        if (FILE* f = fopen(wg_path, "wb")) {
            fwrite(h.data(), 16, wg_n, f);
            fclose(f);
        }
        fprintf(stderr, "wg_times %s: %zu slots, flushes %llu, records %llu\n", wg_path, wg_n,
                w.counters_host->pad[6], w.counters_host->n_records);
    }
#endif
    w.last_records = (int64_t)w.counters_host->n_records;
    w.last_direct = (int64_t)w.counters_host->n_direct;
    return CTG_OK;
}

// fill ReduceJob: what the reduce of a scan's records takes from the scan
// (scanned: it ran -- else no record), and the record counts of the handle
static ReduceJob scan_job(const Workspace& w, const ScanParams& P, const RegionPrefix& pre, bool scanned,
                          int ignore_label, int flags, ctg_result* r) {
    ReduceJob J{};
    J.n = r->n_records = scanned ? (int64_t)w.counters_host->n_records : 0;
    r->n_direct = scanned ? (int64_t)w.counters_host->n_direct : 0;
    J.keys = w.rec.key;
    J.regions = &pre;
    J.R = w.rec;
    J.stats = P.data_kind != CTG_DATA_NONE;
    J.ignore_label = ignore_label;
    J.keep_stats = (flags & CTG_KEEP_STATS) ? 1 : 0;
    J.max_v = scanned ? w.counters_host->max_v : 0;
    J.scale = P.scale;
    J.offset = P.offset;
    return J;
}

// ---------------------------------------------------------------------------
// dense relabelling
// ---------------------------------------------------------------------------
// The dense relabellings below map a label to its rank in the sorted unique
// label table U.  The reduce recognises the ignore label as dense id 0, so with
// ignore_label set the table must start with label 0 even where the array
// holds no 0 -- else the smallest real label would become 0 and its edges
// would be dropped.  Puts a 0 in front of U->nodes when U[0] != 0.
static int keep_zero_first(ctg_result* U, hipStream_t s) {
    uint64_t first = 0;
    if (U->n_nodes > 0) {
        CTG_CHECK(hipMemcpyAsync(&first, U->nodes, 8, hipMemcpyDeviceToHost, s));
        CTG_CHECK(hipStreamSynchronize(s));
    }
    if (U->n_nodes > 0 && first == 0) return CTG_OK;
    DevBuf<uint64_t> t((size_t)(U->n_nodes + 1) * 8);
    if (!t) {
        set_error("out of device memory for the dense relabelling table");
        return CTG_ERR_NOMEM;
    }
    CTG_CHECK(hipMemsetAsync(t, 0, 8, s));
    if (U->n_nodes)
        CTG_CHECK(hipMemcpyAsync(t + 1, U->nodes, (size_t)U->n_nodes * 8, hipMemcpyDeviceToDevice, s));
    dev_free(U->nodes);   // stream-ordered reuse
    U->nodes = t.release();
    U->n_nodes += 1;
    return CTG_OK;
}

// dense re-entry.  Labels that do not fit the face keys' u / v fields -- >=
// 2^32 for a whole array (the keys pack (u,v) as 32+32 bits), >=
// 2^tag_shift for batched blocks: the n labels are relabelled densely through
// their sorted unique labels (a monotone map: sorted dense tables stay sorted
// after mapping back), `rerun` makes the call again on the 32-bit dense labels,
// and the edge and node tables are mapped back.  shape: a whole array (its
// unique labels come from the tile pass), or null.  At most `limit` distinct
// labels.
template <class Rerun>
static int rag_dense_relabel(const uint64_t* l64, int64_t n, const int64_t* shape, int ignore_label, int64_t limit,
                             const char* who, const char* limit_msg, void* stream, Rerun&& rerun, ctg_result** out) {
    hipStream_t s = (hipStream_t)stream;
    ResultPtr U, r;
    int rc = nested(U, [&](ctg_result** u) {
        return shape ? ctg_unique_labels(l64, shape, nullptr, nullptr, CTG_MEM_DEVICE, stream, u)
                     : ctg_unique_values(l64, n, CTG_MEM_DEVICE, stream, u);
    });
    if (rc) return rc;
    if (ignore_label && (rc = keep_zero_first(U.get(), s)) != CTG_OK) return rc;
    if (U->n_nodes > limit) {
        set_error(std::string(who) + limit_msg);
        return CTG_ERR_UNSUPPORTED;
    }
    DevBuf<uint32_t> dense(std::max<int64_t>(n, 1) * 4);
    if (!dense) {
        set_error(std::string(who) + ": out of device memory for the dense relabelling");
        return CTG_ERR_NOMEM;
    }
    CTG_CHECK(launch_remap_dense(l64, n, U->nodes, U->n_nodes, dense, s));
    rc = nested(r, [&](ctg_result** rr) { return rerun((const uint32_t*)dense, rr); });
    dense.reset();   // stream-ordered: later users of the block run after the scan
    if (rc) return rc;
    CTG_CHECK(map_back(U.get(), r.get(), s));
    CTG_CHECK(hipStreamSynchronize(s));
    *out = r.release();
    return CTG_OK;
}

// ---------------------------------------------------------------------------
// steps of ctg_rag_features
// ---------------------------------------------------------------------------
static int validate_features(const void* labels, int label_bits, const void* data, int data_kind, int n_channels,
                             const int32_t* offsets, const int64_t* shape, const int64_t* own_begin,
                             const int64_t* own_end, double hist_lo, double hist_hi, ctg_result** out) {
    const char* bad = nullptr;
    if (!out || !shape || !labels) {
        set_error("ctg_rag_features: null argument");
        return CTG_ERR_ARG;
    }
    *out = nullptr;
    if (label_bits != 32 && label_bits != 64) bad = "label_bits must be 32 or 64";
    else if (n_channels < 0 || n_channels > CTG_MAX_CHANNELS || (n_channels > 0 && !offsets))
        bad = "bad channel/offset arguments";
    else if (data && data_kind != CTG_DATA_F32 && data_kind != CTG_DATA_U8)
        bad = "data_kind must be CTG_DATA_F32 or CTG_DATA_U8";
    else if (!(hist_hi > hist_lo)) bad = "hist_hi must be > hist_lo";
    else
        for (int k = 0; k < 3; ++k)
            if (shape[k] < 0 || (own_begin && (own_begin[k] < 0)) || (own_end && own_end[k] < 0))
                bad = "negative shape/own_begin/own_end";
    if (!bad) return CTG_OK;
    set_error(std::string("ctg_rag_features: ") + bad);
    return CTG_ERR_ARG;
}

// plan tiles: the array, its owned box and the tile depths of both widths
static void plan_whole_tiles(ScanParams& P, const int64_t* shape, const int64_t* own_begin, const int64_t* own_end,
                             const ScanSwitches& sw) {
    for (int k = 0; k < 3; ++k) {
        P.shape[k] = shape[k];
        P.own_begin[k] = own_begin ? own_begin[k] : 0;
        P.own_end[k] = own_end ? std::min(own_end[k], shape[k]) : shape[k];
    }
    const TileDepths td = scan_tile_depths(shape, scan_tile_rows(), scan_tile_rows_narrow());
    P.tile_z = td.tile_z;
    P.tile_z_narrow = td.tile_z_narrow;
    if (sw.tile_z) P.tile_z_narrow = P.tile_z = sw.tile_z;
    if (sw.tile_z_narrow) P.tile_z_narrow = sw.tile_z_narrow;
    P.ablate = sw.ablate;
    P.tail_tiles = sw.tail_tiles;
    P.interior = sw.interior;
}

// density probe: the tile width of a boundary map (narrow_rows_mode) -- where
// the device decides, from the sampled x-face density (cell 10 ~ 0.10, cell 5
// ~ 0.20 changes per pair; threshold 0.14), without a host round trip
static int density_probe(Workspace& w, ScanParams& P, int mode, hipStream_t s) {
    P.narrow_rows = mode;
    if (mode != 2) return CTG_OK;
    P.density = w.small + SLOT_DENSITY;
    CTG_CHECK(hipMemsetAsync(w.small + SLOT_DENSITY, 0, 2 * sizeof(uint32_t), s));
    CTG_CHECK(launch_density(P.labels, P.label_bits, P.shape, 512, w.small + SLOT_DENSITY, s));
    return CTG_OK;
}

// adjacency filter.  Long-range affinity channels: a sample
// counts only if its (u,v) is a RAG edge.  Filtering in the scan (against the
// edge set of a graph-only pass) keeps the non-adjacent pairs -- most
// long-range pairs -- out of the edge tables and records.  Labels >= 2^32 get
// the graph but no filter here: the dense-relabel path re-enters with 32-bit
// labels and filters there.  The filter is a Bloom prefilter (bloom_blocks):
// one load per long-range sample (vs. a probe chain in a set 4x the size); the
// reduce drops its false positives (keys no nearest-neighbour sample flagged).
struct AdjFilter {
    hipStream_t s;
    ResultPtr graph;
    DevBuf<unsigned long long> bloom;
    StreamWait wait{s, false};   // armed once the filter exists
};

static int adjacency_filter(ScanParams& P, const int64_t* shape, const int64_t* own_begin, const int64_t* own_end,
                            double hist_lo, double hist_hi, void* stream, AdjFilter& f) {
    hipStream_t s = f.s;
    int rc = nested(f.graph, [&](ctg_result** g) {
        return ctg_rag_features(P.labels, P.label_bits, nullptr, CTG_DATA_NONE, 0, nullptr, shape, own_begin, own_end, 0,
                                hist_lo, hist_hi, 0, CTG_MEM_DEVICE, stream, g);
    });
    if (rc) return rc;
    const ctg_result* g = f.graph.get();
    uint64_t mx = 0;
    if (g->n_edges > 0) {
        // largest label of the sorted edge table: the v of some row; the max
        // over all v equals the last node
        CTG_CHECK(hipMemcpyAsync(&mx, g->nodes + g->n_nodes - 1, 8, hipMemcpyDeviceToHost, s));
        CTG_CHECK(hipStreamSynchronize(s));
    }
    if (mx >> 32) return CTG_OK;
    const uint32_t blocks = bloom_blocks(g->n_edges);
    if (!f.bloom.alloc((size_t)blocks * 64)) {
        set_error("ctg_rag_features: out of memory (adjacency filter)");
        return CTG_ERR_NOMEM;
    }
    f.wait.arm();
    if ((rc = hip_status(launch_build_bloom(g->edges, g->n_edges, f.bloom, blocks - 1, s), "ctg_rag_features",
                         CTG_ERR_HIP)) != CTG_OK)
        return rc;
    P.bloom = f.bloom;
    P.bloom_mask = blocks - 1;
    return CTG_OK;
}

// channel plan: which channels scan as faces, and whether markers are pushed
static void plan_scan_channels(ScanParams& P, const ChannelClass& cc, int flags, const ScanSwitches& sw) {
    const ChannelPlan cp = plan_channels(cc, P.n_channels, !(flags & CTG_NO_ADJ_FILTER), P.bloom != nullptr,
                                         sw.skip_adj, sw.nn3);
    P.skip_adj_marks = cp.skip_adj_marks;
    P.nn3 = cp.nn3;
    P.nn_mix = cp.nn_mix;
    if (cp.nn3 || cp.nn_mix)
        for (int a = 0; a < 3; ++a) P.nn_ch[a] = cc.nn_ch[a];
    if (cp.nn_mix) {
        P.n_loop = cc.n_loop;
        for (int i = 0; i < cc.n_loop; ++i) P.loop_ch[i] = cc.loop_ch[i];
    }
}

// single-label fix: an array with one label has no record, and its only node
// is the owned box's first voxel (`at`: its element index, or -1 where
// nothing is owned).  64-bit labels: the reduce reads it on the device ...
static int64_t single_label_index(const ScanParams& P) {
    for (int k = 0; k < 3; ++k)
        if (P.own_begin[k] >= P.own_end[k]) return -1;
    return (P.own_begin[0] * P.shape[1] + P.own_begin[1]) * P.shape[2] + P.own_begin[2];
}
// ... 32-bit labels: widened here, after the reduce
static hipError_t widen_single_label(const ScanParams& P, int64_t at, hipStream_t s, ctg_result* r) {
    if (P.label_bits != 32 || r->n_records != 0 || at < 0) return hipSuccess;
    uint32_t l32 = 0;
    hipError_t e = hipMemcpyAsync(&l32, (const uint32_t*)P.labels + at, 4, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    const uint64_t l64 = l32;   // (on s like the rest of the call, and waited for: l64 is a local)
    if (e == hipSuccess) e = hipMemcpyAsync(r->nodes, &l64, 8, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    r->n_nodes = 1;
    return e;
}

// ---------------------------------------------------------------------------
// steps of ctg_rag_blocks
// ---------------------------------------------------------------------------
static int block_plan_error(const BlockPlan& plan) {
    const std::string block = "ctg_rag_blocks: block " + std::to_string(plan.bad_block);
    if (plan.error == BlockPlan::BOX_OUTSIDE) set_error(block + ": box outside its array");
    else if (plan.error == BlockPlan::ARRAY_OUTSIDE) set_error(block + ": array outside the arena");
    else set_error("ctg_rag_blocks: too many tiles in one call");
    return CTG_ERR_ARG;
}

// the block geometry and the scan's tile prefix on the device, and with them
// the batch fields of the scan's parameters: the scan and the node pass read
// the tables until the call is done
struct BlockTables {
    hipStream_t s;
    DevBuf<BlockGeom> geom;
    DevBuf<uint32_t> prefix;
    StreamWait wait{s};
};

static int upload_block_tables(const BlockPlan& plan, int n_blocks, hipStream_t s, BlockTables& t, ScanParams& P) {
    P.tile_z = plan.tile_z;
    P.tag_shift = plan.tag_shift;
    P.label_hi_mask = plan.label_hi_mask;
    P.n_blocks = n_blocks;
    P.batch_tiles = plan.prefix[n_blocks];
    t.geom.alloc(sizeof(BlockGeom) * n_blocks);
    t.prefix.alloc((n_blocks + 1) * 4);
    if (!t.geom || !t.prefix) {
        set_error("ctg_rag_blocks: out of device memory");
        return CTG_ERR_NOMEM;
    }
    CTG_CHECK(hipMemcpyAsync(t.geom, plan.geom.data(), sizeof(BlockGeom) * n_blocks, hipMemcpyHostToDevice, s));
    CTG_CHECK(hipMemcpyAsync(t.prefix, plan.prefix.data(), (n_blocks + 1) * 4, hipMemcpyHostToDevice, s));
    P.blocks = t.geom;
    P.tile_prefix = t.prefix;
    return CTG_OK;
}

// block offsets: the rows of every block in the sorted edge table, then the
// block tags leave the keys
static hipError_t block_edge_offsets(const ScanParams& P, int tag_bits, uint64_t umask, hipStream_t s, ctg_result* r) {
    const int n_blocks = P.n_blocks;
    r->edge_off.assign(n_blocks + 1, 0);
    r->edge_off[n_blocks] = r->n_edges;
    if (!tag_bits || !r->n_edges) return hipSuccess;
    DevBuf<int64_t> bounds((n_blocks + 1) * 8);
    if (!bounds) return hipErrorOutOfMemory;
    CTG_TRY(launch_block_bounds(r->n_edges, r->edges, 2, n_blocks, P.tag_shift, bounds, s));
    CTG_TRY(hipMemcpyAsync(r->edge_off.data(), bounds, (n_blocks + 1) * 8, hipMemcpyDeviceToHost, s));
    CTG_TRY(launch_clear_bits(r->n_edges, r->edges, 2, umask, s));
    return hipStreamSynchronize(s);
}

// block nodes: unique labels of every own box
static int block_nodes(Workspace& w, const ScanParams& P, const BlockPlan& plan, hipStream_t s, ctg_result* r) {
    const int n_blocks = P.n_blocks;
    const int64_t n_tiles = plan.uprefix.back();
    const char* nomem = "ctg_rag_blocks: out of device memory for the block nodes";
    DevBuf<uint32_t> dprefix((n_blocks + 1) * 4);
    DevBuf<int64_t> bounds((n_blocks + 1) * 8);
    if (!dprefix || !bounds) {
        set_error(nomem);
        return CTG_ERR_NOMEM;
    }
    CTG_CHECK(hipMemcpyAsync(dprefix, plan.uprefix.data(), (n_blocks + 1) * 4, hipMemcpyHostToDevice, s));
    DevBuf<uint64_t> nodes;
    int64_t N = 0;
    const int rc = unique_candidates(
        w, candidate_cap_first(plan.own_voxels), INT64_MAX, 32u + (unsigned)plan.tag_bits, s, nomem,
        "ctg_rag_blocks: node candidate buffer overflow",
        [&](uint64_t* cand, unsigned long long* count, int64_t cap) {
            return launch_unique_blocks(P.labels, P.label_bits, P.blocks, dprefix, n_blocks, n_tiles, cand, count, cap, s);
        },
        nodes, &N);
    if (rc) return rc;
    CTG_CHECK(launch_block_bounds(N, nodes, 1, n_blocks, 32, bounds, s));
    r->node_off.assign(n_blocks + 1, 0);
    CTG_CHECK(hipMemcpyAsync(r->node_off.data(), bounds, (n_blocks + 1) * 8, hipMemcpyDeviceToHost, s));
    CTG_CHECK(launch_clear_bits(N, nodes, 1, 0xFFFFFFFFull, s));
    CTG_CHECK(hipStreamSynchronize(s));
    dev_free(r->nodes);
    r->nodes = nodes.release();
    r->n_nodes = N;
    return CTG_OK;
}

// dense re-entry of a whole array whose scan met labels >= 2^32
static int features_dense_reentry(const void* dl, int label_bits, const void* dd, int data_kind, int n_channels,
                                  const int32_t* offsets, const int64_t* shape, const int64_t* own_begin,
                                  const int64_t* own_end, int ignore_label, double hist_lo, double hist_hi, int flags,
                                  void* stream, ctg_result** out) {
    if (label_bits != 64) {
        set_error("ctg_rag_features: internal label overflow on 32-bit labels");
        return CTG_ERR_HIP;
    }
    const int64_t V = shape[0] * shape[1] * shape[2];
    return rag_dense_relabel(
        (const uint64_t*)dl, V, shape, ignore_label, 0xFFFFFFFFll, "ctg_rag_features",
        ": more than 2^32 distinct labels in one array", stream,
        [&](const uint32_t* dense, ctg_result** r) {
            return ctg_rag_features(dense, 32, dd, data_kind, n_channels, offsets, shape, own_begin, own_end,
                                    ignore_label, hist_lo, hist_hi, flags, CTG_MEM_DEVICE, stream, r);
        },
        out);
}

// dense re-entry of a batch whose labels are too large for the tagged keys:
// the arena is relabelled densely (32-bit labels are widened first)
static int blocks_dense_reentry(const void* dl, int label_bits, const void* dd, int data_kind, int n_channels,
                                const int32_t* offsets, const ctg_block_desc* blocks, int n_blocks,
                                int64_t labels_len, int64_t data_len, int ignore_label, double hist_lo,
                                double hist_hi, int flags, int tag_shift, void* stream, ctg_result** out) {
    hipStream_t s = (hipStream_t)stream;
    const uint64_t* l64 = (const uint64_t*)dl;
    DevBuf<uint64_t> wide;
    if (label_bits == 32) {
        if (!wide.alloc(std::max<int64_t>(labels_len, 1) * 8)) {
            set_error("ctg_rag_blocks: out of device memory widening the labels");
            return CTG_ERR_NOMEM;
        }
        CTG_CHECK(launch_u32_to_u64(labels_len, (const uint32_t*)dl, wide, s));
        l64 = wide;
    }
    return rag_dense_relabel(
        l64, labels_len, nullptr, ignore_label, (int64_t)(1ull << tag_shift), "ctg_rag_blocks",
        ": too many distinct labels for one batch of blocks: call with fewer blocks", stream,
        [&](const uint32_t* dense, ctg_result** r) {
            const int rc = ctg_rag_blocks(dense, 32, dd, data_kind, n_channels, offsets, blocks, n_blocks, labels_len,
                                          data_len, ignore_label, hist_lo, hist_hi, flags, CTG_MEM_DEVICE, stream, r);
            wide.reset();   // stream-ordered, as the dense labels
            return rc;
        },
        out);
}

// ---------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------
extern "C" {

int ctg_rag_features(const void* labels, int label_bits, const void* data, int data_kind, int n_channels,
                     const int32_t* offsets, const int64_t* shape, const int64_t* own_begin,
                     const int64_t* own_end, int ignore_label,
                     double hist_lo, double hist_hi, int flags, int mem, void* stream, ctg_result** out) {
    const char* who = "ctg_rag_features";
    ApiCall c;
    int rc = validate_features(labels, label_bits, data, data_kind, n_channels, offsets, shape, own_begin, own_end,
                               hist_lo, hist_hi, out);
    if (rc || (rc = c.begin(stream)) != CTG_OK) return rc;
    Workspace& w = c.w();
    hipStream_t s = c.s;
    const int64_t V = shape[0] * shape[1] * shape[2];
    const size_t dbytes = data ? (size_t)V * (n_channels > 0 ? n_channels : 1) * (data_kind == CTG_DATA_U8 ? 1 : 4) : 0;
    const void *dl = nullptr, *dd = nullptr;
    if ((rc = stage_volumes(w, labels, (size_t)V * (label_bits / 8), data, dbytes, mem, s, &dl, &dd)) != CTG_OK) return rc;
    const bool boundary_map = data && n_channels == 0;
    const ScanSwitches sw = scan_switches(true, boundary_map);

    ScanParams P;
    const ChannelClass cc = scan_common(P, dl, dd, label_bits, data_kind, n_channels, offsets, hist_lo, hist_hi);
    plan_whole_tiles(P, shape, own_begin, own_end, sw);
    if ((rc = density_probe(w, P, narrow_rows_mode(boundary_map, V, sw.narrow_rows), s)) != CTG_OK) return rc;
    AdjFilter adj{s};
    if (cc.long_range && !(flags & CTG_NO_ADJ_FILTER) && V > 0 &&
        (rc = adjacency_filter(P, shape, own_begin, own_end, hist_lo, hist_hi, stream, adj)) != CTG_OK)
        return rc;
    plan_scan_channels(P, cc, flags, sw);

    Ev ev{w, s};
    ev.mark(0);
    if (V == 0) return c.empty(empty_result, out);
    RegionPrefix pre{};
    bool overflow = false;
    if ((rc = scan_records(w, P, V, s, sw, ev, pre, &overflow, who)) != CTG_OK) return rc;
    if (overflow)
        return features_dense_reentry(dl, label_bits, dd, data_kind, n_channels, offsets, shape, own_begin, own_end,
                                      ignore_label, hist_lo, hist_hi, flags, stream, out);
    c.r = new_result(c.dev);
    ReduceJob J = scan_job(w, P, pre, true, ignore_label, flags, c.r.get());
    J.need_adj = need_adj_whole(P.n_channels, P.skip_adj_marks, !(flags & CTG_NO_ADJ_FILTER), P.bloom != nullptr);
    J.defer_stats = (flags & CTG_DEFER_STATS) ? 1 : 0;
    J.min_u = w.counters_host->max_nu ? (uint64_t)(uint32_t)~(uint32_t)w.counters_host->max_nu : 0;
    const int64_t single = single_label_index(P);
    J.single_label_ptr = label_bits == 64 && single >= 0 ? (const uint64_t*)dl + single : nullptr;
    hipError_t e = reduce_records(w, J, s, c.r.get());
    if (e == hipSuccess) e = widen_single_label(P, single, s, c.r.get());
    if ((rc = hip_status(e, who, CTG_ERR_HIP)) != CTG_OK) return rc;
    c.r->partial_adj = J.need_adj == 2 ? 1 : 0;
    return c.end(true, out);
}

// batched per-block sub-graphs / features (the ndist per-block calls)
int ctg_rag_blocks(const void* labels, int label_bits, const void* data, int data_kind, int n_channels,
                   const int32_t* offsets, const ctg_block_desc* blocks, int n_blocks, int64_t labels_len,
                   int64_t data_len, int ignore_label, double hist_lo, double hist_hi, int flags, int mem,
                   void* stream, ctg_result** out) {
    const char* who = "ctg_rag_blocks";
    ApiCall c;
    if (!out || !labels || !blocks || n_blocks < 1 || n_blocks > (1 << 20) || labels_len < 0 ||
        (label_bits != 32 && label_bits != 64) || (data && data_kind != CTG_DATA_F32 && data_kind != CTG_DATA_U8) ||
        n_channels < 0 || n_channels > CTG_MAX_CHANNELS || (n_channels > 0 && !offsets) || !(hist_hi > hist_lo)) {
        set_error("ctg_rag_blocks: bad arguments");
        return CTG_ERR_ARG;
    }
    *out = nullptr;
    const ScanSwitches sw = scan_switches(false, false);
    // plan tiles (a block outside its array or the arena is refused before
    // any GPU work, too many tiles after the staging, as ever)
    const BlockPlan plan = plan_blocks(blocks, n_blocks, data != nullptr, n_channels, labels_len, data_len,
                                       scan_max_x(), scan_tile_rows(), unique_tile_y(), sw.tile_z);
    if (plan.error == BlockPlan::BOX_OUTSIDE || plan.error == BlockPlan::ARRAY_OUTSIDE) return block_plan_error(plan);
    int rc = c.begin(stream);
    if (rc) return rc;
    Workspace& w = c.w();
    hipStream_t s = c.s;
    const void *dl = nullptr, *dd = nullptr;
    if ((rc = stage_volumes(w, labels, (size_t)labels_len * (label_bits / 8), data,
                            data ? (size_t)data_len * (data_kind == CTG_DATA_U8 ? 1 : 4) : 0, mem, s, &dl, &dd)) != CTG_OK)
        return rc;
    if (plan.error != BlockPlan::OK) return block_plan_error(plan);

    ScanParams P;
    scan_common(P, dl, dd, label_bits, data_kind, n_channels, offsets, hist_lo, hist_hi);
    BlockTables tables{s};
    if ((rc = upload_block_tables(plan, n_blocks, s, tables, P)) != CTG_OK) return rc;

    Ev ev{w, s};
    ev.mark(0);
    RegionPrefix pre{};
    bool overflow = false;
    const bool scanned = P.batch_tiles > 0;
    if (!scanned) w.last_scan = ScanReport{};   // (ctg_last_scan: no launch)
    if (scanned && (rc = scan_records(w, P, plan.voxels, s, sw, ev, pre, &overflow, who)) != CTG_OK) return rc;
    if (overflow)
        return blocks_dense_reentry(dl, label_bits, dd, data_kind, n_channels, offsets, blocks, n_blocks, labels_len,
                                    data_len, ignore_label, hist_lo, hist_hi, flags, P.tag_shift, stream, out);
    c.r = new_result(c.dev);
    ctg_result* r = c.r.get();
    ReduceJob J = scan_job(w, P, pre, scanned, ignore_label, flags, r);
    J.need_adj = need_adj_blocks(P.n_channels);
    J.ub = plan.tag_bits ? 32 : 0;
    J.umask = plan.tag_bits ? (1ull << P.tag_shift) - 1ull : ~0ull;
    J.skip_nodes = 1;
    hipError_t e = reduce_records(w, J, s, r);
    if (e == hipSuccess) e = block_edge_offsets(P, plan.tag_bits, J.umask, s, r);
    if ((rc = hip_status(e, who, CTG_ERR_HIP)) != CTG_OK) return rc;
    if (flags & CTG_NO_NODES) r->node_off.assign(n_blocks + 1, 0);
    else if ((rc = block_nodes(w, P, plan, s, r)) != CTG_OK) return rc;
    // same phase split as ctg_rag_features ([5] = reduce end -> nodes)
    return c.end(scanned, out);
}

}  // extern "C"
