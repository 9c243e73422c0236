// C ABI of libctg.so (include/ctg.h): the entry points -- host orchestration
// of the face scan and the result handles.  The allocator and the workspace
// live in ctg_workspace.hip (ctg_pool.h, ctg_buffers.h), the record back half
// in ctg_records.hip, the host decisions in ctg_plan.h.
#include <hip/hip_runtime.h>
#include <cstdlib>
#include <cstring>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_select.hpp>

#include <algorithm>
#include <cstdio>

#include "ctg_internal.h"

namespace ctg {

static thread_local std::string g_err;
void set_error(const std::string& msg) { g_err = msg; }

ResultPtr new_result(int device) {
    ResultPtr r(new ctg_result());
    r->device = device;
    return r;
}

ResultPtr empty_result(int device) {
    ResultPtr r = new_result(device);
    r->edges = (uint64_t*)dev_alloc(16);
    r->nodes = (uint64_t*)dev_alloc(8);
    return r;
}

CTG_BOUNDS_TAKE(api)

}  // namespace ctg

using namespace ctg;

// a nested C-ABI call's handle, owned
template <class Call>
static int nested(ResultPtr& r, Call&& call) {
    ctg_result* raw = nullptr;
    const int rc = call(&raw);
    r.reset(raw);
    return rc;
}

static int stage_in(GrowBuf& stage, const void* src, size_t bytes, int mem, hipStream_t s, const void** dev) {
    if (mem == CTG_MEM_DEVICE || src == nullptr) {
        *dev = src;
        return CTG_OK;
    }
    if (!stage.reserve(bytes)) {
        set_error("out of device memory staging input");
        return CTG_ERR_NOMEM;
    }
    CTG_CHECK(hipMemcpyAsync(stage.p, src, bytes, hipMemcpyHostToDevice, s));
    *dev = stage.p;
    return CTG_OK;
}

// An input of the merge / unique / map entry points on the device: the
// caller's pointer where mem says device, else a copy that lives as long as
// this (the two volume slots go through stage_in).
template <class T>
struct DevInput {
    DevBuf<T> own;
    const T* p = nullptr;
    int put(const T* src, size_t bytes, int mem, hipStream_t s, const char* who) {
        p = src;
        if (mem != CTG_MEM_HOST) return CTG_OK;
        if (!(p = own.alloc(std::max<size_t>(bytes, 1)))) {
            set_error(std::string(who) + ": out of device memory");
            return CTG_ERR_NOMEM;
        }
        if (bytes) CTG_CHECK(hipMemcpyAsync(own, src, bytes, hipMemcpyHostToDevice, s));
        return CTG_OK;
    }
    operator const T*() const { return p; }
};

// A dense output table that may live on the host: kernels write d, which is
// the caller's pointer (mem device) or a device buffer of this object's, copied
// out by copy_back().  An absent table (null, or no bytes) has d null.
template <class T>
struct DenseOut {
    DevBuf<T> own;
    T* d = nullptr;
    T* dst = nullptr;
    size_t bytes = 0;
    hipError_t open(T* out, size_t nbytes, int mem, bool zero, hipStream_t s) {
        if (!out || nbytes == 0) return hipSuccess;
        dst = out;
        bytes = nbytes;
        d = mem == CTG_MEM_HOST ? own.alloc(bytes) : out;
        if (!d) return hipErrorOutOfMemory;
        return zero ? hipMemsetAsync(d, 0, bytes, s) : hipSuccess;
    }
    hipError_t copy_back(hipStream_t s) {
        return own ? hipMemcpyAsync(dst, d, bytes, hipMemcpyDeviceToHost, s) : hipSuccess;
    }
};

// n u64 values -> their sorted distinct values in out (room for n), the count
// in *count_dev (device); key bits [0, end_bit) are compared
static hipError_t sort_unique_u64(Workspace& w, const uint64_t* in, int64_t n, uint64_t* out, uint32_t* count_dev,
                                  hipStream_t s, unsigned end_bit = 64u) {
    DevBuf<uint64_t> sorted(std::max<int64_t>(n, 1) * 8);
    if (!sorted) return hipErrorOutOfMemory;
    hipError_t e = with_temp(w.temp, [&](void* t, size_t& tb) {
        return rocprim::radix_sort_keys(t, tb, in, (uint64_t*)sorted, (size_t)n, 0u, end_bit, s);
    });
    if (e != hipSuccess) return e;
    return with_temp(w.temp, [&](void* t, size_t& tb) {
        return rocprim::unique(t, tb, (uint64_t*)sorted, out, count_dev, (size_t)n, rocprim::equal_to<uint64_t>(), s);
    });
}

// one u32 device word, after everything queued on s
static int read_word(Workspace& w, SmallSlot i, hipStream_t s, int64_t* v) {
    CTG_CHECK(hipMemcpyAsync(w.small_host + i, w.small + i, 4, hipMemcpyDeviceToHost, s));
    CTG_CHECK(hipStreamSynchronize(s));
    *v = w.small_host[i];
    return CTG_OK;
}

// the phase times of a profiled call: scan, pack, sort, segment, reduce, nodes, total
static int read_phase_times(Workspace& w, hipStream_t s) {
    CTG_CHECK(hipStreamSynchronize(s));
    float ms = 0.f;
    for (int i = 0; i < 6; ++i) {
        hipEventElapsedTime(&ms, w.ev[i], w.ev[i + 1]);
        w.last_ms[i] = ms;
    }
    hipEventElapsedTime(&ms, w.ev[0], w.ev[6]);
    w.last_ms[6] = ms;
    return CTG_OK;
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

// dense edge ends and nodes of r -> the labels of the sorted unique table U
static hipError_t map_back(const ctg_result* U, ctg_result* r, hipStream_t s) {
    hipError_t e = launch_gather_labels(U->nodes, r->edges, 2 * r->n_edges, s);
    if (e == hipSuccess) e = launch_gather_labels(U->nodes, r->nodes, r->n_nodes, s);
    return e;
}

// Labels that do not fit the face keys' u / v fields -- >= 2^32 for a whole
// array (the keys pack (u,v) as 32+32 bits), >= 2^tag_shift for
// batched blocks: the n labels are relabelled densely through their sorted
// unique labels (a monotone map: sorted dense tables stay sorted after mapping
// back), `rerun` makes the call again on the 32-bit dense labels, and the edge
// and node tables are mapped back.  shape: a whole array (its unique labels
// come from the tile pass), or null.  At most `limit` distinct labels.
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

// (u,v) pair lists with labels >= 2^32 (merge / union inputs): the sort packs
// (u,v) into one 64-bit key, so the endpoints are replaced by their rank in
// the sorted unique endpoint table (monotone) and mapped back afterwards.
struct DensePairs {
    ResultPtr U;
    DevBuf<uint64_t> dense;
    int build(const uint64_t* dk, int64_t n, hipStream_t s) {
        int rc = nested(U, [&](ctg_result** u) { return ctg_unique_values(dk, 2 * n, CTG_MEM_DEVICE, s, u); });
        if (rc) return rc;
        if (!dense.alloc((size_t)n * 16)) {
            set_error("out of device memory for the dense endpoint relabelling");
            return CTG_ERR_NOMEM;
        }
        CTG_CHECK(launch_remap_dense64(dk, 2 * n, U->nodes, U->n_nodes, dense, s));
        return CTG_OK;
    }
    hipError_t map_back(ctg_result* r, hipStream_t s) { return U ? ::map_back(U.get(), r, s) : hipSuccess; }
};

// The body of the pair-list entry points (ctg_merge_stats, ctg_unique_pairs):
// J describes the call but for the J.n (u,v) pairs dk, which are relabelled
// densely where a label reaches 2^32.
static int reduce_pairs(Workspace& w, ReduceJob& J, const uint64_t* dk, hipStream_t s, const char* who,
                        ctg_result** out) {
    CTG_CHECK(hipMemsetAsync(w.counters, 0, sizeof(Counters), s));
    CTG_CHECK(launch_max_pairs(J.n, dk, &w.counters->max_v, s));
    CTG_CHECK(hipMemcpyAsync(w.counters_host, w.counters, sizeof(Counters), hipMemcpyDeviceToHost, s));
    CTG_CHECK(hipStreamSynchronize(s));
    DensePairs dp;
    J.pairs = dk;
    J.max_v = w.counters_host->max_v;
    if (J.max_v >> 32) {
        const int rc = dp.build(dk, J.n, s);
        if (rc) return rc;
        J.pairs = dp.dense;
        J.max_v = (uint64_t)std::max<int64_t>(dp.U->n_nodes - 1, 0);
    }
    ResultPtr r = new_result(current_device());
    hipError_t e = reduce_records(w, J, s, r.get());
    if (e == hipSuccess) e = dp.map_back(r.get(), s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) {
        set_error(std::string(who) + ": " + hipGetErrorString(e));
        return CTG_ERR_HIP;
    }
    *out = r.release();
    return CTG_OK;
}

// ---------------------------------------------------------------------------
// the face scan
// ---------------------------------------------------------------------------
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

// One face scan with its record bookkeeping: the record buffer grows and the
// scan re-runs when a region overflowed.  *overflow = labels that do not fit
// the key's u / v fields (the caller relabels densely).
static int scan_records(Workspace& w, const ScanParams& P, int64_t V, hipStream_t s, Ev& ev, RegionPrefix& pre,
                        bool* overflow, const char* who) {
    *overflow = false;
    if (getenv("CTG_REC_FRESH")) {   // test hook: start from the smallest record buffer
        CTG_CHECK(hipStreamSynchronize(s));
        free_records(w);
    }
    int64_t need = std::max<int64_t>(w.rec.cap, std::max<int64_t>(1 << 16, V / 24));
    need = (need + NREG - 1) / NREG * NREG;
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
        CTG_CHECK(launch_face_scan(PW, w.rec, w.counters, s));
        ev.mark(1);
        CTG_CHECK(hipMemcpyAsync(w.counters_host, w.counters, sizeof(Counters), hipMemcpyDeviceToHost, s));
        CTG_CHECK(hipStreamSynchronize(s));
        if (w.counters_host->label_overflow) {
            *overflow = true;
            return CTG_OK;
        }
        unsigned long long tot = 0, mx = 0;
        for (int r = 0; r < NREG; ++r) {
            pre.off[r] = (uint32_t)tot;
            tot += w.counters_host->rcount[r];
            mx = std::max(mx, w.counters_host->rcount[r]);
        }
        pre.off[NREG] = (uint32_t)tot;
        w.counters_host->n_records = tot;
        if (tot >= (1ull << 32)) {
            set_error(std::string(who) + ": more than 2^32 records");
            return CTG_ERR_NOMEM;
        }
        if ((int64_t)mx <= w.rec.rcap) break;
        need = ((int64_t)(mx * 5 / 4) + 1024) * NREG;
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

static int bits_u(int64_t v) { return v <= 0 ? 0 : bits_for((uint64_t)v); }

// the per-block nodes of a batched call: unique labels of every own box
static int block_nodes(Workspace& w, const void* dl, int label_bits, const BlockGeom* dgeom, int n_blocks,
                       const std::vector<uint32_t>& uprefix, int64_t own_voxels, hipStream_t s, ctg_result* r) {
    const int64_t n_tiles = uprefix.back();
    DevBuf<uint32_t> dprefix((n_blocks + 1) * 4);
    DevBuf<int64_t> bounds((n_blocks + 1) * 8);
    if (dprefix) CTG_CHECK(hipMemcpyAsync(dprefix, uprefix.data(), (n_blocks + 1) * 4, hipMemcpyHostToDevice, s));
    int64_t cap = std::max<int64_t>(1, std::min<int64_t>(own_voxels, std::max<int64_t>(1 << 16, own_voxels / 8)));
    for (int attempt = 0; attempt < 3; ++attempt) {
        DevBuf<uint64_t> cand(cap * 8), nodes(cap * 8);
        if (!dprefix || !bounds || !cand || !nodes) {
            set_error("ctg_rag_blocks: out of device memory for the block nodes");
            return CTG_ERR_NOMEM;
        }
        CTG_CHECK(hipMemsetAsync(w.counters, 0, sizeof(Counters), s));
        CTG_CHECK(launch_unique_blocks(dl, label_bits, dgeom, dprefix, n_blocks, n_tiles, cand,
                                       &w.counters->n_records, cap, s));
        CTG_CHECK(hipMemcpyAsync(w.counters_host, w.counters, sizeof(Counters), hipMemcpyDeviceToHost, s));
        CTG_CHECK(hipStreamSynchronize(s));
        const int64_t m = (int64_t)w.counters_host->n_records;
        if (m > cap) {
            cap = m + 1024;
            continue;
        }
        int64_t N = 0;
        CTG_CHECK(sort_unique_u64(w, cand, m, nodes, w.small + SLOT_NODES, s, 32u + (unsigned)bits_u(n_blocks - 1)));
        if (int rc = read_word(w, SLOT_NODES, s, &N)) return rc;
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
    set_error("ctg_rag_blocks: node candidate buffer overflow");
    return CTG_ERR_NOMEM;
}

// ---------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------
extern "C" {

int ctg_version(void) { return 1; }

const char* ctg_last_error(void) { return g_err.c_str(); }

int ctg_mgpu_slab(int64_t Z, int world_size, int rank, const int64_t* offsets, int n_channels, int64_t* out) {
    if (Z <= 0 || world_size <= 0 || rank < 0 || rank >= world_size || !out || n_channels < 0 ||
        (n_channels > 0 && !offsets)) {
        set_error("ctg_mgpu_slab: invalid arguments");
        return CTG_ERR_ARG;
    }
    if (world_size > Z) {
        set_error("ctg_mgpu_slab: more ranks than z planes");
        return CTG_ERR_ARG;
    }
    int64_t down = 1, up = 0;   // planes a face / partner reaches below and above a voxel
    for (int c = 0; c < n_channels; ++c) {
        down = std::max<int64_t>(down, -offsets[3 * c]);
        up = std::max<int64_t>(up, offsets[3 * c]);
    }
    if (up > 0 && world_size > 1) {
        set_error("ctg_mgpu_slab: positive z offsets need an upper halo, which the z-slab layout does not have");
        return CTG_ERR_UNSUPPORTED;
    }
    const int64_t z0 = Z * rank / world_size, z1 = Z * (rank + 1) / world_size;
    out[0] = z0 - std::min(down, z0);
    out[1] = z0;
    out[2] = z1;
    return CTG_OK;
}

static bool mgpu_args(const ctg_result* r, int world, const char* who) {
    if (!r || world <= 0 || world > CTG_MGPU_MAX_WORLD) {
        set_error(std::string(who) + ": bad arguments (world size must be 1.." +
                  std::to_string(CTG_MGPU_MAX_WORLD) + ")");
        return false;
    }
    return true;
}

int ctg_mgpu_sample(const ctg_result* local, int64_t* meta, void* stream) {
    DevLock dev_lock;
    if (!mgpu_args(local, 1, "ctg_mgpu_sample") || !meta) return CTG_ERR_ARG;
    CTG_CHECK(mgpu_sample(local->edges, local->n_edges, meta, (hipStream_t)stream));
    return CTG_OK;
}

int ctg_mgpu_split(const ctg_result* local, const int64_t* meta_all, int world_size, int64_t* counts, void* stream) {
    DevLock dev_lock;
    if (!mgpu_args(local, world_size, "ctg_mgpu_split") || !meta_all || !counts) return CTG_ERR_ARG;
    Workspace& w = ws(current_device());
    CTG_CHECK(ws_init(w));
    // one splitter buffer per device: a split on another stream must not
    // overwrite it while an earlier split's k_mgpu_bounds still reads it
    if (w.mgpu_spl_ev) CTG_CHECK(hipStreamWaitEvent((hipStream_t)stream, w.mgpu_spl_ev, 0));
    else CTG_CHECK(hipEventCreateWithFlags(&w.mgpu_spl_ev, hipEventDisableTiming));
    CTG_CHECK(mgpu_split(local->edges, local->n_edges, local->nodes, local->n_nodes, meta_all, world_size,
                         w.mgpu_spl, counts, (hipStream_t)stream));
    CTG_CHECK(hipEventRecord(w.mgpu_spl_ev, (hipStream_t)stream));
    return CTG_OK;
}

int ctg_mgpu_pack(const ctg_result* local, const int64_t* counts_all, int world_size, int rank, int64_t* send,
                  void* stream) {
    DevLock dev_lock;
    if (!mgpu_args(local, world_size, "ctg_mgpu_pack") || !counts_all || rank < 0 || rank >= world_size)
        return CTG_ERR_ARG;
    const int64_t* mine = counts_all + (int64_t)rank * world_size * 2;
    int64_t rows = 0, nodes = 0, words = 0;
    for (int d = 0; d < world_size; ++d) {
        rows += mine[2 * d];
        nodes += mine[2 * d + 1];
        if (d != rank) words += mine[2 * d] * CTG_MGPU_ROW_WORDS + mine[2 * d + 1];
    }
    if (rows != local->n_edges || nodes != local->n_nodes) {
        set_error("ctg_mgpu_pack: counts do not cover this rank's table");
        return CTG_ERR_ARG;
    }
    if (words > 0 && (!send || (!(local->stats && local->stat_sums) && !local->defer.on))) {
        set_error("ctg_mgpu_pack: rows to send need a CTG_KEEP_STATS table and a send buffer");
        return CTG_ERR_ARG;
    }
    if (words > 0 && local->defer.on && local->defer.gen != ws(local->device).gen) {
        set_error("ctg_mgpu_pack: the CTG_DEFER_STATS table's records were overwritten by a later call");
        return CTG_ERR_STALE;
    }
    CTG_CHECK(mgpu_pack(local, counts_all, world_size, rank, send, (hipStream_t)stream));
    return CTG_OK;
}

int ctg_mgpu_merge(ctg_result* local, const int64_t* recv, const int64_t* counts_all, int world_size, int rank,
                   double hist_lo, double hist_hi, void* stream, ctg_result** out) {
    DevLock dev_lock;
    if (!mgpu_args(local, world_size, "ctg_mgpu_merge") || !counts_all || !out || rank < 0 || rank >= world_size ||
        !(hist_hi > hist_lo))
        return CTG_ERR_ARG;
    *out = nullptr;
    if (!local->owned.empty()) {   // a shard's arrays are interior pointers of its owned blocks
        set_error("ctg_mgpu_merge: the local table is itself a merge shard; pass the rank's local call");
        return CTG_ERR_ARG;
    }
    int64_t rows = 0, nodes = 0, recv_words = 0;
    for (int d = 0; d < world_size; ++d) {
        rows += counts_all[((int64_t)rank * world_size + d) * 2];
        nodes += counts_all[((int64_t)rank * world_size + d) * 2 + 1];
        if (d != rank)
            recv_words += counts_all[((int64_t)d * world_size + rank) * 2] * CTG_MGPU_ROW_WORDS +
                          counts_all[((int64_t)d * world_size + rank) * 2 + 1];
    }
    if (rows != local->n_edges || nodes != local->n_nodes) {
        set_error("ctg_mgpu_merge: counts do not cover this rank's table");
        return CTG_ERR_ARG;
    }
    if (recv_words > 0 && !recv) {
        set_error("ctg_mgpu_merge: null receive buffer");
        return CTG_ERR_ARG;
    }
    if (recv_words > 0 && local->defer.on && local->defer.gen != ws(local->device).gen) {
        set_error("ctg_mgpu_merge: the CTG_DEFER_STATS table's records were overwritten by a later call");
        return CTG_ERR_STALE;
    }
    Workspace& w = ws(current_device());
    CTG_CHECK(ws_init(w));
    ResultPtr r = new_result(current_device());
    int lib_rc = CTG_OK;
    const hipError_t e = mgpu_merge(local, recv, counts_all, world_size, rank, hist_lo, hist_hi,
                                    (hipStream_t)stream, r.get(), &lib_rc);
    if (lib_rc != CTG_OK) return lib_rc;   // the message is set already
    if (e != hipSuccess) {
        set_error(std::string("ctg_mgpu_merge: ") + hipGetErrorString(e));
        return e == hipErrorOutOfMemory ? CTG_ERR_NOMEM : CTG_ERR_HIP;
    }
    local->n_edges = 0;
    local->n_nodes = 0;
    *out = r.release();
    return CTG_OK;
}

int ctg_device_count(int* count) {
    CTG_CHECK(hipGetDeviceCount(count));
    return CTG_OK;
}

int ctg_init(int device) {
    int n = 0;
    std::lock_guard<std::recursive_mutex> init_lock(device_mutex(device));
    CTG_CHECK(hipGetDeviceCount(&n));
    if (device < 0 || device >= n) {
        set_error("ctg_init: invalid device " + std::to_string(device));
        return CTG_ERR_ARG;
    }
    CTG_CHECK(hipSetDevice(device));
    CTG_CHECK(ws_init(ws(device)));
    return CTG_OK;
}

int ctg_diag_bounds(uint64_t* out) {
#ifdef CTG_DIAG
    if (!out) return CTG_ERR_ARG;
    CTG_CHECK(hipDeviceSynchronize());
    hipError_t (*take[7])(unsigned long long*) = {bounds_take_api,    bounds_take_scan, bounds_take_sort,
                                                   bounds_take_reduce, bounds_take_mgpu, bounds_take_overlap,
                                                   bounds_take_morph};
    out[0] = out[1] = out[2] = out[3] = 0;
    int found = 0;
    for (int f = 0; f < 7; ++f) {
        unsigned long long h[3] = {0, 0, 0};
        CTG_CHECK(take[f](h));
        if (h[0] && !found) {
            out[0] = (uint64_t)f + 1;   // 1 api, 2 scan, 3 sort, 4 reduce, 5 mgpu, 6 overlap, 7 morph
            out[1] = h[0];
            out[2] = h[1];
            out[3] = h[2];
            found = 1;
        }
    }
    return found;
#else
    (void)out;
    set_error("ctg_diag_bounds: bounds checks exist only in CTG_DIAG builds (make variant EXTRA=-DCTG_DIAG)");
    return CTG_ERR_UNSUPPORTED;
#endif
}

int ctg_set_profiling(int on) {
    ws(current_device()).profiling = on;
    return CTG_OK;
}

int ctg_last_timings(double* ms, int n) {
    Workspace& w = ws(current_device());
    for (int i = 0; i < n && i < 8; ++i) ms[i] = w.last_ms[i];
    return CTG_OK;
}

int ctg_rag_features(const void* labels, int label_bits, const void* data, int data_kind, int n_channels,
                     const int32_t* offsets, const int64_t* shape, const int64_t* own_begin,
                     const int64_t* own_end, int ignore_label,
                     double hist_lo, double hist_hi, int flags, int mem, void* stream, ctg_result** out) {
    DevLock dev_lock;
    if (!out || !shape || !labels) {
        set_error("ctg_rag_features: null argument");
        return CTG_ERR_ARG;
    }
    *out = nullptr;
    if (label_bits != 32 && label_bits != 64) {
        set_error("ctg_rag_features: label_bits must be 32 or 64");
        return CTG_ERR_ARG;
    }
    if (n_channels < 0 || n_channels > CTG_MAX_CHANNELS || (n_channels > 0 && !offsets)) {
        set_error("ctg_rag_features: bad channel/offset arguments");
        return CTG_ERR_ARG;
    }
    if (data && data_kind != CTG_DATA_F32 && data_kind != CTG_DATA_U8) {
        set_error("ctg_rag_features: data_kind must be CTG_DATA_F32 or CTG_DATA_U8");
        return CTG_ERR_ARG;
    }
    if (!(hist_hi > hist_lo)) {
        set_error("ctg_rag_features: hist_hi must be > hist_lo");
        return CTG_ERR_ARG;
    }
    for (int k = 0; k < 3; ++k)
        if (shape[k] < 0 || (own_begin && (own_begin[k] < 0)) || (own_end && own_end[k] < 0)) {
            set_error("ctg_rag_features: negative shape/own_begin/own_end");
            return CTG_ERR_ARG;
        }
    const int dev = current_device();
    Workspace& w = ws(dev);
    CTG_CHECK(ws_init(w));
    hipStream_t s = (hipStream_t)stream;
    const int64_t V = shape[0] * shape[1] * shape[2];
    const size_t lbytes = (size_t)V * (label_bits / 8);
    const size_t dbytes = data ? (size_t)V * (n_channels > 0 ? n_channels : 1) * (data_kind == CTG_DATA_U8 ? 1 : 4) : 0;
    const void* dl = nullptr;
    const void* dd = nullptr;
    int rc = stage_in(w.stage[0], labels, lbytes, mem, s, &dl);
    if (rc) return rc;
    rc = stage_in(w.stage[1], data, dbytes, mem, s, &dd);
    if (rc) return rc;

    ScanParams P;
    const ChannelClass cc = scan_common(P, dl, dd, label_bits, data_kind, n_channels, offsets, hist_lo, hist_hi);
    for (int k = 0; k < 3; ++k) {
        P.shape[k] = shape[k];
        P.own_begin[k] = own_begin ? own_begin[k] : 0;
        P.own_end[k] = own_end ? std::min(own_end[k], shape[k]) : shape[k];
    }
    {
        const TileDepths td = scan_tile_depths(shape, scan_tile_rows(), scan_tile_rows_narrow());
        P.tile_z = td.tile_z;
        P.tile_z_narrow = td.tile_z_narrow;
        if (const char* t = getenv("CTG_TILE_Z")) P.tile_z_narrow = P.tile_z = std::max(1, atoi(t));   // tests
        if (const char* t = getenv("CTG_TILE_Z_NARROW")) P.tile_z_narrow = std::max(1, atoi(t));   // A/B
    }
#ifdef CTG_DIAG   // scan ablations (variant builds only)
    {
        const char* ab = getenv("CTG_ABLATE");
        P.ablate = ab ? atoi(ab) : 0;
    }
#endif
    P.tail_tiles = !(getenv("CTG_TAIL_TILES") && getenv("CTG_TAIL_TILES")[0] == '0');   // (ctg_scan.hip)
    // boundary maps of fragmented volumes (configs[4]: cell 5) scan with
    // 1-row waves: the sampled x-face density decides on the device (cell 10
    // ~ 0.10, cell 5 ~ 0.20 changes per pair; threshold 0.14), without a host
    // round trip.  The probe and the second launch cost ~0.1 ms, so volumes
    // below 2^28 voxels (~645^3, steps of ~2 ms) keep the wide tiles.
    // CTG_NARROW_ROWS=0/1 forces a width.
    if (data && n_channels == 0 && (V >= (1ll << 28) || getenv("CTG_NARROW_ROWS"))) {
        const char* nr = getenv("CTG_NARROW_ROWS");
        if (nr) {
            P.narrow_rows = atoi(nr) ? 1 : 0;
        } else {
            P.density = w.small + SLOT_DENSITY;
            CTG_CHECK(hipMemsetAsync(w.small + SLOT_DENSITY, 0, 2 * sizeof(uint32_t), s));
            CTG_CHECK(launch_density(dl, label_bits, shape, 512, w.small + SLOT_DENSITY, s));
            P.narrow_rows = 2;
        }
    }

    // Long-range affinity channels: a sample counts only if its
    // (u,v) is a RAG edge.  Filtering in the scan (against the edge set of a
    // graph-only pass) keeps the non-adjacent pairs - most long-range pairs -
    // out of the edge tables and records.  Labels >= 2^32 skip it here: the
    // dense-relabel path re-enters with 32-bit labels and filters there.
    unsigned long long* bloom = nullptr;
    ctg_result* adj_graph = nullptr;
    struct AdjRelease {   // the set and its graph live until the scan is done
        unsigned long long*& set;
        ctg_result*& g;
        hipStream_t s;
        ~AdjRelease() {
            if (set) {
                hipStreamSynchronize(s);
                dev_free(set);
            }
            if (g) ctg_free(g);
        }
    } adj_release{bloom, adj_graph, s};

    if (cc.long_range && !(flags & CTG_NO_ADJ_FILTER) && V > 0) {
        rc = ctg_rag_features(dl, label_bits, nullptr, CTG_DATA_NONE, 0, nullptr, shape, own_begin, own_end, 0,
                              hist_lo, hist_hi, 0, CTG_MEM_DEVICE, stream, &adj_graph);
        if (rc) return rc;
        uint64_t mx = 0;
        if (adj_graph->n_edges > 0) {
            // largest label of the sorted edge table: the v of some row; the
            // max over all v equals the last node
            CTG_CHECK(hipMemcpyAsync(&mx, adj_graph->nodes + adj_graph->n_nodes - 1, 8, hipMemcpyDeviceToHost, s));
            CTG_CHECK(hipStreamSynchronize(s));
        }
        if ((mx >> 32) == 0) {
            // Bloom prefilter, 24 bits per stored direction (48 per edge; 32: +3 %
            // records, 12-channel scan +0.5 ms, profiles/r4/tz): one
            // load per long-range sample (vs. a probe chain in a set 4x the
            // size); the reduce drops its false positives (keys no
            // nearest-neighbour sample flagged)
            const int64_t bits = adj_graph->n_edges * 48;
            uint32_t blocks = 128;   // 64-B blocks
            while ((int64_t)blocks * 512 < bits) blocks *= 2;
            bloom = (unsigned long long*)dev_alloc((size_t)blocks * 64);
            if (!bloom) {
                set_error("ctg_rag_features: out of memory (adjacency filter)");
                return CTG_ERR_NOMEM;
            }
            hipError_t e = launch_build_bloom(adj_graph->edges, adj_graph->n_edges, bloom, blocks - 1, s);
            if (e != hipSuccess) {
                set_error(std::string("ctg_rag_features: ") + hipGetErrorString(e));
                return CTG_ERR_HIP;
            }
            P.bloom = bloom;
            P.bloom_mask = blocks - 1;
        }
    }
    {
        const char* sa = getenv("CTG_SKIP_ADJ");
        const char* nn = getenv("CTG_NN3");   // CTG_NN3=0 keeps the channel loop
        const ChannelPlan cp = plan_channels(cc, P.n_channels, !(flags & CTG_NO_ADJ_FILTER), P.bloom != nullptr,
                                             !sa || atoi(sa), !(nn && nn[0] == '0'));
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

    Ev ev{w, s};
    ev.mark(0);
    if (V == 0) {
        *out = empty_result(dev).release();
        return CTG_OK;
    }
    RegionPrefix pre{};
    const bool stats = P.data_kind != CTG_DATA_NONE;
    bool overflow = false;
    rc = scan_records(w, P, V, s, ev, pre, &overflow, "ctg_rag_features");
    if (rc) return rc;
    if (overflow) {
        if (label_bits != 64) {
            set_error("ctg_rag_features: internal label overflow on 32-bit labels");
            return CTG_ERR_HIP;
        }
        return rag_dense_relabel(
            (const uint64_t*)dl, V, shape, ignore_label, 0xFFFFFFFFll, "ctg_rag_features",
            ": more than 2^32 distinct labels in one array", stream,
            [&](const uint32_t* dense, ctg_result** r) {
                return ctg_rag_features(dense, 32, dd, data_kind, n_channels, offsets, shape, own_begin, own_end,
                                        ignore_label, hist_lo, hist_hi, flags, CTG_MEM_DEVICE, stream, r);
            },
            out);
    }
    const int64_t n = (int64_t)w.counters_host->n_records;

    ResultPtr r = new_result(dev);
    r->n_records = n;
    r->n_direct = w.last_direct;
    ReduceJob J{};
    J.n = n;
    J.keys = w.rec.key;
    J.regions = &pre;
    J.R = w.rec;
    J.wide = 0;
    J.stats = stats;
    J.need_adj = P.n_channels > 0 && !P.skip_adj_marks ? ((flags & CTG_NO_ADJ_FILTER) ? 2 : 1) : 0;
    if (P.bloom) J.need_adj = 1;   // drop the Bloom filter's false positives
    J.ignore_label = ignore_label;
    J.keep_stats = (flags & CTG_KEEP_STATS) ? 1 : 0;
    J.defer_stats = (flags & CTG_DEFER_STATS) ? 1 : 0;
    J.max_v = w.counters_host->max_v;
    J.min_u = w.counters_host->max_nu ? (uint64_t)(uint32_t)~(uint32_t)w.counters_host->max_nu : 0;
    J.scale = P.scale;
    J.offset = P.offset;
    // single-label array: the owned origin voxel is the only node
    const int64_t o0 = own_begin ? own_begin[0] : 0, o1 = own_begin ? own_begin[1] : 0,
                  o2 = own_begin ? own_begin[2] : 0;
    const bool has_owned = o0 < P.own_end[0] && o1 < P.own_end[1] && o2 < P.own_end[2];
    J.single_label_ptr = (label_bits == 64 && has_owned)
                             ? (const uint64_t*)dl + ((o0 * shape[1] + o1) * shape[2] + o2)
                             : nullptr;
    hipError_t e = reduce_records(w, J, s, r.get());
    if (e == hipSuccess && label_bits == 32 && r->n_records == 0 && has_owned) {
        // 32-bit labels: widen the single label
        uint32_t l32 = 0;
        e = hipMemcpyAsync(&l32, (const uint32_t*)dl + ((o0 * shape[1] + o1) * shape[2] + o2), 4,
                           hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        uint64_t l64 = l32;
        if (e == hipSuccess) e = hipMemcpy(r->nodes, &l64, 8, hipMemcpyHostToDevice);
        r->n_nodes = 1;
    }
    if (e != hipSuccess) {
        set_error(std::string("ctg_rag_features: ") + hipGetErrorString(e));
        return CTG_ERR_HIP;
    }
    if (w.profiling && (rc = read_phase_times(w, s)) != CTG_OK) return rc;
    r->partial_adj = J.need_adj == 2 ? 1 : 0;
    *out = r.release();
    return CTG_OK;
}

// ---------------------------------------------------------------------------
// batched per-block sub-graphs / features (the ndist per-block calls)
// ---------------------------------------------------------------------------
int ctg_rag_blocks(const void* labels, int label_bits, const void* data, int data_kind, int n_channels,
                   const int32_t* offsets, const ctg_block_desc* blocks, int n_blocks, int64_t labels_len,
                   int64_t data_len, int ignore_label, double hist_lo, double hist_hi, int flags, int mem,
                   void* stream, ctg_result** out) {
    DevLock dev_lock;
    if (!out || !labels || !blocks || n_blocks < 1 || n_blocks > (1 << 20) || labels_len < 0 ||
        (label_bits != 32 && label_bits != 64) || (data && data_kind != CTG_DATA_F32 && data_kind != CTG_DATA_U8) ||
        n_channels < 0 || n_channels > CTG_MAX_CHANNELS || (n_channels > 0 && !offsets) || !(hist_hi > hist_lo)) {
        set_error("ctg_rag_blocks: bad arguments");
        return CTG_ERR_ARG;
    }
    *out = nullptr;
    const int nch = data ? std::max(1, n_channels) : 0;
    int64_t own_voxels = 0, voxels = 0, zmax = 1;
    for (int b = 0; b < n_blocks; ++b) {
        const ctg_block_desc& d = blocks[b];
        int64_t V = 1;
        for (int k = 0; k < 3; ++k) {
            V *= d.shape[k];
            if (d.shape[k] < 0 || d.shape[k] > (k == 2 ? scan_max_x() : 0x7FFFFFFF) || d.own_begin[k] < 0 ||
                d.own_end[k] > d.shape[k] ||
                d.graph_begin[k] < 0 || d.graph_end[k] > d.shape[k]) {
                set_error("ctg_rag_blocks: block " + std::to_string(b) + ": box outside its array");
                return CTG_ERR_ARG;
            }
        }
        if (d.label_offset < 0 || d.label_offset + V > labels_len ||
            (data && (d.data_offset < 0 || d.data_offset + V * nch > data_len))) {
            set_error("ctg_rag_blocks: block " + std::to_string(b) + ": array outside the arena");
            return CTG_ERR_ARG;
        }
        int64_t ov = 1;
        for (int k = 0; k < 3; ++k) ov *= std::max<int64_t>(0, d.own_end[k] - d.own_begin[k]);
        own_voxels += ov;
        voxels += V;
        zmax = std::max(zmax, d.shape[0]);
    }
    const int dev = current_device();
    Workspace& w = ws(dev);
    CTG_CHECK(ws_init(w));
    hipStream_t s = (hipStream_t)stream;
    const void* dl = nullptr;
    const void* dd = nullptr;
    int rc = stage_in(w.stage[0], labels, (size_t)labels_len * (label_bits / 8), mem, s, &dl);
    if (rc) return rc;
    rc = stage_in(w.stage[1], data, data ? (size_t)data_len * (data_kind == CTG_DATA_U8 ? 1 : 4) : 0, mem, s, &dd);
    if (rc) return rc;

    ScanParams P;
    scan_common(P, dl, dd, label_bits, data_kind, n_channels, offsets, hist_lo, hist_hi);
    P.tile_z = (int)std::min<int64_t>(zmax, 128);   // one tile deep for the usual <= 128-plane blocks
    if (const char* t = getenv("CTG_TILE_Z")) P.tile_z = std::max(1, atoi(t));
    const int tag_bits = bits_u(n_blocks - 1);
    P.tag_shift = 32 - tag_bits;
    P.label_hi_mask = tag_bits ? ~((1u << P.tag_shift) - 1u) : 0u;
    P.n_blocks = n_blocks;
    // per-block geometry and the tile prefixes of the scan / node launches
    const int rows = scan_tile_rows(), uty = unique_tile_y();
    std::vector<BlockGeom> geom(n_blocks);
    std::vector<uint32_t> prefix(n_blocks + 1, 0), uprefix(n_blocks + 1, 0);
    for (int b = 0; b < n_blocks; ++b) {
        const ctg_block_desc& d = blocks[b];
        BlockGeom& g = geom[b];
        g.label_offset = d.label_offset;
        g.data_offset = data ? d.data_offset : 0;
        for (int k = 0; k < 3; ++k) {
            g.shape[k] = (int32_t)d.shape[k];
            g.own_begin[k] = (int32_t)d.own_begin[k];
            g.own_end[k] = (int32_t)d.own_end[k];
            g.graph_begin[k] = (int32_t)d.graph_begin[k];
            g.graph_end[k] = (int32_t)d.graph_end[k];
        }
        g.ntx = (int32_t)((d.shape[2] + TILE_X - 1) / TILE_X);
        g.nty = (int32_t)((d.shape[1] + rows - 1) / rows);
        g.ntz = (int32_t)((d.shape[0] + P.tile_z - 1) / P.tile_z);
        const int64_t nt = (int64_t)g.ntx * g.nty * g.ntz;
        int64_t ut = 1;
        const int64_t oe[3] = {std::max<int64_t>(0, d.own_end[0] - d.own_begin[0]),
                               std::max<int64_t>(0, d.own_end[1] - d.own_begin[1]),
                               std::max<int64_t>(0, d.own_end[2] - d.own_begin[2])};
        ut = ((oe[2] + 63) / 64) * ((oe[1] + uty - 1) / uty) * ((oe[0] + 15) / 16);
        if ((int64_t)prefix[b] + nt > 0x7FFFFFFFll || (int64_t)uprefix[b] + ut > 0x7FFFFFFFll) {
            set_error("ctg_rag_blocks: too many tiles in one call");
            return CTG_ERR_ARG;
        }
        prefix[b + 1] = prefix[b] + (uint32_t)nt;
        uprefix[b + 1] = uprefix[b] + (uint32_t)ut;
    }
    P.batch_tiles = prefix[n_blocks];
    BlockGeom* dgeom = (BlockGeom*)dev_alloc(sizeof(BlockGeom) * n_blocks);
    uint32_t* dprefix = (uint32_t*)dev_alloc((n_blocks + 1) * 4);
    struct Release {   // the scan and the node pass read them until the call is done
        BlockGeom* g;
        uint32_t* p;
        hipStream_t s;
        ~Release() {
            hipStreamSynchronize(s);
            dev_free(g);
            dev_free(p);
        }
    } release{dgeom, dprefix, s};
    if (!dgeom || !dprefix) {
        set_error("ctg_rag_blocks: out of device memory");
        return CTG_ERR_NOMEM;
    }
    CTG_CHECK(hipMemcpyAsync(dgeom, geom.data(), sizeof(BlockGeom) * n_blocks, hipMemcpyHostToDevice, s));
    CTG_CHECK(hipMemcpyAsync(dprefix, prefix.data(), (n_blocks + 1) * 4, hipMemcpyHostToDevice, s));
    P.blocks = dgeom;
    P.tile_prefix = dprefix;

    Ev ev{w, s};
    ev.mark(0);
    RegionPrefix pre{};
    bool overflow = false;
    rc = P.batch_tiles ? scan_records(w, P, voxels, s, ev, pre, &overflow, "ctg_rag_blocks") : CTG_OK;
    if (rc) return rc;
    if (overflow) {
        // labels too large for the tagged keys: relabel the arena densely
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
            l64, labels_len, nullptr, ignore_label, (int64_t)(1ull << P.tag_shift), "ctg_rag_blocks",
            ": too many distinct labels for one batch of blocks: call with fewer blocks", stream,
            [&](const uint32_t* dense, ctg_result** r) {
                const int rc_ = ctg_rag_blocks(dense, 32, dd, data_kind, n_channels, offsets, blocks, n_blocks,
                                               labels_len, data_len, ignore_label, hist_lo, hist_hi, flags,
                                               CTG_MEM_DEVICE, stream, r);
                wide.reset();   // stream-ordered, as the dense labels
                return rc_;
            },
            out);
    }
    const int64_t n = P.batch_tiles ? (int64_t)w.counters_host->n_records : 0;
    ResultPtr r = new_result(dev);
    r->n_records = n;
    r->n_direct = P.batch_tiles ? (int64_t)w.counters_host->n_direct : 0;
    ReduceJob J{};
    J.n = n;
    J.keys = w.rec.key;
    J.regions = &pre;
    J.R = w.rec;
    J.stats = P.data_kind != CTG_DATA_NONE;
    // boundary / graph: every key is a face of the block's graph box;
    // affinities: keep the keys of the block's sub-graph (ADJ marks)
    J.need_adj = P.n_channels > 0 ? 1 : 0;
    J.ignore_label = ignore_label;
    J.keep_stats = (flags & CTG_KEEP_STATS) ? 1 : 0;
    J.max_v = P.batch_tiles ? w.counters_host->max_v : 0;
    J.scale = P.scale;
    J.offset = P.offset;
    J.ub = tag_bits ? 32 : 0;
    J.umask = tag_bits ? (1ull << P.tag_shift) - 1ull : ~0ull;
    J.skip_nodes = 1;
    hipError_t e = reduce_records(w, J, s, r.get());
    if (e == hipSuccess) {
        r->edge_off.assign(n_blocks + 1, 0);
        r->edge_off[n_blocks] = r->n_edges;
        if (tag_bits && r->n_edges) {
            DevBuf<int64_t> bounds((n_blocks + 1) * 8);
            e = bounds ? launch_block_bounds(r->n_edges, r->edges, 2, n_blocks, P.tag_shift, bounds, s)
                       : hipErrorOutOfMemory;
            if (e == hipSuccess)
                e = hipMemcpyAsync(r->edge_off.data(), bounds, (n_blocks + 1) * 8, hipMemcpyDeviceToHost, s);
            if (e == hipSuccess) e = launch_clear_bits(r->n_edges, r->edges, 2, J.umask, s);
            if (e == hipSuccess) e = hipStreamSynchronize(s);
        }
    }
    if (e != hipSuccess) {
        set_error(std::string("ctg_rag_blocks: ") + hipGetErrorString(e));
        return CTG_ERR_HIP;
    }
    if (flags & CTG_NO_NODES) r->node_off.assign(n_blocks + 1, 0);
    else rc = block_nodes(w, dl, label_bits, dgeom, n_blocks, uprefix, own_voxels, s, r.get());
    if (rc) return rc;
    // same phase split as ctg_rag_features ([5] = reduce end -> nodes)
    if (w.profiling && P.batch_tiles && (rc = read_phase_times(w, s)) != CTG_OK) return rc;
    r->partial_adj = J.need_adj == 2 ? 1 : 0;
    *out = r.release();
    return CTG_OK;
}

int ctg_result_num_blocks(const ctg_result* r) { return r ? (int)std::max<size_t>(r->edge_off.size(), 1) - 1 : -1; }

int ctg_result_block_offsets(const ctg_result* r, int64_t* edge_off, int64_t* node_off) {
    if (!r || r->edge_off.empty()) {
        set_error("ctg_result_block_offsets: not a batched-blocks result");
        return CTG_ERR_ARG;
    }
    const size_t nb = r->edge_off.size();
    if (edge_off) std::memcpy(edge_off, r->edge_off.data(), nb * 8);
    if (node_off) {
        if (r->node_off.size() == nb) std::memcpy(node_off, r->node_off.data(), nb * 8);
        else std::memset(node_off, 0, nb * 8);
    }
    return CTG_OK;
}

int ctg_unique_labels(const uint64_t* labels, const int64_t* shape, const int64_t* begin, const int64_t* end,
                      int mem, void* stream, ctg_result** out) {
    DevLock dev_lock;
    if (!labels || !shape || !out) {
        set_error("ctg_unique_labels: null argument");
        return CTG_ERR_ARG;
    }
    *out = nullptr;
    int64_t b[3], e[3];
    for (int k = 0; k < 3; ++k) {
        b[k] = begin ? begin[k] : 0;
        e[k] = end ? end[k] : shape[k];
        if (b[k] < 0 || e[k] > shape[k] || b[k] > e[k]) {
            set_error("ctg_unique_labels: box outside the array");
            return CTG_ERR_ARG;
        }
    }
    const int dev = current_device();
    Workspace& w = ws(dev);
    CTG_CHECK(ws_init(w));
    hipStream_t s = (hipStream_t)stream;
    const int64_t V = shape[0] * shape[1] * shape[2];
    const void* dl = nullptr;
    int rc = stage_in(w.stage[0], labels, (size_t)V * 8, mem, s, &dl);
    if (rc) return rc;
    const int64_t nb = (e[0] - b[0]) * (e[1] - b[1]) * (e[2] - b[2]);
    if (nb == 0) {
        *out = empty_result(dev).release();
        return CTG_OK;
    }
    ResultPtr r = new_result(dev);
    int64_t cap = std::min<int64_t>(nb, std::max<int64_t>(1 << 16, nb / 8));
    for (int attempt = 0; attempt < 3; ++attempt) {
        DevBuf<uint64_t> cand(cap * 8), nodes(cap * 8);
        if (!cand || !nodes) {
            set_error("ctg_unique_labels: out of device memory");
            return CTG_ERR_NOMEM;
        }
        CTG_CHECK(hipMemsetAsync(w.counters, 0, sizeof(Counters), s));
        CTG_CHECK(launch_unique_tiles((const uint64_t*)dl, shape, b, e, cand, &w.counters->n_records, cap, s));
        CTG_CHECK(hipMemcpyAsync(w.counters_host, w.counters, sizeof(Counters), hipMemcpyDeviceToHost, s));
        CTG_CHECK(hipStreamSynchronize(s));
        const int64_t m = (int64_t)w.counters_host->n_records;
        if (m > cap) {
            cap = std::min<int64_t>(nb, m + 1024);
            continue;
        }
        CTG_CHECK(sort_unique_u64(w, cand, m, nodes, w.small + SLOT_NODES, s));
        if ((rc = read_word(w, SLOT_NODES, s, &r->n_nodes)) != CTG_OK) return rc;
        r->nodes = nodes.release();
        r->edges = (uint64_t*)dev_alloc(16);
        *out = r.release();
        return CTG_OK;
    }
    set_error("ctg_unique_labels: candidate buffer overflow");
    return CTG_ERR_NOMEM;
}

int ctg_unique_values(const uint64_t* values, int64_t n, int mem, void* stream, ctg_result** out) {
    DevLock dev_lock;
    if (!out || n < 0 || (n > 0 && !values)) {
        set_error("ctg_unique_values: bad arguments");
        return CTG_ERR_ARG;
    }
    *out = nullptr;
    const int dev = current_device();
    Workspace& w = ws(dev);
    CTG_CHECK(ws_init(w));
    hipStream_t s = (hipStream_t)stream;
    if (n == 0) {
        *out = empty_result(dev).release();
        return CTG_OK;
    }
    ResultPtr r = new_result(dev);
    r->edges = (uint64_t*)dev_alloc(16);
    r->nodes = (uint64_t*)dev_alloc(n * 8);
    if (!r->nodes) {
        set_error("ctg_unique_values: out of device memory");
        return CTG_ERR_NOMEM;
    }
    DevInput<uint64_t> in;
    int rc = in.put(values, (size_t)n * 8, mem, s, "ctg_unique_values");
    if (rc) return rc;
    CTG_CHECK(sort_unique_u64(w, in, n, r->nodes, w.small + SLOT_NODES, s));
    if ((rc = read_word(w, SLOT_NODES, s, &r->n_nodes)) != CTG_OK) return rc;
    *out = r.release();
    return CTG_OK;
}

int ctg_merge_stats(const uint64_t* keys, const double* sums, const uint32_t* records, int64_t n, double hist_lo,
                    double hist_hi, int keep_stats, int mem, void* stream, ctg_result** out) {
    DevLock dev_lock;
    if (!out || n < 0 || (n > 0 && (!keys || !sums || !records))) {
        set_error("ctg_merge_stats: bad arguments");
        return CTG_ERR_ARG;
    }
    *out = nullptr;
    const int dev = current_device();
    Workspace& w = ws(dev);
    CTG_CHECK(ws_init(w));
    hipStream_t s = (hipStream_t)stream;
    if (n == 0) {
        *out = empty_result(dev).release();
        return CTG_OK;
    }
    // inputs to device (merge buffers are separate from the scan records)
    DevInput<uint64_t> dk;
    DevInput<double> ds;
    DevInput<uint32_t> dr;
    int rc = dk.put(keys, (size_t)n * 16, mem, s, "ctg_merge_stats");
    if (!rc) rc = ds.put(sums, (size_t)n * 16, mem, s, "ctg_merge_stats");
    if (!rc) rc = dr.put(records, (size_t)n * WREC_WORDS * 4, mem, s, "ctg_merge_stats");
    if (rc) return rc;
    ReduceJob J{};
    J.n = n;
    J.R.key = nullptr;
    J.R.sums = (double2*)ds.p;
    J.R.hist = (uint32_t*)dr.p;
    J.R.cap = n;
    J.wide = 1;
    J.stats = 1;
    J.need_adj = 1;
    J.ignore_label = 0;
    J.keep_stats = keep_stats;
    J.scale = (double)NBINS / (hist_hi - hist_lo);
    J.offset = hist_lo;
    return reduce_pairs(w, J, dk, s, "ctg_merge_stats", out);
}

int ctg_merge_feature_rows(const uint64_t* ids, const double* rows, int64_t n, int64_t id_begin, int64_t id_end,
                           double* out, int mem, void* stream) {
    DevLock dev_lock;
    if (n < 0 || id_end < id_begin || (n > 0 && (!ids || !rows)) || (id_end > id_begin && !out)) {
        set_error("ctg_merge_feature_rows: bad arguments");
        return CTG_ERR_ARG;
    }
    if (id_end - id_begin > 0xFFFFFFFFll || n > 0xFFFFFFFFll) {
        set_error("ctg_merge_feature_rows: more than 2^32 edges or rows in one call");
        return CTG_ERR_UNSUPPORTED;
    }
    const int64_t E = id_end - id_begin;
    if (E == 0) return CTG_OK;
    const int dev = current_device();
    Workspace& w = ws(dev);
    CTG_CHECK(ws_init(w));
    hipStream_t s = (hipStream_t)stream;
    const bool host = mem == CTG_MEM_HOST;
    DevInput<uint64_t> di;
    DevInput<double> dr;
    DevBuf<double> own_o;
    double* dout = out;
    int rc = di.put(ids, (size_t)n * 8, mem, s, "ctg_merge_feature_rows");
    if (!rc) rc = dr.put(rows, (size_t)n * N_FEATURES * 8, mem, s, "ctg_merge_feature_rows");
    if (rc) return rc;
    if (host && !(dout = own_o.alloc(E * N_FEATURES * 8))) {
        set_error("ctg_merge_feature_rows: out of device memory");
        return CTG_ERR_NOMEM;
    }
    CTG_CHECK(hipMemsetAsync(dout, 0, E * N_FEATURES * 8, s));
    if (n) {
        DevBuf<uint32_t> k_in(n * 4), k_out(n * 4), i_in(n * 4), i_out(n * 4);
        if (!k_in || !k_out || !i_in || !i_out) {
            set_error("ctg_merge_feature_rows: out of device memory");
            return CTG_ERR_NOMEM;
        }
        CTG_CHECK(hipMemsetAsync(w.small + SLOT_BAD_ID, 0, 4, s));
        CTG_CHECK(launch_row_keys(n, di, (uint64_t)id_begin, (uint64_t)id_end, k_in, i_in, w.small + SLOT_BAD_ID, s));
        const unsigned kb = (unsigned)bits_for((uint64_t)std::max<int64_t>(E - 1, 1));
        CTG_CHECK(with_temp(w.temp, [&](void* t, size_t& tb) {
            return rocprim::radix_sort_pairs(t, tb, k_in.p, k_out.p, i_in.p, i_out.p, (size_t)n, 0u, kb, s);
        }));
        CTG_CHECK(launch_merge_feature_rows(n, k_out, i_out, dr, dout, s));
        CTG_CHECK(hipMemcpyAsync(w.small_host + SLOT_BAD_ID, w.small + SLOT_BAD_ID, 4, hipMemcpyDeviceToHost, s));
    }
    if (host) CTG_CHECK(hipMemcpyAsync(out, dout, E * N_FEATURES * 8, hipMemcpyDeviceToHost, s));
    CTG_CHECK(hipStreamSynchronize(s));
    if (n && w.small_host[SLOT_BAD_ID]) {
        set_error("ctg_merge_feature_rows: an edge id lies outside [id_begin, id_end)");
        return CTG_ERR_ARG;
    }
    return CTG_OK;
}

int ctg_unique_pairs(const uint64_t* pairs, int64_t n, int mem, void* stream, ctg_result** out) {
    DevLock dev_lock;
    if (!out || n < 0 || (n > 0 && !pairs)) {
        set_error("ctg_unique_pairs: bad arguments");
        return CTG_ERR_ARG;
    }
    *out = nullptr;
    const int dev = current_device();
    Workspace& w = ws(dev);
    CTG_CHECK(ws_init(w));
    hipStream_t s = (hipStream_t)stream;
    if (n == 0) {
        *out = empty_result(dev).release();
        return CTG_OK;
    }
    DevInput<uint64_t> dk;
    int rc = dk.put(pairs, (size_t)n * 16, mem, s, "ctg_unique_pairs");
    if (rc) return rc;
    ReduceJob J{};
    J.n = n;
    J.stats = 0;
    J.need_adj = 0;
    J.scale = 1.0;
    J.offset = 0.0;
    return reduce_pairs(w, J, dk, s, "ctg_unique_pairs", out);
}

// ---------------------------------------------------------------------------
// label overlaps and segment morphology (kernels and back halves:
// ctg_overlap.hip, ctg_morph.hip).  What the entry points share comes first.
// ---------------------------------------------------------------------------
static int hip_status(hipError_t e, const char* who) {
    if (e == hipSuccess) return CTG_OK;
    set_error(std::string(who) + ": " + hipGetErrorString(e));
    return e == hipErrorOutOfMemory ? CTG_ERR_NOMEM : CTG_ERR_HIP;
}

// the box [b, e) of a call: begin / end default to the whole array, the box
// lies inside it and holds *nb < 2^32 - 1 voxels
static int box_of(const char* who, const int64_t* shape, const int64_t* begin, const int64_t* end, int64_t* b,
                  int64_t* e, int64_t* nb) {
    for (int k = 0; k < 3; ++k) {
        b[k] = begin ? begin[k] : 0;
        e[k] = end ? end[k] : shape[k];
        if (shape[k] < 0 || b[k] < 0 || e[k] > shape[k] || b[k] > e[k]) {
            set_error(std::string(who) + ": box outside the array");
            return CTG_ERR_ARG;
        }
    }
    *nb = (e[0] - b[0]) * (e[1] - b[1]) * (e[2] - b[2]);
    if (*nb >= 0xFFFFFFFFll) {   // (a record per voxel at most; the run table numbers records in 32 bits)
        set_error(std::string(who) + ": boxes of 2^32 voxels or more are not supported");
        return CTG_ERR_UNSUPPORTED;
    }
    return CTG_OK;
}

// an overlaps / a morphology result without rows: the placeholders of
// empty_result plus the counts' / the moments'
static ResultPtr empty_overlaps(int device) {
    ResultPtr r = empty_result(device);
    r->counts = (uint64_t*)dev_alloc(8);
    return r;
}
static ResultPtr empty_morphology(int device) {
    ResultPtr r = empty_result(device);
    r->moments = (uint64_t*)dev_alloc(8);
    return r;
}

// A table call on the current device: its initialised workspace, its stream
// and its result, which starts as `empty` makes it.  begin(), the work, then
// end() -- or, with nothing to do, hand r out as it is.
struct TableCall {
    Workspace* wp = nullptr;
    hipStream_t s = nullptr;
    ResultPtr r;
    int begin(void* stream, ResultPtr (*empty)(int)) {
        const int dev = current_device();
        Workspace& w = ws(dev);
        CTG_CHECK(ws_init(w));
        wp = &w;
        s = (hipStream_t)stream;
        r = empty(dev);
        return CTG_OK;
    }
    // a scan's epilogue: the phase times of a profiled call (timed: it ran the phases), the workspace's record counts
    int end(bool timed, ctg_result** out) {
        Workspace& w = *wp;
        if (w.profiling && timed) {
            const int rc = read_phase_times(w, s);
            if (rc != CTG_OK) return rc;
        }
        CTG_CHECK(hipStreamSynchronize(s));
        w.last_records = r->n_records;
        w.last_direct = r->n_direct;
        *out = r.release();
        return CTG_OK;
    }
};

// A label volume of ctg_label_overlaps / ctg_morphology whose labels reach
// 2^32: the box's sorted unique labels U and the whole array as 32-bit ranks in
// U (monotone; voxels outside the box get some rank and are never read).
struct DenseSide {
    ResultPtr U;
    DevBuf<uint32_t> ids;
    int build(const void* vol, const int64_t* shape, const int64_t* b, const int64_t* e, void* stream,
              const char* who) {
        int rc = nested(U, [&](ctg_result** u) {
            return ctg_unique_labels((const uint64_t*)vol, shape, b, e, CTG_MEM_DEVICE, stream, u);
        });
        if (rc) return rc;
        if (U->n_nodes > 0xFFFFFFFFll) {
            set_error(std::string(who) + ": more than 2^32 distinct labels in one box");
            return CTG_ERR_UNSUPPORTED;
        }
        const int64_t V = shape[0] * shape[1] * shape[2];
        if (!ids.alloc((size_t)V * 4)) {
            set_error(std::string(who) + ": out of device memory for the dense relabelling");
            return CTG_ERR_NOMEM;
        }
        CTG_CHECK(launch_remap_dense((const uint64_t*)vol, V, U->nodes, U->n_nodes, ids, (hipStream_t)stream));
        return CTG_OK;
    }
};

int ctg_label_overlaps(const void* labels, int label_bits, const void* values, int value_bits, const int64_t* shape,
                       const int64_t* begin, const int64_t* end, int with_ignore, uint64_t ignore_label, int mem,
                       void* stream, ctg_result** out) {
    const char* who = "ctg_label_overlaps";
    DevLock dev_lock;
    if (!labels || !values || !shape || !out) {
        set_error("ctg_label_overlaps: null argument");
        return CTG_ERR_ARG;
    }
    *out = nullptr;
    if ((label_bits != 32 && label_bits != 64) || (value_bits != 32 && value_bits != 64)) {
        set_error("ctg_label_overlaps: label_bits and value_bits must be 32 or 64");
        return CTG_ERR_ARG;
    }
    int64_t b[3], e[3], nb = 0;
    int rc = box_of(who, shape, begin, end, b, e, &nb);
    if (rc) return rc;
    TableCall c;
    if ((rc = c.begin(stream, empty_overlaps)) != CTG_OK) return rc;
    if (nb == 0) {
        *out = c.r.release();
        return CTG_OK;
    }
    Workspace& w = *c.wp;
    hipStream_t s = c.s;
    ctg_result* r = c.r.get();
    const int64_t V = shape[0] * shape[1] * shape[2];
    const void *dl = nullptr, *dv = nullptr;
    rc = stage_in(w.stage[0], labels, (size_t)V * (label_bits / 8), mem, s, &dl);
    if (!rc) rc = stage_in(w.stage[1], values, (size_t)V * (value_bits / 8), mem, s, &dv);
    if (rc) return rc;
    unsigned over = 0;
    if ((rc = hip_status(overlap_tables(w, dl, label_bits, dv, value_bits, shape, b, e, with_ignore, ignore_label, s,
                                        r, &over),
                         who)) != CTG_OK)
        return rc;
    if (over) {
        // labels >= 2^32 do not fit the 32 + 32 bit keys.  1: the side(s) that
        // hold them become monotone dense ids
        DenseSide da, db;
        if ((over & 1u) && (rc = da.build(dl, shape, b, e, stream, who)) != CTG_OK) return rc;
        if ((over & 2u) && (rc = db.build(dv, shape, b, e, stream, who)) != CTG_OK) return rc;
        // 2: so does the ignore label (absent from the box: nothing to skip)
        if ((over & 2u) && with_ignore) {
            DevBuf<uint32_t> rank(4);
            uint32_t h = 0;
            if (!rank) return hip_status(hipErrorOutOfMemory, who);
            CTG_CHECK(launch_overlap_find(db.U->nodes, db.U->n_nodes, ignore_label, rank, s));
            CTG_CHECK(hipMemcpyAsync(&h, rank.p, 4, hipMemcpyDeviceToHost, s));
            CTG_CHECK(hipStreamSynchronize(s));
            with_ignore = h != 0xFFFFFFFFu;
            ignore_label = h;
        }
        // 3: the scan runs again on the ids
        unsigned again = 0;
        if ((rc = hip_status(overlap_tables(w, da.U ? (const void*)da.ids.p : dl, da.U ? 32 : label_bits,
                                            db.U ? (const void*)db.ids.p : dv, db.U ? 32 : value_bits, shape, b, e,
                                            with_ignore, ignore_label, s, r, &again),
                             who)) != CTG_OK)
            return rc;
        // 4: which cannot overflow
        if (again) {
            set_error("ctg_label_overlaps: dense ids past 2^32");
            return CTG_ERR_UNSUPPORTED;
        }
        // 5: the sorted tables map back to labels
        CTG_CHECK(launch_overlap_map_back(r->n_edges, r->edges, da.U ? da.U->nodes : nullptr,
                                          da.U ? da.U->n_nodes : 0, db.U ? db.U->nodes : nullptr,
                                          db.U ? db.U->n_nodes : 0, s));
        if (da.U) CTG_CHECK(launch_gather_labels(da.U->nodes, r->nodes, r->n_nodes, s));
    }
    return c.end(r->n_records > 0, out);
}

int ctg_merge_overlaps(const uint64_t* pairs, const uint64_t* counts, int64_t n, int mem, void* stream,
                       ctg_result** out) {
    DevLock dev_lock;
    if (!out || n < 0 || (n > 0 && (!pairs || !counts))) {
        set_error("ctg_merge_overlaps: bad arguments");
        return CTG_ERR_ARG;
    }
    *out = nullptr;
    if (n >= 0xFFFFFFFFll) {
        set_error("ctg_merge_overlaps: 2^32 rows or more in one call");
        return CTG_ERR_UNSUPPORTED;
    }
    TableCall c;
    int rc = c.begin(stream, empty_overlaps);
    if (rc) return rc;
    if (n == 0) {
        *out = c.r.release();
        return CTG_OK;
    }
    Workspace& w = *c.wp;
    hipStream_t s = c.s;
    ResultPtr& r = c.r;
    DevInput<uint64_t> dp, dc;
    rc = dp.put(pairs, (size_t)n * 16, mem, s, "ctg_merge_overlaps");
    if (!rc) rc = dc.put(counts, (size_t)n * 8, mem, s, "ctg_merge_overlaps");
    if (rc) return rc;
    CTG_CHECK(hipMemsetAsync(w.counters, 0, sizeof(Counters), s));
    CTG_CHECK(launch_max_pairs(n, dp, &w.counters->max_v, s));
    CTG_CHECK(hipMemcpyAsync(w.counters_host, w.counters, sizeof(Counters), hipMemcpyDeviceToHost, s));
    CTG_CHECK(hipStreamSynchronize(s));
    DensePairs dense;
    const uint64_t* src = dp;
    if (w.counters_host->max_v >> 32) {
        if ((rc = dense.build(dp, n, s)) != CTG_OK) return rc;
        if (dense.U->n_nodes > 0xFFFFFFFFll) {
            set_error("ctg_merge_overlaps: more than 2^32 distinct labels");
            return CTG_ERR_UNSUPPORTED;
        }
        src = dense.dense;
    }
    DevBuf<uint64_t> key((size_t)n * 8);
    if (!key) return hip_status(hipErrorOutOfMemory, "ctg_merge_overlaps");
    CTG_CHECK(launch_overlap_pack(n, src, key, s));
    if ((rc = hip_status(overlap_reduce(w, key, dc, n, s, r.get()), "ctg_merge_overlaps")) != CTG_OK) return rc;
    CTG_CHECK(dense.map_back(r.get(), s));
    CTG_CHECK(hipStreamSynchronize(s));
    r->n_records = n;
    *out = r.release();
    return CTG_OK;
}

int ctg_max_overlaps(const ctg_result* r, uint64_t label_begin, uint64_t label_end, uint64_t* out_labels,
                     uint64_t* out_counts, int mem, void* stream) {
    DevLock dev_lock;
    if (!r || label_end < label_begin || (label_end > label_begin && !out_labels)) {
        set_error("ctg_max_overlaps: bad arguments");
        return CTG_ERR_ARG;
    }
    if (!r->counts || (r->n_nodes > 0 && !r->row_off)) {
        set_error("ctg_max_overlaps: not an overlaps result (ctg_label_overlaps, ctg_merge_overlaps)");
        return CTG_ERR_ARG;
    }
    const uint64_t n = label_end - label_begin;
    if (n == 0) return CTG_OK;
    hipStream_t s = (hipStream_t)stream;
    DenseOut<uint64_t> ol, oc;
    int rc = hip_status(ol.open(out_labels, n * 8, mem, true, s), "ctg_max_overlaps");
    if (!rc) rc = hip_status(oc.open(out_counts, n * 8, mem, true, s), "ctg_max_overlaps");
    if (rc) return rc;
    CTG_CHECK(launch_overlap_argmax(r, label_begin, label_end, ol.d, oc.d, s));
    CTG_CHECK(ol.copy_back(s));
    CTG_CHECK(oc.copy_back(s));
    CTG_CHECK(hipStreamSynchronize(s));
    return CTG_OK;
}

int ctg_morphology(const void* labels, int label_bits, const int64_t* shape, const int64_t* begin, const int64_t* end,
                   const int64_t* origin, int mem, void* stream, ctg_result** out) {
    const char* who = "ctg_morphology";
    DevLock dev_lock;
    if (!labels || !shape || !out) {
        set_error("ctg_morphology: null argument");
        return CTG_ERR_ARG;
    }
    *out = nullptr;
    if (label_bits != 32 && label_bits != 64) {
        set_error("ctg_morphology: label_bits must be 32 or 64");
        return CTG_ERR_ARG;
    }
    int64_t b[3], e[3], o[3], nb = 0;
    int rc = box_of(who, shape, begin, end, b, e, &nb);
    if (rc) return rc;
    for (int k = 0; k < 3; ++k) {
        o[k] = origin ? origin[k] : 0;
        // a coordinate below 2^31 and fewer than 2^32 voxels: no sum reaches 2^63
        if (o[k] < 0 || o[k] >= (1ll << 31) || o[k] + e[k] >= (1ll << 31)) {
            set_error("ctg_morphology: origin + end must stay below 2^31 on every axis (origin >= 0)");
            return CTG_ERR_ARG;
        }
    }
    TableCall c;
    if ((rc = c.begin(stream, empty_morphology)) != CTG_OK) return rc;
    if (nb == 0) {
        *out = c.r.release();
        return CTG_OK;
    }
    Workspace& w = *c.wp;
    hipStream_t s = c.s;
    ctg_result* r = c.r.get();
    const int64_t V = shape[0] * shape[1] * shape[2];
    const void* dl = nullptr;
    if ((rc = stage_in(w.stage[0], labels, (size_t)V * (label_bits / 8), mem, s, &dl)) != CTG_OK) return rc;
    unsigned over = 0;
    if ((rc = hip_status(morph_tables(w, dl, label_bits, shape, b, e, o, s, r, &over), who)) != CTG_OK) return rc;
    if (over) {
        // labels >= 2^32 do not fit the table's 32-bit keys.  1: the labels
        // become monotone dense ids (2: no ignore label here)
        DenseSide d;
        if ((rc = d.build(dl, shape, b, e, stream, who)) != CTG_OK) return rc;
        // 3: the scan runs again on the ids
        unsigned again = 0;
        if ((rc = hip_status(morph_tables(w, d.ids.p, 32, shape, b, e, o, s, r, &again), who)) != CTG_OK) return rc;
        // 4: which cannot overflow
        if (again) {
            set_error("ctg_morphology: dense ids past 2^32");
            return CTG_ERR_UNSUPPORTED;
        }
        // 5: the sorted ids map back to labels
        CTG_CHECK(launch_gather_labels(d.U->nodes, r->nodes, r->n_nodes, s));
    }
    return c.end(true, out);
}

int ctg_merge_morphology(const double* rows, int64_t n, int mem, void* stream, ctg_result** out) {
    DevLock dev_lock;
    if (!out || n < 0 || (n > 0 && !rows)) {
        set_error("ctg_merge_morphology: bad arguments");
        return CTG_ERR_ARG;
    }
    *out = nullptr;
    if (n >= 0xFFFFFFFFll) {
        set_error("ctg_merge_morphology: 2^32 rows or more in one call");
        return CTG_ERR_UNSUPPORTED;
    }
    TableCall c;
    int rc = c.begin(stream, empty_morphology);
    if (rc) return rc;
    if (n == 0) {
        *out = c.r.release();
        return CTG_OK;
    }
    hipStream_t s = c.s;
    DevInput<double> dr;
    if ((rc = dr.put(rows, (size_t)n * CTG_MORPH_COLS * 8, mem, s, "ctg_merge_morphology")) != CTG_OK) return rc;
    int bad = 0;
    if ((rc = hip_status(morph_merge(*c.wp, dr, n, s, c.r.get(), &bad), "ctg_merge_morphology")) != CTG_OK) return rc;
    if (bad) {
        set_error("ctg_merge_morphology: a row's id is not an integer in [0, 2^53), or its size, centre or box is "
                  "negative or not finite");
        return CTG_ERR_ARG;
    }
    CTG_CHECK(hipStreamSynchronize(s));
    *out = c.r.release();
    return CTG_OK;
}

int ctg_morphology_rows(const ctg_result* r, uint64_t label_begin, uint64_t label_end, double* out, double* rows,
                        int mem, void* stream) {
    DevLock dev_lock;
    if (!r || label_end < label_begin) {
        set_error("ctg_morphology_rows: bad arguments");
        return CTG_ERR_ARG;
    }
    if (!r->moments) {
        set_error("ctg_morphology_rows: not a morphology result (ctg_morphology, ctg_merge_morphology)");
        return CTG_ERR_ARG;
    }
    hipStream_t s = (hipStream_t)stream;
    const int64_t N = r->n_nodes;
    if (N > 0) {   // the id column is a float64: the largest label (the last: nodes ascend) must fit it
        uint64_t top = 0;
        CTG_CHECK(hipMemcpyAsync(&top, r->nodes + (N - 1), 8, hipMemcpyDeviceToHost, s));
        CTG_CHECK(hipStreamSynchronize(s));
        if (top >= (1ull << 53)) {
            set_error("ctg_morphology_rows: a label of 2^53 or more does not fit the float64 id column "
                      "(ctg_result_copy_moments holds any label)");
            return CTG_ERR_UNSUPPORTED;
        }
    }
    const uint64_t n = label_end - label_begin;
    if (n > (1ull << 40)) {
        set_error("ctg_morphology_rows: label range too large");
        return CTG_ERR_ARG;
    }
    DenseOut<double> od, orw;
    int rc = hip_status(od.open(out, (size_t)n * CTG_MORPH_COLS * 8, mem, true, s), "ctg_morphology_rows");
    if (!rc) rc = hip_status(orw.open(rows, (size_t)N * CTG_MORPH_COLS * 8, mem, false, s), "ctg_morphology_rows");
    if (rc) return rc;
    if (!od.d && !orw.d) return CTG_OK;
    CTG_CHECK(launch_morph_rows(r, label_begin, label_end, od.d, orw.d, s));
    CTG_CHECK(od.copy_back(s));
    CTG_CHECK(orw.copy_back(s));
    CTG_CHECK(hipStreamSynchronize(s));
    return CTG_OK;
}

int ctg_map_edge_ids(const uint64_t* global_edges, int64_t n_global, const uint64_t* query, int64_t n_query,
                     int64_t* out_ids, int mem, void* stream) {
    DevLock dev_lock;
    if (n_global < 0 || n_query < 0 || (n_query > 0 && (!query || !out_ids))) {
        set_error("ctg_map_edge_ids: bad arguments");
        return CTG_ERR_ARG;
    }
    if (n_query == 0) return CTG_OK;
    hipStream_t s = (hipStream_t)stream;
    if (mem == CTG_MEM_DEVICE) {
        CTG_CHECK(launch_find_edges(global_edges, n_global, query, n_query, out_ids, s));
        return CTG_OK;
    }
    DevInput<uint64_t> g, q;
    DevBuf<int64_t> o(n_query * 8);
    int rc = g.put(global_edges, (size_t)n_global * 16, CTG_MEM_HOST, s, "ctg_map_edge_ids");
    if (!rc) rc = q.put(query, (size_t)n_query * 16, CTG_MEM_HOST, s, "ctg_map_edge_ids");
    if (rc) return rc;
    if (!o) {
        set_error("ctg_map_edge_ids: out of device memory");
        return CTG_ERR_NOMEM;
    }
    CTG_CHECK(launch_find_edges(g, n_global, q, n_query, o, s));
    CTG_CHECK(hipMemcpyAsync(out_ids, o, n_query * 8, hipMemcpyDeviceToHost, s));
    CTG_CHECK(hipStreamSynchronize(s));
    return CTG_OK;
}

int64_t ctg_result_num_edges(const ctg_result* r) { return r ? r->n_edges : -1; }
int64_t ctg_result_num_nodes(const ctg_result* r) { return r ? r->n_nodes : -1; }

static int copy_out(void* dst, const void* src, size_t bytes, int mem) {
    if (bytes == 0) return CTG_OK;
    if (!dst || !src) {
        set_error("copy: null pointer");
        return CTG_ERR_ARG;
    }
    CTG_CHECK(hipMemcpy(dst, src, bytes, mem == CTG_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost));
    return CTG_OK;
}

int ctg_result_copy_edges(const ctg_result* r, uint64_t* dst, int mem) {
    return copy_out(dst, r->edges, (size_t)r->n_edges * 16, mem);
}
int ctg_result_copy_nodes(const ctg_result* r, uint64_t* dst, int mem) {
    return copy_out(dst, r->nodes, (size_t)r->n_nodes * 8, mem);
}
int ctg_result_copy_features(const ctg_result* r, double* dst, int mem) {
    if (!r->features && r->n_edges) {
        set_error("result has no features (graph-only call)");
        return CTG_ERR_ARG;
    }
    return copy_out(dst, r->features, (size_t)r->n_edges * N_FEATURES * 8, mem);
}
int ctg_result_copy_stats(const ctg_result* r, double* sums_dst, uint32_t* records_dst, int mem) {
    if (!r->stats && r->n_edges) {
        set_error("result has no statistics (call with keep_stats=1 and data)");
        return CTG_ERR_ARG;
    }
    int rc = copy_out(sums_dst, r->stat_sums, (size_t)r->n_edges * 16, mem);
    if (rc) return rc;
    return copy_out(records_dst, r->stats, (size_t)r->n_edges * WREC_WORDS * 4, mem);
}
int ctg_result_copy_counts(const ctg_result* r, uint64_t* dst, int mem) {
    if (!r->counts) {
        set_error("result has no counts (not an overlaps result)");
        return CTG_ERR_ARG;
    }
    return copy_out(dst, r->counts, (size_t)r->n_edges * 8, mem);
}
int ctg_result_copy_moments(const ctg_result* r, uint64_t* dst, int mem) {
    if (!r || !r->moments) {
        set_error("result has no moments (not a morphology result)");
        return CTG_ERR_ARG;
    }
    return copy_out(dst, r->moments, (size_t)r->n_nodes * MORPH_WORDS * 8, mem);
}
const uint64_t* ctg_result_device_edges(const ctg_result* r) { return r ? r->edges : nullptr; }
const double* ctg_result_device_features(const ctg_result* r) { return r ? r->features : nullptr; }
int ctg_result_info(const ctg_result* r, int64_t* n_records, int64_t* n_direct) {
    if (!r) return CTG_ERR_ARG;
    if (n_records) *n_records = r->n_records;
    if (n_direct) *n_direct = r->n_direct;
    return CTG_OK;
}

void ctg_free(ctg_result* r) {
    if (!r) return;
    int d = current_device();
    if (r->device >= 0 && r->device != d) hipSetDevice(r->device);
    if (!r->owned.empty()) {   // the handle's arrays point into these (ctg_mgpu_merge)
        for (void* p : r->owned) dev_free(p);
    } else {
        dev_free(r->edges);
        dev_free(r->nodes);
        dev_free(r->features);
    }
    dev_free(r->stats);
    dev_free(r->stat_sums);
    dev_free(r->counts);
    dev_free(r->row_off);
    dev_free(r->moments);
    if (r->device >= 0 && r->device != d) hipSetDevice(d);
    delete r;
}

int ctg_synth_volume(uint64_t* labels, float* boundary, const int64_t* shape, int64_t z_offset,
                     const int64_t* global_shape, int cell, uint64_t seed, uint64_t label_offset, double noise_amp,
                     void* stream) {
    if (!labels || !shape || cell <= 0) {
        set_error("ctg_synth_volume: bad arguments");
        return CTG_ERR_ARG;
    }
    int64_t g[3] = {z_offset + shape[0], shape[1], shape[2]};
    if (global_shape)
        for (int k = 0; k < 3; ++k) g[k] = global_shape[k];
    CTG_CHECK(launch_synth(labels, boundary, shape, z_offset, g, cell, seed, label_offset, noise_amp,
                           (hipStream_t)stream));
    return CTG_OK;
}

int ctg_synth_affinities(const float* boundary, float* affs, const int64_t* shape, int n_channels,
                         const int32_t* offsets, void* stream) {
    if (!boundary || !affs || !shape || !offsets || n_channels <= 0) {
        set_error("ctg_synth_affinities: bad arguments");
        return CTG_ERR_ARG;
    }
    CTG_CHECK(launch_synth_aff(boundary, affs, shape, n_channels, offsets, (hipStream_t)stream));
    return CTG_OK;
}

}  // extern "C"
