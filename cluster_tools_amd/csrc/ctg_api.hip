// C ABI of libctg.so (include/ctg.h): the error state, the result handles and
// the entry points that are neither the face scan (ctg_api_scan.hip), a label
// table (ctg_api_tables.hip), the thresholded components (ctg_api_cc.hip) nor
// the multi-GPU exchange (ctg_api_mgpu.hip) -- device and profiling, unique /
// merge / map, the synthetic volumes -- and the definitions behind ctg_api.h,
// the sorting ones included: of the API files only this one instantiates
// rocPRIM.  The allocator and the workspace live in
// ctg_workspace.hip (ctg_pool.h, ctg_buffers.h), the record back half in
// ctg_records.hip, the host decisions in ctg_plan.h.
#include <hip/hip_runtime.h>
#include <cstdlib>
#include <cstring>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_select.hpp>

#include <algorithm>
#include <cstdio>

#include "ctg_api.h"

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

int hip_status(hipError_t e, const char* who, int oom_status) {
    if (e == hipSuccess) return CTG_OK;
    set_error(std::string(who) + ": " + hipGetErrorString(e));
    return e == hipErrorOutOfMemory ? oom_status : CTG_ERR_HIP;
}

int box_of(const char* who, const int64_t* shape, const int64_t* begin, const int64_t* end, int64_t max_voxels,
           CallBox* box) {
    *box = call_box(shape, begin, end, max_voxels);
    if (box->error == CallBox::OUTSIDE) {
        set_error(std::string(who) + ": box outside the array");
        return CTG_ERR_ARG;
    }
    if (box->error == CallBox::TOO_LARGE) {
        set_error(std::string(who) + ": boxes of 2^32 voxels or more are not supported");
        return CTG_ERR_UNSUPPORTED;
    }
    return CTG_OK;
}

int stage_in(GrowBuf& stage, const void* src, size_t bytes, int mem, hipStream_t s, const void** dev) {
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

hipError_t sort_unique_u64(Workspace& w, const uint64_t* in, int64_t n, uint64_t* out, uint32_t* count_dev,
                           hipStream_t s, unsigned end_bit) {
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

int read_word(Workspace& w, SmallSlot i, hipStream_t s, int64_t* v) {
    CTG_CHECK(hipMemcpyAsync(w.small_host + i, w.small + i, 4, hipMemcpyDeviceToHost, s));
    CTG_CHECK(hipStreamSynchronize(s));
    *v = w.small_host[i];
    return CTG_OK;
}

int read_phase_times(Workspace& w, hipStream_t s) {
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

hipError_t map_back(const ctg_result* U, ctg_result* r, hipStream_t s) {
    hipError_t e = launch_gather_labels(U->nodes, r->edges, 2 * r->n_edges, s);
    if (e == hipSuccess) e = launch_gather_labels(U->nodes, r->nodes, r->n_nodes, s);
    return e;
}

}  // namespace ctg

using namespace ctg;

// The body of the pair-list entry points (ctg_merge_stats, ctg_unique_pairs):
// J describes the call but for the J.n (u,v) pairs dk, which are relabelled
// densely where a label reaches 2^32.
static int reduce_pairs(ApiCall& c, ReduceJob& J, const uint64_t* dk, const char* who, ctg_result** out) {
    Workspace& w = c.w();
    hipStream_t s = c.s;
    DensePairs dp;
    StreamWait wait{s};   // (for the caller's inputs too: its own guard covers only its staging)
    CTG_CHECK(hipMemsetAsync(w.counters, 0, sizeof(Counters), s));
    CTG_CHECK(launch_max_pairs(J.n, dk, &w.counters->max_v, s));
    CTG_CHECK(hipMemcpyAsync(w.counters_host, w.counters, sizeof(Counters), hipMemcpyDeviceToHost, s));
    CTG_CHECK(hipStreamSynchronize(s));
    J.pairs = dk;
    J.max_v = w.counters_host->max_v;
    if (J.max_v >> 32) {
        const int rc = dp.build(dk, J.n, s);
        if (rc) return rc;
        J.pairs = dp.dense;
        J.max_v = (uint64_t)std::max<int64_t>(dp.U->n_nodes - 1, 0);
    }
    c.r = new_result(c.dev);
    hipError_t e = reduce_records(w, J, s, c.r.get());
    if (e == hipSuccess) e = dp.map_back(c.r.get(), s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    const int rc = hip_status(e, who, CTG_ERR_HIP);
    if (rc) return rc;
    wait.disarm();
    return c.end(false, out);
}

// ---------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------
extern "C" {

int ctg_version(void) { return 1; }

const char* ctg_last_error(void) { return g_err.c_str(); }

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
    hipError_t (*take[8])(unsigned long long*) = {bounds_take_api,    bounds_take_scan, bounds_take_sort,
                                                   bounds_take_reduce, bounds_take_mgpu, bounds_take_overlap,
                                                   bounds_take_morph,  bounds_take_region};
    out[0] = out[1] = out[2] = out[3] = 0;
    int found = 0;
    for (int f = 0; f < 8; ++f) {
        unsigned long long h[3] = {0, 0, 0};
        CTG_CHECK(take[f](h));
        if (h[0] && !found) {
            out[0] = (uint64_t)f + 1;   // 1 api, 2 scan, 3 sort, 4 reduce, 5 mgpu, 6 overlap, 7 morph, 8 region
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

int ctg_last_sort(int64_t* out, int n) {
    if (!out || n < 0) {
        set_error("ctg_last_sort: null argument");
        return CTG_ERR_ARG;
    }
    const SortReport& r = ws(current_device()).last_sort;
    int64_t v[CTG_SORT_WORDS];
    v[CTG_SORT_PATH] = r.path;
    v[CTG_SORT_PACKED] = r.packed;
    v[CTG_SORT_GROUP_TRIED] = r.group_tried;
    v[CTG_SORT_GROUP_DONE] = r.group_done;
    v[CTG_SORT_GROUP_WHY] = r.group_tried && !r.group_done ? (int)r.group.why : 0;
    v[CTG_SORT_GROUP_SHIFT] = r.group.shift;
    v[CTG_SORT_GROUP_BUCKETS] = r.group.nbk;
    v[CTG_SORT_GROUP_LARGEST] = r.largest;
    v[CTG_SORT_IB] = r.ib;
    v[CTG_SORT_NB] = r.nb;
    v[CTG_SORT_UB] = r.ub;
    v[CTG_SORT_N] = r.n;
    for (int i = 0; i < n && i < CTG_SORT_WORDS; ++i) out[i] = v[i];
    return CTG_OK;
}

int ctg_last_scan(int64_t* out, int n) {
    if (!out || n < 0) {
        set_error("ctg_last_scan: null buffer or negative count");
        return CTG_ERR_ARG;
    }
    const ScanReport& r = ws(current_device()).last_scan;
    int64_t v[CTG_SCAN_WORDS];
    v[CTG_SCAN_WAVES] = r.waves[0];
    v[CTG_SCAN_INTERIOR_WAVES] = r.interior[0];
    v[CTG_SCAN_NARROW_WAVES] = r.waves[1];
    v[CTG_SCAN_NARROW_INTERIOR_WAVES] = r.interior[1];
    for (int i = 0; i < n && i < CTG_SCAN_WORDS; ++i) out[i] = v[i];
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
    ApiCall c;
    if (!labels || !shape || !out) {
        set_error("ctg_unique_labels: null argument");
        return CTG_ERR_ARG;
    }
    *out = nullptr;
    CallBox box;
    int rc = box_of("ctg_unique_labels", shape, begin, end, 0, &box);
    if (rc || (rc = c.begin(stream)) != CTG_OK) return rc;
    Workspace& w = c.w();
    hipStream_t s = c.s;
    const int64_t V = shape[0] * shape[1] * shape[2];
    const void* dl = nullptr;
    if ((rc = stage_in(w.stage[0], labels, (size_t)V * 8, mem, s, &dl)) != CTG_OK) return rc;
    if (box.voxels == 0) return c.empty(empty_result, out);
    c.r = new_result(c.dev);
    DevBuf<uint64_t> nodes;
    rc = unique_candidates(
        w, candidate_cap_first(box.voxels), box.voxels, 64u, s, "ctg_unique_labels: out of device memory",
        "ctg_unique_labels: candidate buffer overflow",
        [&](uint64_t* cand, unsigned long long* count, int64_t cap) {
            return launch_unique_tiles((const uint64_t*)dl, shape, box.b, box.e, cand, count, cap, s);
        },
        nodes, &c.r->n_nodes);
    if (rc) return rc;
    c.r->nodes = nodes.release();
    c.r->edges = (uint64_t*)dev_alloc(16);
    return c.end(false, out);
}

int ctg_unique_values(const uint64_t* values, int64_t n, int mem, void* stream, ctg_result** out) {
    ApiCall c;
    if (!out || n < 0 || (n > 0 && !values)) {
        set_error("ctg_unique_values: bad arguments");
        return CTG_ERR_ARG;
    }
    *out = nullptr;
    int rc = c.begin(stream);
    if (rc) return rc;
    if (n == 0) return c.empty(empty_result, out);
    Workspace& w = c.w();
    hipStream_t s = c.s;
    ResultPtr& r = c.r = new_result(c.dev);
    r->edges = (uint64_t*)dev_alloc(16);
    r->nodes = (uint64_t*)dev_alloc(n * 8);
    if (!r->nodes) {
        set_error("ctg_unique_values: out of device memory");
        return CTG_ERR_NOMEM;
    }
    DevInput<uint64_t> in;
    StreamWait wait{s};
    if ((rc = in.put(values, (size_t)n * 8, mem, s, "ctg_unique_values")) != CTG_OK) return rc;
    CTG_CHECK(sort_unique_u64(w, in, n, r->nodes, w.small + SLOT_NODES, s));
    if ((rc = read_word(w, SLOT_NODES, s, &r->n_nodes)) != CTG_OK) return rc;
    wait.disarm();
    return c.end(false, out);
}

int ctg_merge_stats(const uint64_t* keys, const double* sums, const uint32_t* records, int64_t n, double hist_lo,
                    double hist_hi, int keep_stats, int mem, void* stream, ctg_result** out) {
    ApiCall c;
    if (!out || n < 0 || (n > 0 && (!keys || !sums || !records))) {
        set_error("ctg_merge_stats: bad arguments");
        return CTG_ERR_ARG;
    }
    *out = nullptr;
    int rc = c.begin(stream);
    if (rc) return rc;
    if (n == 0) return c.empty(empty_result, out);
    hipStream_t s = c.s;
    // inputs to device (merge buffers are separate from the scan records)
    DevInput<uint64_t> dk;
    DevInput<double> ds;
    DevInput<uint32_t> dr;
    StreamWait wait{s};
    rc = dk.put(keys, (size_t)n * 16, mem, s, "ctg_merge_stats");
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
    if ((rc = reduce_pairs(c, J, dk, "ctg_merge_stats", out)) == CTG_OK) wait.disarm();
    return rc;
}

int ctg_merge_feature_rows(const uint64_t* ids, const double* rows, int64_t n, int64_t id_begin, int64_t id_end,
                           double* out, int mem, void* stream) {
    ApiCall c;
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
    int rc = c.begin(stream);
    if (rc) return rc;
    Workspace& w = c.w();
    hipStream_t s = c.s;
    const bool host = mem == CTG_MEM_HOST;
    DevInput<uint64_t> di;
    DevInput<double> dr;
    DevBuf<double> own_o;
    StreamWait wait{s};
    double* dout = out;
    rc = di.put(ids, (size_t)n * 8, mem, s, "ctg_merge_feature_rows");
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
    wait.disarm();
    if (n && w.small_host[SLOT_BAD_ID]) {
        set_error("ctg_merge_feature_rows: an edge id lies outside [id_begin, id_end)");
        return CTG_ERR_ARG;
    }
    return CTG_OK;
}

int ctg_unique_pairs(const uint64_t* pairs, int64_t n, int mem, void* stream, ctg_result** out) {
    ApiCall c;
    if (!out || n < 0 || (n > 0 && !pairs)) {
        set_error("ctg_unique_pairs: bad arguments");
        return CTG_ERR_ARG;
    }
    *out = nullptr;
    int rc = c.begin(stream);
    if (rc) return rc;
    if (n == 0) return c.empty(empty_result, out);
    DevInput<uint64_t> dk;
    StreamWait wait{c.s};
    if ((rc = dk.put(pairs, (size_t)n * 16, mem, c.s, "ctg_unique_pairs")) != CTG_OK) return rc;
    ReduceJob J{};
    J.n = n;
    J.stats = 0;
    J.need_adj = 0;
    J.scale = 1.0;
    J.offset = 0.0;
    if ((rc = reduce_pairs(c, J, dk, "ctg_unique_pairs", out)) == CTG_OK) wait.disarm();
    return rc;
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
    StreamWait wait{s};
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
    wait.disarm();
    return CTG_OK;
}

int64_t ctg_result_num_edges(const ctg_result* r) { return r ? r->n_edges : -1; }
int64_t ctg_result_num_nodes(const ctg_result* r) { return r ? r->n_nodes : -1; }

// The accessors' copy, on the copy stream of the handle's device and waited
// for: the calls that fill a handle end synchronised, so its tables are ready
// on any stream, and the copy neither runs on the null stream nor waits for it.
// (No device lock: a copy does not queue behind another thread's call.  The
// call that made the handle made that device's workspace, copy stream included.)
static int copy_out(const ctg_result* r, void* dst, const void* src, size_t bytes, int mem) {
    if (bytes == 0) return CTG_OK;
    if (!dst || !src) {
        set_error("copy: null pointer");
        return CTG_ERR_ARG;
    }
    const int cur = current_device(), dev = r->device >= 0 ? r->device : cur;
    Workspace& w = ws(dev);
    if (!w.ready) {
        set_error("copy: the handle's device has no workspace");
        return CTG_ERR_ARG;
    }
    if (dev != cur) CTG_CHECK(hipSetDevice(dev));
    hipError_t e = hipMemcpyAsync(dst, src, bytes, mem == CTG_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost,
                                  w.copy_stream);
    if (e == hipSuccess) e = hipStreamSynchronize(w.copy_stream);
    if (dev != cur) hipSetDevice(cur);
    CTG_CHECK(e);
    return CTG_OK;
}

int ctg_result_copy_edges(const ctg_result* r, uint64_t* dst, int mem) {
    return copy_out(r, dst, r->edges, (size_t)r->n_edges * 16, mem);
}
int ctg_result_copy_nodes(const ctg_result* r, uint64_t* dst, int mem) {
    return copy_out(r, dst, r->nodes, (size_t)r->n_nodes * 8, mem);
}
int ctg_result_copy_features(const ctg_result* r, double* dst, int mem) {
    if (!r->features && r->n_edges) {
        set_error("result has no features (graph-only call)");
        return CTG_ERR_ARG;
    }
    return copy_out(r, dst, r->features, (size_t)r->n_edges * N_FEATURES * 8, mem);
}
int ctg_result_copy_stats(const ctg_result* r, double* sums_dst, uint32_t* records_dst, int mem) {
    if (!r->stats && r->n_edges) {
        set_error("result has no statistics (call with keep_stats=1 and data)");
        return CTG_ERR_ARG;
    }
    int rc = copy_out(r, sums_dst, r->stat_sums, (size_t)r->n_edges * 16, mem);
    if (rc) return rc;
    return copy_out(r, records_dst, r->stats, (size_t)r->n_edges * WREC_WORDS * 4, mem);
}
int ctg_result_copy_counts(const ctg_result* r, uint64_t* dst, int mem) {
    if (!r->counts) {
        set_error("result has no counts (not an overlaps result)");
        return CTG_ERR_ARG;
    }
    return copy_out(r, dst, r->counts, (size_t)r->n_edges * 8, mem);
}
int ctg_result_copy_moments(const ctg_result* r, uint64_t* dst, int mem) {
    if (!r || !r->moments) {
        set_error("result has no moments (not a morphology result)");
        return CTG_ERR_ARG;
    }
    return copy_out(r, dst, r->moments, (size_t)r->n_nodes * MORPH_WORDS * 8, mem);
}
int ctg_result_copy_region(const ctg_result* r, uint64_t* counts, double* sums, float* minmax, int mem) {
    if (!r || !r->reg_count) {
        set_error("result has no region moments (not a region-features result)");
        return CTG_ERR_ARG;
    }
    int rc = counts ? copy_out(r, counts, r->reg_count, (size_t)r->n_nodes * 8, mem) : CTG_OK;
    if (!rc && sums) rc = copy_out(r, sums, r->reg_sum, (size_t)r->n_nodes * 8, mem);
    if (!rc && minmax) rc = copy_out(r, minmax, r->reg_minmax, (size_t)r->n_nodes * 8, mem);
    return rc;
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
    dev_free(r->reg_count);
    dev_free(r->reg_sum);
    dev_free(r->reg_minmax);
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
