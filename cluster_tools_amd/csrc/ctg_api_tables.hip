// C ABI of libctg.so (include/ctg.h): label overlaps, segment morphology,
// region features and assignments (kernels and back halves: ctg_overlap.hip,
// ctg_morph.hip, ctg_region.hip, ctg_take.hip).  What the entry
// points share comes first; the call scaffold is ctg_api.h's.
#include <hip/hip_runtime.h>

#include <numeric>

#include "ctg_api.h"
#include "ctg_take.h"

using namespace ctg;

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

static ResultPtr empty_region(int device) {
    ResultPtr r = empty_result(device);
    r->reg_count = (uint64_t*)dev_alloc(8);
    r->reg_sum = (double*)dev_alloc(8);
    r->reg_minmax = (float*)dev_alloc(8);
    return r;
}

// an assignment under construction: freed unless release()d to the caller
struct AssignmentFree {
    void operator()(ctg_assignment* a) const { ctg_assignment_free(a); }
};
using AssignmentPtr = std::unique_ptr<ctg_assignment, AssignmentFree>;

// A label volume of ctg_label_overlaps / ctg_morphology / ctg_region_features whose labels reach
// 2^32: the box's sorted unique labels U and the whole array as 32-bit ranks in
// U (monotone; voxels outside the box get some rank and are never read).  The
// ids are read until the call is done: the entry point's StreamWait follows its sides.
struct DenseSide {
    ResultPtr U;
    DevBuf<uint32_t> ids;
    int build(const void* vol, const int64_t* shape, const int64_t* b, const int64_t* e, void* stream,
              const char* who) {
        int rc = nested(U, [&](ctg_result** u) {
            return ctg_unique_labels((const uint64_t*)vol, shape, b, e, CTG_MEM_DEVICE, stream, u);
        });
        if (rc) return rc;
        if (U->n_nodes > RECORD_LIMIT) {
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

// step 2: the ignore label as a rank of side's table; absent from the box: nothing to skip
static int dense_ignore_rank(const DenseSide& side, int* has_ignore, uint64_t* ignore_label, hipStream_t s,
                             const char* who) {
    if (!side.U || !*has_ignore) return CTG_OK;
    DevBuf<uint32_t> rank(4);
    StreamWait wait{s};
    uint32_t h = 0;
    if (!rank) return hip_status(hipErrorOutOfMemory, who);
    CTG_CHECK(launch_overlap_find(side.U->nodes, side.U->n_nodes, *ignore_label, rank, s));
    CTG_CHECK(hipMemcpyAsync(&h, rank.p, 4, hipMemcpyDeviceToHost, s));
    CTG_CHECK(hipStreamSynchronize(s));
    wait.disarm();
    *has_ignore = h != 0xFFFFFFFFu;
    *ignore_label = h;
    return CTG_OK;
}

// The scan of a table call, with its re-entry where labels reach 2^32 and do not fit the 32-bit keys.  vol, bits: the
// call's n label volumes (device) and their widths; scan(&over) scans them as they stand then -- it reads them and the
// ignore pair anew on every call.  0: the scan as given.  If it reports overflow (bit k: volume k), 1: those volumes
// become monotone dense ids (d[k]); 2: so does the ignore label, if it is one of volume `ignore_vol`'s; 3: the scan
// runs again on the ids; 4: which cannot overflow; 5: r's nodes, which are the first volume's, map back to labels
// through d[0].U.  Whatever else holds ids (the pairs of the overlaps) the caller maps back.
template <class Scan>
static int dense_reentry(const char* who, const void** vol, int* bits, int n, int ignore_vol, int* has_ignore,
                         uint64_t* ignore_label, const int64_t* shape, const int64_t* b, const int64_t* e,
                         void* stream, Scan&& scan, DenseSide* d, ctg_result* r) {
    unsigned over = 0, again = 0;
    int rc = hip_status(scan(&over), who);
    if (rc || !over) return rc;
    for (int k = 0; k < n; ++k) {
        if (!(over >> k & 1u)) continue;
        if ((rc = d[k].build(vol[k], shape, b, e, stream, who)) != CTG_OK) return rc;
        vol[k] = d[k].ids.p;
        bits[k] = 32;
    }
    if (ignore_vol >= 0 &&
        (rc = dense_ignore_rank(d[ignore_vol], has_ignore, ignore_label, (hipStream_t)stream, who)) != CTG_OK)
        return rc;
    if ((rc = hip_status(scan(&again), who)) != CTG_OK) return rc;
    if (again) {
        set_error(std::string(who) + ": dense ids past 2^32");
        return CTG_ERR_UNSUPPORTED;
    }
    if (d[0].U) CTG_CHECK(launch_gather_labels(d[0].U->nodes, r->nodes, r->n_nodes, (hipStream_t)stream));
    return CTG_OK;
}

// The epilogue of a table scan (ApiCall::end, table): it ends synchronised, so the call's guard waits no more.
static int end_table(ApiCall& c, bool timed, StreamWait& wait, ctg_result** out) {
    const int rc = c.end(timed, out, true);
    if (rc == CTG_OK) wait.disarm();
    return rc;
}

// ctg_merge_morphology and ctg_merge_region_features: n float64 rows of `cols` columns -> a result of `empty`'s kind
// by `merge`.  (clear_first: the region call clears *out before its argument check, the morphology call after it.)
static int merge_rows_entry(const char* who, const double* rows, int64_t n, int cols, int mem, void* stream,
                            ResultPtr (*empty)(int),
                            hipError_t (*merge)(Workspace&, const double*, int64_t, hipStream_t, ctg_result*, int*),
                            const char* bad_message, bool clear_first, ctg_result** out) {
    ApiCall c;
    if (clear_first && out) *out = nullptr;
    if (!out || n < 0 || (n > 0 && !rows)) {
        set_error(std::string(who) + ": bad arguments");
        return CTG_ERR_ARG;
    }
    *out = nullptr;
    if (n >= RECORD_LIMIT) {
        set_error(std::string(who) + ": 2^32 rows or more in one call");
        return CTG_ERR_UNSUPPORTED;
    }
    int rc = c.begin(stream, empty);
    if (rc) return rc;
    if (n == 0) return c.end(false, out);
    hipStream_t s = c.s;
    DevInput<double> dr;
    StreamWait wait{s};
    if ((rc = dr.put(rows, (size_t)n * cols * 8, mem, s, who)) != CTG_OK) return rc;
    int bad = 0;
    if ((rc = hip_status(merge(c.w(), dr, n, s, c.r.get(), &bad), who)) != CTG_OK) return rc;
    if (bad) {
        set_error(std::string(who) + bad_message);
        return CTG_ERR_ARG;
    }
    CTG_CHECK(hipStreamSynchronize(s));
    wait.disarm();
    return c.end(false, out);
}

// ctg_morphology_rows and ctg_region_rows, after the checks of their own: the N nodes of r as float64 rows of `cols`
// columns, dense over [label_begin, label_end) into out and / or compact into rows, by launch(od, orw).  copy_fn: the
// call that holds any label.  (range_first: the region call checks the label range before the top label, the
// morphology call after it.)
template <class Launch>
static int rows_entry(const char* who, const ctg_result* r, uint64_t label_begin, uint64_t label_end, int cols,
                      const char* copy_fn, bool range_first, double* out, double* rows, int mem, hipStream_t s,
                      Launch&& launch) {
    const int64_t N = r->n_nodes;
    const uint64_t n = label_end - label_begin;
    const auto range = [&]() -> int {
        if (n <= (1ull << 40)) return CTG_OK;
        set_error(std::string(who) + ": label range too large");
        return CTG_ERR_ARG;
    };
    // the id column is a float64: the largest label (the last: nodes ascend) must fit it
    const auto top_label = [&]() -> int {
        uint64_t top = 0;
        if (N == 0) return CTG_OK;
        CTG_CHECK(hipMemcpyAsync(&top, r->nodes + (N - 1), 8, hipMemcpyDeviceToHost, s));
        CTG_CHECK(hipStreamSynchronize(s));
        if (top < (1ull << 53)) return CTG_OK;
        set_error(std::string(who) + ": a label of 2^53 or more does not fit the float64 id column (" + copy_fn +
                  " holds any label)");
        return CTG_ERR_UNSUPPORTED;
    };
    int rc = range_first ? range() : top_label();
    if (!rc) rc = range_first ? top_label() : range();
    if (rc) return rc;
    DenseOut<double> od, orw;
    StreamWait wait{s};
    rc = hip_status(od.open(out, (size_t)n * cols * 8, mem, true, s), who);
    if (!rc) rc = hip_status(orw.open(rows, (size_t)N * cols * 8, mem, false, s), who);
    if (rc) return rc;
    if (od.d || orw.d) {
        CTG_CHECK(launch(od.d, orw.d));
        CTG_CHECK(od.copy_back(s));
        CTG_CHECK(orw.copy_back(s));
        CTG_CHECK(hipStreamSynchronize(s));
    }
    wait.disarm();
    return CTG_OK;
}

extern "C" {

int ctg_label_overlaps(const void* labels, int label_bits, const void* values, int value_bits, const int64_t* shape,
                       const int64_t* begin, const int64_t* end, int with_ignore, uint64_t ignore_label, int mem,
                       void* stream, ctg_result** out) {
    const char* who = "ctg_label_overlaps";
    ApiCall c;
    if (!labels || !values || !shape || !out) {
        set_error("ctg_label_overlaps: null argument");
        return CTG_ERR_ARG;
    }
    *out = nullptr;
    if ((label_bits != 32 && label_bits != 64) || (value_bits != 32 && value_bits != 64)) {
        set_error("ctg_label_overlaps: label_bits and value_bits must be 32 or 64");
        return CTG_ERR_ARG;
    }
    CallBox box;
    int rc = box_of(who, shape, begin, end, RECORD_LIMIT, &box);
    if (rc || (rc = c.begin(stream, empty_overlaps)) != CTG_OK) return rc;
    if (box.voxels == 0) return c.end(false, out);
    const int64_t *b = box.b, *e = box.e;
    Workspace& w = c.w();
    hipStream_t s = c.s;
    ctg_result* r = c.r.get();
    const int64_t V = shape[0] * shape[1] * shape[2];
    const void *dl = nullptr, *dv = nullptr;
    rc = stage_in(w.stage[0], labels, (size_t)V * (label_bits / 8), mem, s, &dl);
    if (!rc) rc = stage_in(w.stage[1], values, (size_t)V * (value_bits / 8), mem, s, &dv);
    if (rc) return rc;
    const void* vol[2] = {dl, dv};
    int bits[2] = {label_bits, value_bits};
    DenseSide d[2];
    StreamWait wait{s};
    rc = dense_reentry(who, vol, bits, 2, 1, &with_ignore, &ignore_label, shape, b, e, stream,
                       [&](unsigned* over) {
                           return overlap_tables(w, vol[0], bits[0], vol[1], bits[1], shape, b, e, with_ignore,
                                                 ignore_label, s, r, over);
                       },
                       d, r);
    if (rc) return rc;
    // 5, the overlaps' own: the pairs map back to labels
    CTG_CHECK(launch_overlap_map_back(r->n_edges, r->edges, d[0].U ? d[0].U->nodes : nullptr,
                                      d[0].U ? d[0].U->n_nodes : 0, d[1].U ? d[1].U->nodes : nullptr,
                                      d[1].U ? d[1].U->n_nodes : 0, s));
    return end_table(c, r->n_records > 0, wait, out);
}

int ctg_merge_overlaps(const uint64_t* pairs, const uint64_t* counts, int64_t n, int mem, void* stream,
                       ctg_result** out) {
    ApiCall c;
    if (!out || n < 0 || (n > 0 && (!pairs || !counts))) {
        set_error("ctg_merge_overlaps: bad arguments");
        return CTG_ERR_ARG;
    }
    *out = nullptr;
    if (n >= RECORD_LIMIT) {
        set_error("ctg_merge_overlaps: 2^32 rows or more in one call");
        return CTG_ERR_UNSUPPORTED;
    }
    int rc = c.begin(stream, empty_overlaps);
    if (rc) return rc;
    if (n == 0) return c.end(false, out);
    Workspace& w = c.w();
    hipStream_t s = c.s;
    ResultPtr& r = c.r;
    DevInput<uint64_t> dp, dc;
    DensePairs dense;
    DevBuf<uint64_t> key;
    StreamWait wait{s};
    rc = dp.put(pairs, (size_t)n * 16, mem, s, "ctg_merge_overlaps");
    if (!rc) rc = dc.put(counts, (size_t)n * 8, mem, s, "ctg_merge_overlaps");
    if (rc) return rc;
    CTG_CHECK(hipMemsetAsync(w.counters, 0, sizeof(Counters), s));
    CTG_CHECK(launch_max_pairs(n, dp, &w.counters->max_v, s));
    CTG_CHECK(hipMemcpyAsync(w.counters_host, w.counters, sizeof(Counters), hipMemcpyDeviceToHost, s));
    CTG_CHECK(hipStreamSynchronize(s));
    const uint64_t* src = dp;
    if (w.counters_host->max_v >> 32) {
        if ((rc = dense.build(dp, n, s)) != CTG_OK) return rc;
        if (dense.U->n_nodes > RECORD_LIMIT) {
            set_error("ctg_merge_overlaps: more than 2^32 distinct labels");
            return CTG_ERR_UNSUPPORTED;
        }
        src = dense.dense;
    }
    if (!key.alloc((size_t)n * 8)) return hip_status(hipErrorOutOfMemory, "ctg_merge_overlaps");
    CTG_CHECK(launch_overlap_pack(n, src, key, s));
    if ((rc = hip_status(overlap_reduce(w, key, dc, n, s, r.get()), "ctg_merge_overlaps")) != CTG_OK) return rc;
    CTG_CHECK(dense.map_back(r.get(), s));
    CTG_CHECK(hipStreamSynchronize(s));
    wait.disarm();
    r->n_records = n;
    return c.end(false, out);
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
    StreamWait wait{s};
    int rc = hip_status(ol.open(out_labels, n * 8, mem, true, s), "ctg_max_overlaps");
    if (!rc) rc = hip_status(oc.open(out_counts, n * 8, mem, true, s), "ctg_max_overlaps");
    if (rc) return rc;
    CTG_CHECK(launch_overlap_argmax(r, label_begin, label_end, ol.d, oc.d, s));
    CTG_CHECK(ol.copy_back(s));
    CTG_CHECK(oc.copy_back(s));
    CTG_CHECK(hipStreamSynchronize(s));
    wait.disarm();
    return CTG_OK;
}

int ctg_morphology(const void* labels, int label_bits, const int64_t* shape, const int64_t* begin, const int64_t* end,
                   const int64_t* origin, int mem, void* stream, ctg_result** out) {
    const char* who = "ctg_morphology";
    ApiCall c;
    if (!labels || !shape || !out) {
        set_error("ctg_morphology: null argument");
        return CTG_ERR_ARG;
    }
    *out = nullptr;
    if (label_bits != 32 && label_bits != 64) {
        set_error("ctg_morphology: label_bits must be 32 or 64");
        return CTG_ERR_ARG;
    }
    CallBox box;
    int64_t o[3];
    int rc = box_of(who, shape, begin, end, RECORD_LIMIT, &box);
    if (rc) return rc;
    const int64_t *b = box.b, *e = box.e;
    for (int k = 0; k < 3; ++k) {
        o[k] = origin ? origin[k] : 0;
        // a coordinate below 2^31 and fewer than 2^32 voxels: no sum reaches 2^63
        if (o[k] < 0 || o[k] >= (1ll << 31) || o[k] + e[k] >= (1ll << 31)) {
            set_error("ctg_morphology: origin + end must stay below 2^31 on every axis (origin >= 0)");
            return CTG_ERR_ARG;
        }
    }
    if ((rc = c.begin(stream, empty_morphology)) != CTG_OK) return rc;
    if (box.voxels == 0) return c.end(false, out);
    Workspace& w = c.w();
    hipStream_t s = c.s;
    ctg_result* r = c.r.get();
    const int64_t V = shape[0] * shape[1] * shape[2];
    const void* dl = nullptr;
    if ((rc = stage_in(w.stage[0], labels, (size_t)V * (label_bits / 8), mem, s, &dl)) != CTG_OK) return rc;
    DenseSide d;
    StreamWait wait{s};
    rc = dense_reentry(   // (2: no ignore label here)
        who, &dl, &label_bits, 1, -1, nullptr, nullptr, shape, b, e, stream,
        [&](unsigned* over) { return morph_tables(w, dl, label_bits, shape, b, e, o, s, r, over); }, &d, r);
    if (rc) return rc;
    return end_table(c, true, wait, out);
}

int ctg_merge_morphology(const double* rows, int64_t n, int mem, void* stream, ctg_result** out) {
    return merge_rows_entry(
        "ctg_merge_morphology", rows, n, CTG_MORPH_COLS, mem, stream, empty_morphology, morph_merge,
        ": a row's id is not an integer in [0, 2^53), or its size, centre or box is negative or not finite", false,
        out);
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
    return rows_entry("ctg_morphology_rows", r, label_begin, label_end, CTG_MORPH_COLS, "ctg_result_copy_moments",
                      false, out, rows, mem, s,
                      [&](double* od, double* oc) { return launch_morph_rows(r, label_begin, label_end, od, oc, s); });
}

int ctg_region_features(const void* labels, int label_bits, const void* data, int data_kind, const int64_t* shape,
                        const int64_t* begin, const int64_t* end, int has_ignore, uint64_t ignore_label, int mem,
                        void* stream, ctg_result** out) {
    const char* who = "ctg_region_features";
    ApiCall c;
    if (out) *out = nullptr;
    if (!labels || !data || !shape || !out) {
        set_error("ctg_region_features: null argument");
        return CTG_ERR_ARG;
    }
    if (label_bits != 32 && label_bits != 64) {
        set_error("ctg_region_features: label_bits must be 32 or 64");
        return CTG_ERR_ARG;
    }
    if (data_kind != CTG_DATA_F32 && data_kind != CTG_DATA_U8) {
        set_error("ctg_region_features: data_kind must be CTG_DATA_F32 or CTG_DATA_U8");
        return CTG_ERR_ARG;
    }
    if (!mem_ok("ctg_region_features", mem)) return CTG_ERR_ARG;
    CallBox box;
    int rc = box_of(who, shape, begin, end, RECORD_LIMIT, &box);
    if (rc || (rc = c.begin(stream, empty_region)) != CTG_OK) return rc;
    if (box.voxels == 0) return c.end(false, out);
    const int64_t *b = box.b, *e = box.e;
    Workspace& w = c.w();
    hipStream_t s = c.s;
    ctg_result* r = c.r.get();
    const int64_t V = shape[0] * shape[1] * shape[2];
    const void *dl = nullptr, *dd = nullptr;
    rc = stage_in(w.stage[0], labels, (size_t)V * (label_bits / 8), mem, s, &dl);
    if (!rc) rc = stage_in(w.stage[1], data, (size_t)V * (data_kind == CTG_DATA_U8 ? 1 : 4), mem, s, &dd);
    if (rc) return rc;
    DenseSide d;
    StreamWait wait{s};
    rc = dense_reentry(who, &dl, &label_bits, 1, 0, &has_ignore, &ignore_label, shape, b, e, stream,
                       [&](unsigned* over) {
                           return region_tables(w, dl, label_bits, dd, data_kind, shape, b, e, has_ignore,
                                                ignore_label, s, r, over);
                       },
                       &d, r);
    if (rc) return rc;
    return end_table(c, r->n_records > 0, wait, out);
}

int ctg_merge_region_features(const double* rows, int64_t n, int mem, void* stream, ctg_result** out) {
    return merge_rows_entry(
        "ctg_merge_region_features", rows, n, CTG_REGION_COLS, mem, stream, empty_region, region_merge,
        ": a row's id is not an integer in [0, 2^53), or its count is negative or not finite", true, out);
}

int ctg_region_rows(const ctg_result* r, uint64_t label_begin, uint64_t label_end, int form, double norm, double* out,
                    double* rows, int mem, void* stream) {
    DevLock dev_lock;
    if (!r || label_end < label_begin) {
        set_error("ctg_region_rows: bad arguments");
        return CTG_ERR_ARG;
    }
    if (form != CTG_REGION_SUMS && form != CTG_REGION_FEATURES) {
        set_error("ctg_region_rows: form must be CTG_REGION_SUMS or CTG_REGION_FEATURES");
        return CTG_ERR_ARG;
    }
    if (!(norm > 0.0) || !(norm < 1.0 / 0.0)) {
        set_error("ctg_region_rows: norm must be finite and positive");
        return CTG_ERR_ARG;
    }
    if (!r->reg_count) {
        set_error("ctg_region_rows: not a region-features result (ctg_region_features, ctg_merge_region_features)");
        return CTG_ERR_ARG;
    }
    hipStream_t s = (hipStream_t)stream;
    return rows_entry("ctg_region_rows", r, label_begin, label_end, CTG_REGION_COLS, "ctg_result_copy_region", true,
                      out, rows, mem, s, [&](double* od, double* orw) {
                          return launch_region_rows(r, label_begin, label_end, form, norm, od, orw, s);
                      });
}

int ctg_assignment_dense(const uint64_t* table, int64_t n, int mem, void* stream, ctg_assignment** out) {
    ApiCall c;
    if (out) *out = nullptr;
    if (!out || n < 0 || (n > 0 && !table)) {
        set_error("ctg_assignment_dense: bad arguments");
        return CTG_ERR_ARG;
    }
    if (!mem_ok("ctg_assignment_dense", mem)) return CTG_ERR_ARG;
    int rc = c.begin(stream);
    if (rc) return rc;
    hipStream_t s = c.s;
    AssignmentPtr a(new ctg_assignment());
    a->device = c.dev;
    a->kind = CTG_ASSIGN_DENSE;
    a->n = n;
    a->size = (uint64_t)n;
    DevBuf<unsigned long long> stat(16);
    StreamWait wait{s};
    if (!stat || !(a->table = (uint64_t*)dev_alloc(std::max<size_t>((size_t)n * 8, 8))))
        return hip_status(hipErrorOutOfMemory, "ctg_assignment_dense");
    CTG_CHECK(hipMemsetAsync(stat.p, 0, 16, s));
    if (n)
        CTG_CHECK(hipMemcpyAsync(a->table, table, (size_t)n * 8,
                                 mem == CTG_MEM_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, s));
    CTG_CHECK(launch_take_max(a->table, n, stat, s));
    unsigned long long h[2] = {0, 0};
    CTG_CHECK(hipMemcpyAsync(h, stat.p, 16, hipMemcpyDeviceToHost, s));
    CTG_CHECK(hipStreamSynchronize(s));
    wait.disarm();
    a->max_value = h[1];
    *out = a.release();
    return CTG_OK;
}

int ctg_assignment_sparse(const uint64_t* keys, const uint64_t* values, int64_t n, int mem, void* stream,
                          ctg_assignment** out) {
    const char* who = "ctg_assignment_sparse";
    ApiCall c;
    if (out) *out = nullptr;
    if (!out || n < 0 || (n > 0 && (!keys || !values))) {
        set_error("ctg_assignment_sparse: bad arguments");
        return CTG_ERR_ARG;
    }
    if (!mem_ok("ctg_assignment_sparse", mem)) return CTG_ERR_ARG;
    if (n > (1ll << 40)) {
        set_error("ctg_assignment_sparse: more than 2^40 pairs");
        return CTG_ERR_UNSUPPORTED;
    }
    int rc = c.begin(stream);
    if (rc) return rc;
    hipStream_t s = c.s;
    AssignmentPtr a(new ctg_assignment());
    a->device = c.dev;
    a->kind = CTG_ASSIGN_SPARSE;
    a->n = n;
    a->size = take_capacity(n);
    const size_t slot_bytes = (size_t)a->size * 16;
    DevBuf<unsigned long long> stat(16);
    DevInput<uint64_t> dk, dv;
    StreamWait wait{s};
    if (!stat || !(a->table = (uint64_t*)dev_alloc((size_t)take_table_words(a->size) * 8)))
        return hip_status(hipErrorOutOfMemory, who);
    rc = dk.put(keys, (size_t)n * 8, mem, s, who);
    if (!rc) rc = dv.put(values, (size_t)n * 8, mem, s, who);
    if (rc) return rc;
    CTG_CHECK(hipMemsetAsync(stat.p, 0, 16, s));
    CTG_CHECK(hipMemsetAsync(a->table, 0xFF, slot_bytes, s));               // every slot free
    CTG_CHECK(hipMemsetAsync((char*)a->table + slot_bytes, 0, 16, s));      // the side words
    CTG_CHECK(launch_take_build(dk, dv, n, a->table, a->size, stat, s));
    unsigned long long h[2] = {0, 0};
    CTG_CHECK(hipMemcpyAsync(h, stat.p, 16, hipMemcpyDeviceToHost, s));
    CTG_CHECK(hipStreamSynchronize(s));
    wait.disarm();
    if (h[0]) {
        set_error("ctg_assignment_sparse: " + std::to_string(h[0]) + " duplicate key(s)");
        return CTG_ERR_ARG;
    }
    a->max_value = h[1];
    *out = a.release();
    return CTG_OK;
}

int ctg_assignment_info(const ctg_assignment* a, int64_t* n, uint64_t* max_value, int* kind) {
    if (!a) {
        set_error("ctg_assignment_info: null handle");
        return CTG_ERR_ARG;
    }
    if (n) *n = a->n;
    if (max_value) *max_value = a->max_value;
    if (kind) *kind = a->kind;
    return CTG_OK;
}

void ctg_assignment_free(ctg_assignment* a) {
    if (!a) return;
    const int d = current_device();
    if (a->device >= 0 && a->device != d) hipSetDevice(a->device);
    dev_free(a->table);
    if (a->device >= 0 && a->device != d) hipSetDevice(d);
    delete a;
}

int ctg_apply_assignment(const ctg_assignment* a, const void* labels, int label_bits, int64_t n,
                         const int64_t* seg_begin, const uint64_t* seg_offset, int64_t n_seg, int allow_missing,
                         uint64_t* out, uint64_t* seg_nonzero, uint64_t* missing, int mem, void* stream) {
    const char* who = "ctg_apply_assignment";
    ApiCall c;
    if (!a || !seg_nonzero || !missing || (n > 0 && !labels) || (seg_begin && !seg_offset && n_seg > 0)) {
        set_error("ctg_apply_assignment: null argument");
        return CTG_ERR_ARG;
    }
    if (label_bits != 32 && label_bits != 64) {
        set_error("ctg_apply_assignment: label_bits must be 32 or 64");
        return CTG_ERR_ARG;
    }
    if (!mem_ok("ctg_apply_assignment", mem)) return CTG_ERR_ARG;
    if (n < 0 || (seg_begin && n_seg < 0)) {
        set_error("ctg_apply_assignment: negative n or n_seg");
        return CTG_ERR_ARG;
    }
    if (seg_begin && n_seg > 0x7FFFFFFFll) {
        set_error("ctg_apply_assignment: 2^31 segments or more in one call");
        return CTG_ERR_UNSUPPORTED;
    }
    const TakeChunks chunks = take_chunk_prefix(seg_begin, n_seg, n, TAKE_CHUNK);
    if (chunks.error == TakeChunks::BAD_SEGMENTS) {
        set_error("ctg_apply_assignment: seg_begin must ascend from 0 to n");
        return CTG_ERR_ARG;
    }
    if (chunks.error == TakeChunks::TOO_MANY_CHUNKS) {
        set_error("ctg_apply_assignment: 2^43 voxels or more in one call");
        return CTG_ERR_UNSUPPORTED;
    }
    if (allow_missing && a->kind != CTG_ASSIGN_SPARSE) {
        set_error("ctg_apply_assignment: allow_missing needs a sparse assignment");
        return CTG_ERR_ARG;
    }
    if (out && (const void*)out == labels && label_bits != 64) {
        set_error("ctg_apply_assignment: in place needs 64-bit labels");
        return CTG_ERR_ARG;
    }
    if (((uintptr_t)labels & (uintptr_t)(label_bits / 8 - 1)) || ((uintptr_t)out & 7u)) {
        set_error("ctg_apply_assignment: labels and out must be aligned to their element size");
        return CTG_ERR_ARG;
    }
    const int64_t ns = seg_begin ? n_seg : 1;
    int rc = c.begin(stream);
    if (rc) return rc;
    hipStream_t s = c.s;
    missing[0] = missing[1] = 0;
    for (int64_t k = 0; k < ns; ++k) seg_nonzero[k] = 0;
    if (n == 0) return CTG_OK;
    // one device block: seg_begin (ns + 1), seg_off (ns), the counts (missing 2 + nonzero ns x slots), prefix (ns + 1, u32)
    const int slots = take_count_slots(ns);
    const size_t words = (size_t)(ns + 1) + (size_t)ns + 2 + (size_t)ns * slots;
    std::vector<uint64_t> h(words + ((size_t)ns + 2) / 2, 0);
    const int64_t whole[2] = {0, n};
    std::copy_n(seg_begin ? seg_begin : whole, ns + 1, (int64_t*)h.data());
    if (seg_begin) std::copy_n(seg_offset, ns, h.data() + ns + 1);
    h[2 * ns + 2] = ~0ull;   // the smallest missing label starts at all ones
    std::copy(chunks.prefix.begin(), chunks.prefix.end(), (uint32_t*)(h.data() + words));
    DevBuf<uint64_t> seg(h.size() * 8), dout;
    DevInput<char> dl;
    StreamWait wait{s};
    if (!seg) return hip_status(hipErrorOutOfMemory, who);
    CTG_CHECK(hipMemcpyAsync(seg.p, h.data(), h.size() * 8, hipMemcpyHostToDevice, s));
    const bool host = mem == CTG_MEM_HOST;
    const size_t lbytes = (size_t)n * (label_bits / 8);
    if ((rc = dl.put((const char*)labels, lbytes, mem, s, who)) != CTG_OK) return rc;
    uint64_t* o = out;
    if (host && out) {
        // (a host call in place: the copy of the labels is overwritten instead)
        o = (const void*)out == labels ? (uint64_t*)dl.own.p : dout.alloc((size_t)n * 8);
        if (!o) return hip_status(hipErrorOutOfMemory, who);
    }
    TakeArgs A{};
    A.labels = dl.p;
    A.out = o;
    A.seg_begin = (const int64_t*)seg.p;
    A.seg_off = seg.p + ns + 1;
    A.missing = (unsigned long long*)(seg.p + 2 * ns + 1);
    A.seg_nonzero = A.missing + 2;
    A.prefix = (const uint32_t*)(seg.p + words);
    A.n_seg = (int)ns;
    A.nz_slots = slots;
    A.table = a->table;
    A.size = a->size;
    A.par = (int)(((uintptr_t)dl.p / (uintptr_t)(label_bits / 8)) & 1u);
    A.wide_store = o && (int)(((uintptr_t)o >> 3) & 1u) == A.par;
    Ev ev{c.w(), s};   // a profiled call: the kernel is phase 0, the other phases are empty
    ev.mark(0);
    CTG_CHECK(launch_take(A, label_bits, a->kind == CTG_ASSIGN_DENSE, chunks.prefix[ns], s));
    for (int i = 1; i <= 6; ++i) ev.mark(i);
    std::vector<uint64_t> back((size_t)ns * slots + 2);
    CTG_CHECK(hipMemcpyAsync(back.data(), seg.p + 2 * ns + 1, back.size() * 8, hipMemcpyDeviceToHost, s));
    if (host && out) CTG_CHECK(hipMemcpyAsync(out, o, (size_t)n * 8, hipMemcpyDeviceToHost, s));
    CTG_CHECK(hipStreamSynchronize(s));
    wait.disarm();
    if (c.w().profiling && (rc = read_phase_times(c.w(), s)) != CTG_OK) return rc;
    missing[0] = back[0];
    missing[1] = back[0] ? back[1] : 0;
    for (int64_t k = 0; k < ns; ++k)
        seg_nonzero[k] = std::accumulate(back.begin() + 2 + k * slots, back.begin() + 2 + (k + 1) * slots, (uint64_t)0);
    if (missing[0] && !allow_missing) {
        set_error(std::string(who) + ": " + std::to_string(missing[0]) + " voxel(s) without an entry, the smallest label " +
                  std::to_string(missing[1]) +
                  (a->kind == CTG_ASSIGN_DENSE ? " (the table has " + std::to_string(a->n) + " entries)" : ""));
        return CTG_ERR_MISSING;
    }
    return CTG_OK;
}

}  // extern "C"
