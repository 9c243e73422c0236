// What the C-ABI entry points share (ctg_api.hip: handles, unique / merge /
// map; ctg_api_scan.hip: the face scan; ctg_api_tables.hip: label overlaps
// and morphology; ctg_api_cc.hip: the thresholded components;
// ctg_api_edt.hip: the distance transform; ctg_api_ws.hip: the seeded
// watershed; ctg_api_mgpu.hip: the multi-GPU exchange): the call scaffold, the
// status of a HIP error, the mem check, inputs and outputs that may live on the
// host, the prologue of a dense-volume call (DenseCall: box, extent, VolBox,
// staging and output by element width), a call's device words read back, and
// the dense relabelling of (u,v) pair lists.  Every scope that owns pool blocks
// declares a StreamWait (ctg_buffers.h) after them.  No rocPRIM here: the two helpers
// that sort (sort_unique_u64, and with it unique_candidates) are defined in
// ctg_api.hip.
#pragma once
#include <algorithm>
#include <string>

#include "ctg_internal.h"

namespace ctg {

// who: hip error string, and the status it maps to.  Out of memory is
// CTG_ERR_NOMEM unless the site has always reported CTG_ERR_HIP for it
// (oom_status), as every CTG_CHECK site does.
int hip_status(hipError_t e, const char* who, int oom_status = CTG_ERR_NOMEM);

// the box [b, e) of a call (ctg_plan.h: call_box) with its two errors;
// max_voxels 0: no limit
int box_of(const char* who, const int64_t* shape, const int64_t* begin, const int64_t* end, int64_t max_voxels,
           CallBox* box);

// mem is CTG_MEM_HOST or CTG_MEM_DEVICE, or the error is set
inline bool mem_ok(const char* who, int mem) {
    if (mem == CTG_MEM_HOST || mem == CTG_MEM_DEVICE) return true;
    set_error(std::string(who) + ": mem must be CTG_MEM_HOST or CTG_MEM_DEVICE");
    return false;
}

// a host volume into the workspace's staging slot; a device one as it is
int stage_in(GrowBuf& stage, const void* src, size_t bytes, int mem, hipStream_t s, const void** dev);
// `bytes` of a call's device words into host, after everything queued on s
inline int read_words(const void* ptr, size_t bytes, hipStream_t s, void* host) {
    CTG_CHECK(hipMemcpyAsync(host, ptr, bytes, hipMemcpyDeviceToHost, s));
    CTG_CHECK(hipStreamSynchronize(s));
    return CTG_OK;
}
// one u32 device word, after everything queued on s
int read_word(Workspace& w, SmallSlot i, hipStream_t s, int64_t* v);
// the phase times of a profiled call: scan, pack, sort, segment, reduce, nodes, total
int read_phase_times(Workspace& w, hipStream_t s);
// dense edge ends and nodes of r -> the labels of the sorted unique table U
hipError_t map_back(const ctg_result* U, ctg_result* r, hipStream_t s);
// n u64 values -> their sorted distinct values in out (room for n), the count
// in *count_dev (device); key bits [0, end_bit) are compared
hipError_t sort_unique_u64(Workspace& w, const uint64_t* in, int64_t n, uint64_t* out, uint32_t* count_dev,
                           hipStream_t s, unsigned end_bit = 64u);

// One call of an entry point that uses the device's workspace: the device lock
// (from construction, so the argument checks run under it), then begin(): the
// initialised workspace, the stream, and the result as `make` makes it
// (new_result: a bare handle; empty_result and its kin: the placeholders of a
// table without rows; none: the call has no handle, or makes it later).  The
// work follows, then end() -- or, with nothing to do, empty().
struct ApiCall {
    DevLock lock;
    int dev = 0;
    Workspace* wp = nullptr;
    hipStream_t s = nullptr;
    ResultPtr r;
    int begin(void* stream, ResultPtr (*make)(int) = nullptr) {
        dev = current_device();
        wp = &ws(dev);
        CTG_CHECK(ws_init(*wp));
        s = (hipStream_t)stream;
        if (make) r = make(dev);
        return CTG_OK;
    }
    Workspace& w() const { return *wp; }
    int empty(ResultPtr (*make)(int), ctg_result** out) {
        *out = make(dev).release();
        return CTG_OK;
    }
    // The epilogue: the phase times of a profiled call (timed: it ran the
    // phases), then the handle goes out.  table: a table scan, which ends
    // synchronised and leaves its record counts in the workspace.
    int end(bool timed, ctg_result** out, bool table = false) {
        if (wp->profiling && timed) {
            const int rc = read_phase_times(*wp, s);
            if (rc != CTG_OK) return rc;
        }
        if (table) {
            CTG_CHECK(hipStreamSynchronize(s));
            wp->last_records = r->n_records;
            wp->last_direct = r->n_direct;
        }
        *out = r.release();
        return CTG_OK;
    }
};

// a nested C-ABI call's handle, owned
template <class Call>
int nested(ResultPtr& r, Call&& call) {
    ctg_result* raw = nullptr;
    const int rc = call(&raw);
    r.reset(raw);
    return rc;
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

// The prologue of a dense-volume call (components, distance transform,
// watershed): open() is box_of plus what the entry points derive from the box;
// in() stages an array-sized input and out() opens the box-sized output, each
// of `width` bytes per element.  s is set once the call has begun.
struct DenseCall {
    const char* who;
    int mem;
    hipStream_t s = nullptr;
    CallBox box{};
    int64_t n[3] = {}, V = 0;   // the box's extent and voxels
    size_t elems = 0;           // the array's elements
    VolBox vol{};
    int open(const int64_t* shape, const int64_t* begin, const int64_t* end, int64_t max_voxels) {
        const int rc = box_of(who, shape, begin, end, max_voxels, &box);
        if (rc) return rc;
        for (int k = 0; k < 3; ++k) n[k] = box.e[k] - box.b[k];
        V = box.voxels;
        elems = (size_t)shape[0] * shape[1] * shape[2];
        vol = vol_box(shape, box);
        return CTG_OK;
    }
    template <class T>
    int in(DevInput<T>& d, const void* src, size_t width) const {
        return d.put((const T*)src, elems * width, mem, s, who);
    }
    template <class T>
    int out(DenseOut<T>& o, void* dst, size_t width) const {
        return hip_status(o.open((T*)dst, (size_t)V * width, mem, false, s), who);
    }
};

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
    hipError_t map_back(ctg_result* r, hipStream_t s) { return U ? ctg::map_back(U.get(), r, s) : hipSuccess; }
};

// One unique-label candidate pass, for a whole box and for the boxes of a
// batch: launch(cand, count, cap) queues the kernel that appends the candidate
// labels (one per tile and flush, so labels repeat) and counts them past cap;
// a pass that counted more than cap runs again with room for them, three
// attempts in all.  The candidates' sorted distinct values (key bits
// [0, end_bit)) come back in nodes, their number in *N.  cap: the first
// capacity; bound: candidate_cap_regrow's.
template <class Launch>
int unique_candidates(Workspace& w, int64_t cap, int64_t bound, unsigned end_bit, hipStream_t s,
                      const char* nomem_msg, const char* overflow_msg, Launch&& launch, DevBuf<uint64_t>& nodes,
                      int64_t* N) {
    for (int attempt = 0; attempt < 3; ++attempt) {
        DevBuf<uint64_t> cand(cap * 8);
        StreamWait wait{s};
        if (!cand || !nodes.alloc(cap * 8)) {
            set_error(nomem_msg);
            return CTG_ERR_NOMEM;
        }
        CTG_CHECK(hipMemsetAsync(w.counters, 0, sizeof(Counters), s));
        CTG_CHECK(launch((uint64_t*)cand, &w.counters->n_records, cap));
        CTG_CHECK(hipMemcpyAsync(w.counters_host, w.counters, sizeof(Counters), hipMemcpyDeviceToHost, s));
        CTG_CHECK(hipStreamSynchronize(s));
        const int64_t m = (int64_t)w.counters_host->n_records;
        if (m > cap) {
            wait.disarm();
            cap = candidate_cap_regrow(m, bound);
            nodes.reset();
            continue;
        }
        CTG_CHECK(sort_unique_u64(w, cand, m, nodes, w.small + SLOT_NODES, s, end_bit));
        const int rc = read_word(w, SLOT_NODES, s, N);
        if (rc == CTG_OK) wait.disarm();
        return rc;
    }
    set_error(overflow_msg);
    return CTG_ERR_NOMEM;
}

}  // namespace ctg
