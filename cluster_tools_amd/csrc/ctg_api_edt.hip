// C ABI of the exact Euclidean distance transform (include/ctg.h:
// ctg_distance_transform) over the kernels of ctg_edt.hip.  The host decisions
// -- which passes run, where each pass keeps its stacks, the grids -- are
// ctg_plan.h's (edt_passes, edt_line_plan, edt_x_grid).
#include <hip/hip_runtime.h>

#include <cmath>

#include "ctg_api.h"
#include "ctg_edt.h"

using namespace ctg;

extern "C" {

int ctg_distance_transform(const void* src, int src_kind, int src_bits, const int64_t* shape, const int64_t* begin,
                           const int64_t* end, double threshold, uint64_t label, const double* pitch, int flags,
                           void* out, int mem, void* stream, uint64_t* info) {
    const char* who = "ctg_distance_transform";
    ApiCall c;
    if (info) info[0] = info[1] = info[2] = info[3] = 0;
    if (!src || !shape || !out) {
        set_error("ctg_distance_transform: null argument");
        return CTG_ERR_ARG;
    }
    int kind = -1;   // launch_edt_x's
    if (src_kind == CTG_EDT_SRC_NONZERO && src_bits == 8) kind = 0;
    else if (src_kind == CTG_EDT_SRC_GREATER && src_bits == 32) kind = 1;
    else if (src_kind == CTG_EDT_SRC_EQUAL && (src_bits == 32 || src_bits == 64)) kind = src_bits == 32 ? 2 : 3;
    if (kind < 0) {
        set_error("ctg_distance_transform: src_kind / src_bits must be NONZERO / 8, GREATER / 32 or EQUAL / 32 or 64");
        return CTG_ERR_ARG;
    }
    if (flags & ~(CTG_EDT_TO_BACKGROUND | CTG_EDT_2D | CTG_EDT_OUT_D2)) {
        set_error("ctg_distance_transform: unknown flag");
        return CTG_ERR_ARG;
    }
    if (!mem_ok(who, mem)) return CTG_ERR_ARG;
    double p[3] = {1.0, 1.0, 1.0};
    for (int k = 0; pitch && k < 3; ++k) {
        p[k] = pitch[k];
        if (!std::isfinite(p[k]) || !(p[k] > 0.0)) {
            set_error("ctg_distance_transform: every pitch must be finite and positive");
            return CTG_ERR_ARG;
        }
    }
    DenseCall D{who, mem};
    int rc = D.open(shape, begin, end, EDT_MAX_VOXELS);
    if (rc) return rc;
    const int64_t* n = D.n;
    if (n[0] >= EDT_MAX_AXIS || n[1] >= EDT_MAX_AXIS || n[2] >= EDT_MAX_AXIS) {
        set_error("ctg_distance_transform: boxes with an axis of 32768 or more are not supported");
        return CTG_ERR_UNSUPPORTED;
    }
    const int64_t V = D.V;
    if (V == 0) return CTG_OK;
    if ((rc = c.begin(stream)) != CTG_OK) return rc;
    hipStream_t s = D.s = c.s;
    const bool two_d = (flags & CTG_EDT_2D) != 0, out_d2 = (flags & CTG_EDT_OUT_D2) != 0;
    const EdtPasses passes = edt_passes(n, two_d);
    // the last pass writes the result: the z pass, or the y pass where there is none
    const EdtLinePlan py = edt_line_plan(n[1], n[0], n[2]), pz = edt_line_plan(n[0], n[1], n[2]);
    const EdtLinePlan& last = passes.z ? pz : py;
    DevInput<char> ds;
    DenseOut<char> o;
    DevBuf<uint16_t> dx;
    DevBuf<uint32_t> dyx;
    DevBuf<uint64_t> stack;
    DevBuf<unsigned long long> words;   // info[4], then the last pass's partials
    StreamWait wait{s};
    if ((rc = D.in(ds, src, (size_t)(src_bits / 8))) != CTG_OK) return rc;
    const int64_t stack_bytes = std::max<int64_t>(passes.y ? py.stack_bytes : 0, passes.z ? pz.stack_bytes : 0);
    if (!dx.alloc((size_t)V * 2) || (passes.y && passes.z && !dyx.alloc((size_t)V * 4)) ||
        (stack_bytes && !stack.alloc((size_t)stack_bytes)) ||
        !words.alloc((size_t)(4 + last.grid * EDT_PART_WORDS) * 8))
        return hip_status(hipErrorOutOfMemory, who);
    if ((rc = D.out(o, out, out_d2 ? 8 : 4)) != CTG_OK) return rc;
    CTG_CHECK(hipMemsetAsync(words.p, 0, 4 * 8, s));
    EdtSrc A{};
    A.src = ds.p;
    A.box = D.vol;
    A.threshold = (float)threshold;
    A.label = label;
    A.invert = (flags & CTG_EDT_TO_BACKGROUND) != 0;
    EdtLineArgs L{};
    for (int k = 0; k < 3; ++k) {
        L.n[k] = A.box.n[k];
        L.p[k] = p[k];
    }
    L.diag2 = edt_diag2(n, p, two_d);
    L.stack = stack;
    L.out_d2 = out_d2;
    L.part = words.p + 4;
    Ev ev{c.w(), s};
    ev.mark(0);
    CTG_CHECK(launch_edt_x(A, kind, dx, words, s));
    ev.mark(1);
    if (passes.y) {
        L.in = dx.p;
        L.in32 = 0;
        L.axis = 1;
        L.final_pass = !passes.z;
        L.out = passes.z ? (void*)dyx.p : (void*)o.d;
        CTG_CHECK(launch_edt_line(L, py, s));
    }
    ev.mark(2);
    if (passes.z) {
        L.in = passes.y ? (const void*)dyx.p : (const void*)dx.p;
        L.in32 = passes.y;
        L.axis = 0;
        L.final_pass = 1;
        L.out = o.d;
        CTG_CHECK(launch_edt_line(L, pz, s));
    }
    CTG_CHECK(launch_edt_fold(L.part, last.grid, words, s));
    ev.mark(3);
    ev.mark(4);
    ev.mark(5);
    ev.mark(6);
    CTG_CHECK(o.copy_back(s));
    if (info) CTG_CHECK(hipMemcpyAsync(info, words.p, 4 * 8, hipMemcpyDeviceToHost, s));
    // always waited for, a device-resident call without info too
    CTG_CHECK(hipStreamSynchronize(s));
    if (c.w().profiling && (rc = read_phase_times(c.w(), s)) != CTG_OK) return rc;
    return CTG_OK;
}

}  // extern "C"
