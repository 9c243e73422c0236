// Host rendering of the exact Euclidean distance transform: the three passes
// of csrc/ctg_edt.hip run serially over the functions the kernels share
// (csrc/ctg_edt.h: the row's seed words and their nearest-seed lookups, the
// envelope's push and seek, D2 and the diagonal) and the plan functions of
// csrc/ctg_plan.h.  Built by tests/test_edt_host.py with the host compiler and
// -fsanitize=address,undefined.  One query per input line, one answer line each:
//
//   plan LINE OUTER NX          -> lds groups grid stack_bytes
//   passes NZ NY NX TWO_D       -> y z
//   xgrid ROWS                  -> workgroups of the x pass (edt_x_grid)
//   edt NZ NY NX PZ PY PX TWO_D BITS
//                               BITS: NZ*NY*NX characters 0 / 1, 1 a seed; the pitches as
//                               C hexadecimal floats.  -> n_seeds n_unseeded argmax d2
//                               (float64 bits, hex) and the float32 result's bits (hex)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../cluster_tools_amd/csrc/ctg_edt.h"
#include "../cluster_tools_amd/csrc/ctg_plan.h"

using namespace ctg;

namespace {

struct VecStack {   // a lane's stack of `cap` entries; an access past it is the sanitizer's to report
    std::vector<EdtEntry> e;
    explicit VecStack(int cap) : e((size_t)cap) {}
    EdtEntry get(int k) const { return e.at((size_t)k); }
    void set(int k, EdtEntry v) { e.at((size_t)k) = v; }
};

struct Fold {   // the last pass's arg-max and unseeded count
    double best = -1.0;
    uint32_t best_i = 0;
    uint64_t unseeded = 0;
    void offer(double d2, int64_t i) {
        if (d2 > best || (d2 == best && (uint32_t)i < best_i)) {
            best = d2;
            best_i = (uint32_t)i;
        }
    }
};

// the x pass: a row's ballots as words, the bits above them, the lookups
void pass_x(const std::string& bits, const int64_t* n, std::vector<uint16_t>& dx, uint64_t* seeds) {
    const int nx = (int)n[2], nw = (nx + 63) >> 6, ns = (nw + 63) >> 6;
    std::vector<uint64_t> W((size_t)nw), S((size_t)ns);
    for (int64_t row = 0; row < n[0] * n[1]; ++row) {
        for (int w = 0; w < nw; ++w) {
            uint64_t m = 0;
            for (int lane = 0; lane < 64; ++lane) {
                const int x = (w << 6) + lane;
                if (x < nx && bits[(size_t)(row * nx + x)] == '1') m |= 1ull << lane;
            }
            W[(size_t)w] = m;
            *seeds += (uint64_t)__builtin_popcountll(m);
        }
        for (int sw = 0; sw < ns; ++sw) {
            uint64_t m = 0;
            for (int lane = 0; lane < 64; ++lane) {
                const int w = (sw << 6) + lane;
                if (w < nw && W[(size_t)w] != 0) m |= 1ull << lane;
            }
            S[(size_t)sw] = m;
        }
        for (int x = 0; x < nx; ++x) dx[(size_t)(row * nx + x)] = (uint16_t)edt_row_distance(W.data(), S.data(), ns, x);
    }
}

// one envelope pass, column by column, as k_edt_line takes them
void pass_line(const void* in, bool in32, void* out, bool final_pass, int axis, const int64_t* n, const double* p,
               double diag2, Fold* F) {
    const int64_t nx = n[2], plane = n[1] * nx;
    const int len = (int)n[axis];
    const int64_t step = axis == 1 ? nx : plane, outer_stride = axis == 1 ? plane : nx;
    const int64_t outer = axis == 1 ? n[0] : n[1];
    const EdtAxis X{p[1], p[2], p[axis] * p[axis], len};
    for (int64_t o = 0; o < outer; ++o) {
        for (int64_t x = 0; x < nx; ++x) {
            const int64_t base = o * outer_stride + x;
            VecStack S(len);
            int k = -1;
            EdtEntry top = 0;
            for (int q = 0; q < len; ++q) {
                const uint32_t v = in32 ? ((const uint32_t*)in)[base + q * step] : ((const uint16_t*)in)[base + q * step];
                if (v == (in32 ? EDT_NONE32 : EDT_NONE16)) continue;
                if (in32) edt_push(S, k, top, (uint32_t)q, v & 0xFFFFu, v >> 16, X);
                else edt_push(S, k, top, (uint32_t)q, 0u, v, X);
            }
            if (k < 0) {
                for (int t = 0; t < len; ++t) {
                    const int64_t i = base + t * step;
                    if (final_pass) {
                        ((float*)out)[i] = (float)std::sqrt(diag2);
                        F->offer(diag2, i);
                    } else {
                        ((uint32_t*)out)[i] = EDT_NONE32;
                    }
                }
                if (final_pass) F->unseeded += (uint64_t)len;
                continue;
            }
            int j = 0;
            EdtEntry cur = S.get(0), nxt = edt_next(S, k, 0);
            for (int t = 0; t < len; ++t) {
                edt_seek(S, k, j, cur, nxt, (uint32_t)t);
                const int64_t i = base + t * step;
                const uint32_t q = edt_q(cur), d = (uint32_t)t > q ? (uint32_t)t - q : q - (uint32_t)t;
                if (final_pass) {
                    const double d2 = axis == 1 ? edt_d2(0u, d, edt_b(cur), p) : edt_d2(d, edt_a(cur), edt_b(cur), p);
                    ((float*)out)[i] = (float)std::sqrt(d2);
                    F->offer(d2, i);
                } else {
                    ((uint32_t*)out)[i] = d | (edt_b(cur) << 16);
                }
            }
        }
    }
}

std::string run_edt(std::istringstream& is) {
    int64_t n[3];
    double p[3];
    std::string ps[3], bits;
    int two_d = 0;
    is >> n[0] >> n[1] >> n[2] >> ps[0] >> ps[1] >> ps[2] >> two_d >> bits;
    for (int k = 0; k < 3; ++k) p[k] = std::strtod(ps[k].c_str(), nullptr);
    const int64_t V = n[0] * n[1] * n[2];
    if (!is || V <= 0 || (int64_t)bits.size() != V) return "bad";
    std::vector<uint16_t> dx((size_t)V);
    std::vector<uint32_t> dyx;
    std::vector<float> out((size_t)V);
    uint64_t seeds = 0;
    Fold F;
    pass_x(bits, n, dx, &seeds);
    const EdtPasses passes = edt_passes(n, two_d != 0);
    const double diag2 = edt_diag2(n, p, two_d != 0);
    if (passes.y) {
        if (passes.z) dyx.resize((size_t)V);
        pass_line(dx.data(), false, passes.z ? (void*)dyx.data() : (void*)out.data(), !passes.z, 1, n, p, diag2, &F);
    }
    if (passes.z)
        pass_line(passes.y ? (const void*)dyx.data() : (const void*)dx.data(), passes.y, out.data(), true, 0, n, p, diag2, &F);
    uint64_t d2bits;
    std::memcpy(&d2bits, &F.best, 8);
    std::string r;
    char buf[96];
    std::snprintf(buf, sizeof buf, "%llu %llu %u %llx", (unsigned long long)seeds, (unsigned long long)F.unseeded,
                  F.best_i, (unsigned long long)d2bits);
    r = buf;
    for (float f : out) {
        uint32_t b;
        std::memcpy(&b, &f, 4);
        std::snprintf(buf, sizeof buf, " %x", b);
        r += buf;
    }
    return r;
}

}  // namespace

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream is(line);
        std::string cmd;
        is >> cmd;
        if (cmd == "plan") {
            int64_t len, outer, nx;
            is >> len >> outer >> nx;
            const EdtLinePlan P = edt_line_plan(len, outer, nx);
            std::printf("%d %lld %lld %lld\n", P.lds, (long long)P.groups, (long long)P.grid, (long long)P.stack_bytes);
        } else if (cmd == "passes") {
            int64_t n[3];
            int two_d;
            is >> n[0] >> n[1] >> n[2] >> two_d;
            const EdtPasses P = edt_passes(n, two_d != 0);
            std::printf("%d %d\n", (int)P.y, (int)P.z);
        } else if (cmd == "xgrid") {
            int64_t rows;
            is >> rows;
            std::printf("%lld\n", (long long)edt_x_grid(rows));
        } else if (cmd == "edt") {
            std::printf("%s\n", run_edt(is).c_str());
        } else {
            std::printf("unknown\n");
        }
    }
    return 0;
}
