// Host check of the face scan's FAST40 histogram slot (sample_slot<true>,
// csrc/ctg_stats.h) for tests/test_slot_exact.py: every one of the 2^32 float
// bit patterns goes through the new rule, through the compare / select ladder
// it replaced (kept here as the reference) and through hist_slot for the
// default [0, 1] range (scale 40, offset 0); the three must agree.  Prints
// "checked N", "mismatch_ladder N", "mismatch_hist_slot N" and the first few
// differing patterns; exit status 1 on any mismatch.
//
// Host code only (the conversion's device form, v_cvt_i32_f64, is spelt out in
// trunc_sat_i32's host branch):
//   hipcc -O2 -std=c++17 --offload-host-only tools/slot_exact.hip -o slot_exact -lpthread
#include "../cluster_tools_amd/csrc/ctg_stats.h"

#include <atomic>
#include <cstdio>
#include <cstring>
#include <thread>
#include <vector>

// sample_slot<true> as it stood before the integer clamp: trunc + 1, then four
// compare / select pairs (left outlier, right outlier, NaN, m == 40)
static inline int ladder40(double dx) {
    const double m = dx * 40.0;
    int s = (int)((unsigned)ctg::trunc_sat_i32(m) + 1u);   // (wraps at saturation, as the device add does)
    s = m <= -1.0 ? 0 : s;
    s = !(m < (double)ctg::NBINS) ? ctg::NBINS + 1 : s;
    s = m != m ? 0 : s;
    return m == (double)ctg::NBINS ? ctg::NBINS : s;
}

int main() {
    const unsigned hw = std::thread::hardware_concurrency();
    const unsigned nt = hw == 0 ? 1u : (hw > 16u ? 16u : hw);
    std::atomic<unsigned long long> bad_ladder{0}, bad_hist{0}, checked{0};
    std::atomic<int> shown{0};
    std::vector<std::thread> th;
    for (unsigned t = 0; t < nt; ++t) {
        th.emplace_back([&, t]() {
            const unsigned long long total = 1ull << 32;
            const unsigned long long b0 = total * t / nt, b1 = total * (t + 1) / nt;
            unsigned long long bl = 0, bh = 0;
            for (unsigned long long b = b0; b < b1; ++b) {
                const uint32_t bits = (uint32_t)b;
                float x;
                std::memcpy(&x, &bits, 4);
                const double dx = (double)x;
                const int s = ctg::sample_slot<true>(dx, 40.0, 0.0);
                const int l = ladder40(dx);
                const int h = ctg::hist_slot(dx, 40.0, 0.0);
                if (s != l || s != h) {
                    bl += s != l;
                    bh += s != h;
                    if (shown.fetch_add(1) < 8)
                        std::fprintf(stderr, "bits %08x (%.9g): new %d, ladder %d, hist_slot %d\n", bits, (double)x, s,
                                     l, h);
                }
            }
            bad_ladder += bl;
            bad_hist += bh;
            checked += b1 - b0;
        });
    }
    for (auto& t : th) t.join();
    std::printf("checked %llu\nmismatch_ladder %llu\nmismatch_hist_slot %llu\n", checked.load(), bad_ladder.load(),
                bad_hist.load());
    return (bad_ladder.load() || bad_hist.load()) ? 1 : 0;
}
