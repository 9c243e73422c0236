// Host-side check that vigra_quantiles_cross (crossing search) and
// vigra_quantiles (keypoint walk) give bit-identical quantiles.
// build: hipcc -O2 -std=c++17 --offload-arch=gfx950 tools/quantile_fuzz.hip -o /tmp/qfuzz && /tmp/qfuzz
//
// --dump N SEED: N seeded cases of float32 samples binned with ctg::hist_slot
// and finalised with vigra_quantiles_cross, one line each, for the Python
// oracle to re-derive (tests/test_abi.py::test_host_statistics_match_python_oracle):
//   kind lo hi n min max, the 42 slots, q10 q25 q50 q75 q90, the n samples' f32 bits (hex); blank-separated
// kind 0..2: ranges [0,1], [-1,2], [-0.37,0.91]; kind 3: u8 samples k/255 on [0,1].
#include "../cluster_tools_amd/csrc/ctg_reduce.hip"
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>

static int dump(long n_cases, uint64_t seed) {
    std::mt19937_64 rng(seed);
    static const double LO[4] = {0.0, -1.0, -0.37, 0.0}, HI[4] = {1.0, 2.0, 0.91, 1.0};
    auto unit = [&]() { return (double)(rng() >> 11) * (1.0 / 9007199254740992.0); };
    for (long it = 0; it < n_cases; ++it) {
        const int kind = (int)(it % 4);
        const double lo = LO[kind], hi = HI[kind], w = hi - lo;
        const double scale = (double)ctg::NBINS / w, offset = lo;   // as ctg_rag_features sets them
        const int shape = (int)(rng() % 4);   // 0: any sample kind, 1: edges and their neighbours only,
                                              // 2: one to three bins, 3: few samples
        const int n = 1 + (int)(rng() % (shape == 3 ? 4 : 48));
        const int k0 = (int)(rng() % ctg::NBINS), nk = 1 + (int)(rng() % 3);
        float x[48];
        uint32_t h[ctg::NSLOTS] = {0};
        for (int j = 0; j < n; ++j) {
            float v;
            if (kind == 3) {
                v = (float)(rng() % 256) / 255.0f;
            } else {
                const int pick = shape == 1 ? 1 + (int)(rng() % 3) : (int)(rng() % 7);
                const int k = shape == 2 ? std::min(k0 + (int)(rng() % nk), (int)ctg::NBINS) : (int)(rng() % (ctg::NBINS + 1));
                const float edge = (float)(lo + (double)k * w / (double)ctg::NBINS);
                if (pick == 0 || (shape == 2 && pick > 3)) v = (float)(lo + ((double)k + unit()) * w / (double)ctg::NBINS);
                else if (pick == 1) v = edge;
                else if (pick == 2) v = std::nextafterf(edge, INFINITY);
                else if (pick == 3) v = std::nextafterf(edge, -INFINITY);
                else if (pick == 4) v = (float)(lo - unit() * w);                               // left of the range
                else if (pick == 5) v = (float)(hi + unit() * w);                               // right of the range
                else v = (float)(lo - unit() * w / (double)ctg::NBINS);                         // (-1, 0] bins: bin 0
            }
            x[j] = v;
            ++h[ctg::hist_slot((double)v, scale, offset)];
        }
        float mn = x[0], mx = x[0];
        for (int j = 1; j < n; ++j) {
            mn = std::fmin(mn, x[j]);
            mx = std::fmax(mx, x[j]);
        }
        double q[5] = {0, 0, 0, 0, 0};
        ctg::vigra_quantiles_cross(h, (double)n, (double)mn, (double)mx, scale, offset, q);
        std::printf("%d %.17g %.17g %d %.17g %.17g", kind, lo, hi, n, (double)mn, (double)mx);
        for (int s = 0; s < ctg::NSLOTS; ++s) std::printf(" %u", h[s]);
        for (int i = 0; i < 5; ++i) std::printf(" %.17g", q[i]);
        for (int j = 0; j < n; ++j) {
            uint32_t b;
            std::memcpy(&b, &x[j], 4);
            std::printf(" %08x", b);
        }
        std::printf("\n");
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 4 && std::strcmp(argv[1], "--dump") == 0)
        return dump(std::atol(argv[2]), (uint64_t)std::strtoull(argv[3], nullptr, 10));
    std::mt19937_64 rng(12345);
    long bad = 0, n = 0;
    for (int it = 0; it < 2000000; ++it) {
        uint32_t h[ctg::NSLOTS] = {0};
        const int mode = it % 7;
        const int nz = 1 + (int)(rng() % (mode == 0 ? 1 : mode == 1 ? 3 : 42));
        for (int j = 0; j < nz; ++j) {
            int slot = (int)(rng() % ctg::NSLOTS);
            if (mode == 2 && (slot == 0 || slot == ctg::NSLOTS - 1)) slot = 1 + (int)(rng() % ctg::NBINS);
            h[slot] += 1 + (uint32_t)(rng() % (mode == 3 ? 3 : 2000));
        }
        uint64_t cnt = 0;
        int lo = -1, hi = -1;
        for (int s = 0; s < ctg::NSLOTS; ++s) {
            cnt += h[s];
            if (h[s]) { if (lo < 0) lo = s; hi = s; }
        }
        std::uniform_real_distribution<double> U(0.0, 1.0);
        auto in_slot = [&](int s, bool low) {
            if (s == 0) return -U(rng) * 3.0;
            if (s == ctg::NSLOTS - 1) return 1.0 + 1e-6 + U(rng) * 3.0;
            const int k = s - 1;
            const int r = (int)(rng() % 4);
            if (r == 0) return (double)(float)(k / 40.0);                      // bin edge
            if (r == 1 && k == ctg::NBINS - 1 && !low) return 1.0;            // top edge maps into bin 39
            return (double)(float)((k + U(rng)) / 40.0);
        };
        double vmin = in_slot(lo, true), vmax = in_slot(hi, false);
        if (lo == hi && vmin > vmax) std::swap(vmin, vmax);
        const double scale = (mode == 6) ? 40.0 / 255.0 : 40.0, offset = (mode == 6) ? 0.0 : 0.0;
        if (mode == 6) { vmin *= 255.0; vmax *= 255.0; }
        double a[5] = {0, 0, 0, 0, 0}, b[5] = {0, 0, 0, 0, 0};
        ctg::vigra_quantiles(h, (double)cnt, vmin, vmax, scale, offset, a);
        ctg::vigra_quantiles_cross(h, (double)cnt, vmin, vmax, scale, offset, b);
        ++n;
        if (std::memcmp(a, b, sizeof a) != 0) {
            if (bad < 10) {
                std::printf("mismatch it=%d mode=%d cnt=%llu vmin=%.17g vmax=%.17g lo=%d hi=%d\n", it, mode,
                            (unsigned long long)cnt, vmin, vmax, lo, hi);
                for (int q = 0; q < 5; ++q) std::printf("  q%d walk=%.17g cross=%.17g\n", q, a[q], b[q]);
            }
            ++bad;
        }
    }
    std::printf("%ld / %ld mismatches\n", bad, n);
    return bad != 0;
}
