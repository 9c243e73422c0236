// Host rendering of the seeded watershed: the rounds of ctg_ws.hip run serially
// over the very functions the kernels call (csrc/ctg_ws.h: the key, the order,
// the pick, the hook, the chase) and the plan functions of csrc/ctg_plan.h.
// Built with the host compiler and -fsanitize=address,undefined by
// tests/test_ws_host.py, which compares its answers with the oracles of
// tests/ws_cases.py.  One query per line on stdin, one answer per line:
//
//   key BITS                  -> ws_key_bits of a float32's bits
//   cap U                     -> ws_round_cap(U)
//   plan NZ NY NX TWO_D       -> voxels grid parent key best pick slices (bytes)
//   flood TWO_D NZ NY NX h.. s..   heights as float32 bits, seeds as u64
//                             -> rounds chase_launches label..
#include <cstdint>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../cluster_tools_amd/csrc/ctg_plan.h"
#include "../cluster_tools_amd/csrc/ctg_ws.h"

using namespace ctg;

namespace {

struct Flood {
    WsBox B;
    std::vector<uint32_t> parent, key, pick;
    std::vector<uint64_t> best;
    int rounds = 0, launches = 0;
};

// false: a cap was passed
bool flood(Flood& f, const std::vector<uint64_t>& seeds) {
    const uint32_t V = (uint32_t)seeds.size();
    const auto par = [&](uint32_t u) { return f.parent.at(u); };
    const auto key = [&](uint32_t u) { return f.key.at(u); };
    const auto picked = [&](uint32_t u) { return f.pick.at(u); };
    const auto load = [](const uint32_t* p) { return *p; };
    int64_t U = 0;
    for (uint32_t i = 0; i < V; ++i) {   // k_ws_init
        f.parent[i] = seeds[i] ? i | WS_SEEDED : i;
        f.best[i] = WS_NO_KEY;
        f.pick[i] = WS_NO_EDGE;
        U += seeds[i] == 0;
    }
    if (U == V) return true;   // no seed: nothing to flood from
    const int cap = ws_round_cap(U);
    bool finished = U == 0;
    for (int round = 0; round < cap && !finished; ++round) {
        ++f.rounds;
        for (int pass = 0; pass < 2; ++pass)   // k_ws_pick<0>, <1>
            for (uint32_t i = 0; i < V; ++i) {
                const uint32_t r = f.parent[i];
                if (r & WS_SEEDED) continue;
                const WsEdge e = ws_voxel_pick(f.B, i, r, par, key);
                if (e.key == WS_NO_KEY) continue;
                if (pass == 0) f.best.at(r) = std::min(f.best.at(r), e.key);
                else if (f.best.at(r) == e.key) f.pick.at(r) = std::min(f.pick.at(r), e.id);
            }
        int64_t hooks = 0;
        for (uint32_t i = 0; i < V; ++i) {   // k_ws_hook
            if (f.parent[i] != i || f.pick[i] == WS_NO_EDGE) continue;
            if ((int64_t)(f.pick[i] / 3u) + ws_axis_step(f.B, (int)(f.pick[i] % 3u)) >= V) return false;
            const uint32_t t = ws_hook(f.B, i, f.pick[i], par, picked);
            f.best[i] = t;
            hooks += t != i;
        }
        if (hooks == 0) {
            finished = true;
            break;
        }
        for (uint32_t i = 0; i < V; ++i) {   // k_ws_apply
            if (f.parent[i] != i || f.pick[i] == WS_NO_EDGE) continue;
            f.parent[i] = (uint32_t)f.best[i];
            f.best[i] = WS_NO_KEY;
            f.pick[i] = WS_NO_EDGE;
        }
        for (int k = 0;; ++k) {   // k_ws_chase
            if (k == WS_CHASE_LAUNCHES) return false;
            bool done = true;
            // (from the far end, so that the serial run does not flatten every chain on its way)
            for (uint32_t j = V; j-- > 0;) {
                const uint32_t x = f.parent[j];
                if (x == j || (x & WS_SEEDED)) continue;
                f.parent[j] = ws_chase(f.parent.data(), x, load, &done);
            }
            f.launches = std::max(f.launches, k + 1);
            if (done) break;
        }
    }
    return finished;
}

}  // namespace

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd;
        in >> cmd;
        if (cmd == "key") {
            uint32_t b;
            in >> b;
            std::printf("%u\n", ws_key_bits(b));
        } else if (cmd == "cap") {
            int64_t u;
            in >> u;
            std::printf("%d\n", ws_round_cap(u));
        } else if (cmd == "plan") {
            int64_t n[3];
            int two_d;
            in >> n[0] >> n[1] >> n[2] >> two_d;
            const WsPlan p = ws_plan(n, two_d != 0);
            std::printf("%lld %lld %lld %lld %lld %lld %lld\n", (long long)p.voxels, (long long)p.grid,
                        (long long)p.parent_bytes, (long long)p.key_bytes, (long long)p.best_bytes,
                        (long long)p.pick_bytes, (long long)p.slices);
        } else if (cmd == "flood") {
            int two_d;
            int64_t n[3];
            in >> two_d >> n[0] >> n[1] >> n[2];
            const int64_t V = n[0] * n[1] * n[2];
            if (V <= 0 || V > (1 << 24)) return 2;
            Flood f;
            f.B = WsBox{{(uint32_t)n[0], (uint32_t)n[1], (uint32_t)n[2]}, two_d};
            f.parent.resize(V);
            f.key.resize(V);
            f.pick.resize(V);
            f.best.resize(V);
            std::vector<uint64_t> seeds(V);
            for (int64_t i = 0; i < V; ++i) {
                uint32_t b;
                in >> b;
                f.key[i] = ws_key_bits(b);
            }
            for (int64_t i = 0; i < V; ++i) in >> seeds[i];
            if (!in) return 2;
            if (!flood(f, seeds)) return 3;
            std::string out = std::to_string(f.rounds) + " " + std::to_string(f.launches);
            for (int64_t i = 0; i < V; ++i) {
                const uint32_t p = f.parent[i];
                out += ' ';
                out += std::to_string((p & WS_SEEDED) ? seeds[p & WS_INDEX] : 0ull);
            }
            std::puts(out.c_str());
        } else if (!cmd.empty()) {
            return 2;
        }
    }
    return 0;
}
