// Host driver of csrc/ctg_uf.h (the union-find and the run-head bit helpers the
// kernels of ctg_cc.hip run) and of the labelling's plan functions
// (csrc/ctg_plan.h: cc_neighbor_rows, cc_grid, cc_seam_voxel, cc_seam_partner,
// cc_segments) for tests/test_cc_host.py: reads one query per line from stdin
// and prints the answer, one line each.
//
//   rows C                         -> n, then dz dy dil per neighbour row
//   grid NZ NY NX                  -> tiles z y x, seam threads x y z, segments
//   label C NZ NY NX v...          -> n, then the labels: a serial rendering of the
//                                     tile, seam, flatten and number steps over the
//                                     0 / 1 volume v (C order)
//   merge N_LABELS N a b a b ...   -> max_id, then the table; `bad` for a member that
//                                     is 0 or not below N_LABELS
//   find CAP x p...                -> over root: uf_find on the parent array p
//
// The device's atomics are a plain load and a plain compare-and-store here.
//
// g++ -std=c++17 -fsanitize=address,undefined tools/cc_check.cpp -o cc_check
#include <cinttypes>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../cluster_tools_amd/csrc/ctg_plan.h"
#include "../cluster_tools_amd/csrc/ctg_uf.h"

using namespace ctg;

static uint32_t load(const uint32_t* p) { return *p; }
static uint32_t amin(uint32_t* p, uint32_t v) {
    const uint32_t old = *p;
    if (v < old) *p = v;
    return old;
}

// k_cc_tile: the tile (tz, ty, tx) of the box n of the 0 / 1 volume vol into parent
static void tile_step(int conn, const int64_t* n, const std::vector<int>& vol, int64_t tz, int64_t ty, int64_t tx,
                      std::vector<uint32_t>& parent, int* over) {
    std::vector<uint64_t> bits(CC_ROWS, 0);
    std::vector<uint32_t> par((size_t)CC_ROWS * TILE_X, UF_NONE);
    for (int z = 0; z < CC_TILE_Z; ++z)
        for (int y = 0; y < CC_TILE_Y; ++y) {
            const int64_t gz = tz * CC_TILE_Z + z, gy = ty * CC_TILE_Y + y;
            uint64_t m = 0;
            for (int x = 0; x < TILE_X; ++x) {
                const int64_t gx = tx * TILE_X + x;
                if (gz < n[0] && gy < n[1] && gx < n[2] && vol[(size_t)((gz * n[1] + gy) * n[2] + gx)]) m |= 1ull << x;
            }
            const int r = z * CC_TILE_Y + y;
            bits[r] = m;
            for (int x = 0; x < TILE_X; ++x)
                if ((run_starts(m) >> x) & 1) par[r * TILE_X + x] = (uint32_t)(r * TILE_X + x);
        }
    const CcRows R = cc_neighbor_rows(conn);
    const uint32_t cap = CC_ROWS * TILE_X;
    for (int z = 0; z < CC_TILE_Z; ++z)
        for (int y = 0; y < CC_TILE_Y; ++y) {
            const int r = z * CC_TILE_Y + y;
            const uint64_t m = bits[r];
            for (int k = 0; k < R.n; ++k) {
                const int z2 = z + R.dz[k], y2 = y + R.dy[k];
                if (z2 < 0 || y2 < 0 || y2 >= CC_TILE_Y) continue;
                const int r2 = z2 * CC_TILE_Y + y2;
                const uint64_t m2 = bits[r2];
                for (int x = 0; x < TILE_X; ++x) {
                    if ((contact_same(m, m2) >> x) & 1)
                        uf_union(par.data(), (uint32_t)(r * TILE_X + run_head(m, x)),
                                 (uint32_t)(r2 * TILE_X + run_head(m2, x)), cap, load, amin, over);
                    if (!R.dil[k]) continue;
                    if ((contact_up(m, m2) >> x) & 1)
                        uf_union(par.data(), (uint32_t)(r * TILE_X + x), (uint32_t)(r2 * TILE_X + run_head(m2, x - 1)), cap,
                                 load, amin, over);
                    if ((contact_down(m, m2) >> x) & 1)
                        uf_union(par.data(), (uint32_t)(r * TILE_X + run_head(m, x)), (uint32_t)(r2 * TILE_X + x + 1), cap,
                                 load, amin, over);
                }
            }
        }
    for (int z = 0; z < CC_TILE_Z; ++z)
        for (int y = 0; y < CC_TILE_Y; ++y)
            for (int x = 0; x < TILE_X; ++x) {
                const int64_t gz = tz * CC_TILE_Z + z, gy = ty * CC_TILE_Y + y, gx = tx * TILE_X + x;
                if (gz >= n[0] || gy >= n[1] || gx >= n[2]) continue;
                const int r = z * CC_TILE_Y + y;
                uint32_t val = UF_NONE;
                if ((bits[r] >> x) & 1) {
                    const uint32_t root = uf_find(par.data(), (uint32_t)(r * TILE_X + run_head(bits[r], x)), cap, load, over);
                    const int64_t lz = root / (CC_TILE_Y * TILE_X), ly = (root / TILE_X) % CC_TILE_Y, lx = root % TILE_X;
                    val = (uint32_t)(((tz * CC_TILE_Z + lz) * n[1] + ty * CC_TILE_Y + ly) * n[2] + tx * TILE_X + lx);
                }
                parent[(size_t)((gz * n[1] + gy) * n[2] + gx)] = val;
            }
}

// k_cc_seams
static void seam_step(int conn, const int64_t* n, const CcGrid& g, std::vector<uint32_t>& parent, int* over) {
    const uint32_t cap = (uint32_t)parent.size();
    for (int64_t i = 0; i < g.seam_threads; ++i) {
        const CcSeamVoxel v = cc_seam_voxel(g, n[1], n[2], i);
        if (!v.take) continue;
        const uint32_t me = parent[(size_t)((v.z * n[1] + v.y) * n[2] + v.x)];
        if (me == UF_NONE) continue;
        for (int dz = -1; dz <= 1; ++dz)
            for (int dy = -1; dy <= 1; ++dy)
                for (int dx = -1; dx <= 1; ++dx) {
                    if (!cc_seam_partner(conn, v.z, v.y, v.x, dz, dy, dx)) continue;
                    const int64_t qz = v.z + dz, qy = v.y + dy, qx = v.x + dx;
                    if (qz < 0 || qy < 0 || qx < 0 || qz >= n[0] || qy >= n[1] || qx >= n[2]) continue;
                    const uint32_t other = parent[(size_t)((qz * n[1] + qy) * n[2] + qx)];
                    if (other == UF_NONE) continue;
                    uf_union(parent.data(), me, other, cap, load, amin, over);
                }
    }
}

// k_uf_flatten, k_uf_scan, k_uf_write: ids[i] = rank of i's root among all roots + plus, 0 for UF_NONE
static uint64_t number_step(std::vector<uint32_t>& parent, uint64_t plus, std::vector<uint64_t>& ids, int* over) {
    const int64_t n = (int64_t)parent.size(), segs = cc_segments(n);
    std::vector<uint32_t> rank((size_t)n, 0), seg((size_t)segs + 1, 0);
    for (int64_t sg = 0; sg < segs; ++sg) {
        uint32_t run = 0;
        for (int64_t p = sg * CC_SEG; p < std::min(n, (sg + 1) * CC_SEG); ++p) {
            if (parent[(size_t)p] == UF_NONE) continue;
            const uint32_t r = uf_find(parent.data(), parent[(size_t)p], (uint32_t)n, load, over);
            parent[(size_t)p] = r;
            if (r == (uint32_t)p) rank[(size_t)p] = run++;
        }
        seg[(size_t)sg] = run;
    }
    uint32_t total = 0;
    for (int64_t sg = 0; sg < segs; ++sg) {
        const uint32_t c = seg[(size_t)sg];
        seg[(size_t)sg] = total;
        total += c;
    }
    ids.assign((size_t)n, 0);
    for (int64_t i = 0; i < n; ++i) {
        const uint32_t r = parent[(size_t)i];
        if (r != UF_NONE) ids[(size_t)i] = (uint64_t)seg[(size_t)(r / CC_SEG)] + rank[r] + plus;
    }
    return total;
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd;
        if (!(in >> cmd)) continue;
        if (cmd == "rows") {
            int c;
            in >> c;
            const CcRows R = cc_neighbor_rows(c);
            printf("%d", R.n);
            for (int k = 0; k < R.n; ++k) printf(" %d %d %d", R.dz[k], R.dy[k], R.dil[k]);
            printf("\n");
        } else if (cmd == "grid") {
            int64_t n[3];
            in >> n[0] >> n[1] >> n[2];
            const CcGrid g = cc_grid(n);
            printf("%" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 "\n", g.nt[0], g.nt[1],
                   g.nt[2], g.seam[0], g.seam[1], g.seam[2], g.segs);
        } else if (cmd == "label") {
            int conn;
            int64_t n[3];
            in >> conn >> n[0] >> n[1] >> n[2];
            std::vector<int> vol((size_t)(n[0] * n[1] * n[2]));
            for (int& v : vol) in >> v;
            const CcGrid g = cc_grid(n);
            std::vector<uint32_t> parent(vol.size(), UF_NONE);
            int over = 0;
            for (int64_t tz = 0; tz < g.nt[0]; ++tz)
                for (int64_t ty = 0; ty < g.nt[1]; ++ty)
                    for (int64_t tx = 0; tx < g.nt[2]; ++tx) tile_step(conn, n, vol, tz, ty, tx, parent, &over);
            seam_step(conn, n, g, parent, &over);
            std::vector<uint64_t> ids;
            const uint64_t total = number_step(parent, 1, ids, &over);
            if (over) {
                printf("over\n");
                continue;
            }
            printf("%" PRIu64, total);
            for (uint64_t v : ids) printf(" %" PRIu64, v);
            printf("\n");
        } else if (cmd == "merge") {
            uint64_t n_labels;
            int64_t n;
            in >> n_labels >> n;
            if (!cc_nodes_fit(n_labels)) {
                printf("unsupported\n");
                continue;
            }
            std::vector<uint32_t> parent((size_t)n_labels);
            for (size_t i = 0; i < parent.size(); ++i) parent[i] = (uint32_t)i;
            int over = 0;
            bool bad = false;
            for (int64_t i = 0; i < n; ++i) {
                uint64_t a, b;
                in >> a >> b;
                if (a == 0 || b == 0 || a >= n_labels || b >= n_labels) bad = true;
                else uf_union(parent.data(), (uint32_t)a, (uint32_t)b, (uint32_t)n_labels, load, amin, &over);
            }
            if (bad || over) {
                printf(bad ? "bad\n" : "over\n");
                continue;
            }
            std::vector<uint64_t> ids;
            const uint64_t total = number_step(parent, 0, ids, &over);
            printf("%" PRIu64, total ? total - 1 : 0);
            for (uint64_t v : ids) printf(" %" PRIu64, v);
            printf("\n");
        } else if (cmd == "find") {
            uint32_t cap, x;
            in >> cap >> x;
            std::vector<uint32_t> parent;
            for (uint32_t p; in >> p;) parent.push_back(p);
            int over = 0;
            const uint32_t root = uf_find(parent.data(), x, cap, load, &over);
            printf("%d %u\n", over, root);
        } else {
            fprintf(stderr, "cc_check: unknown query '%s'\n", cmd.c_str());
            return 2;
        }
    }
    return 0;
}
