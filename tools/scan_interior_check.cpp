// Host check of the face scan's interior predicate (csrc/ctg_plan.h:
// scan_wave_interior, scan_interior_waves) for tests/test_scan_interior_plan.py.
//
//   scan_interior_check
//       sweeps shapes around the tile edges, owned boxes on and off the array's
//       edges, both row counts and tile depths 1, 2 and 4; for every wave of
//       every tile the predicate is compared with the plane loop's masks and
//       clamps, evaluated per lane, row and plane as k_face_scan defines them
//       (csrc/ctg_scan.hip): interior iff every mask is full and every clamp
//       is the identity.  The closed-form count of interior waves is compared
//       with the count over the waves, without and with tail tiles.  Prints
//       "waves W interior I launches L mismatches M" (the first mismatches on
//       stderr); exit status 1 if M > 0.
//   scan_interior_check Z Y X  obz oby obx  oez oey oex  x0 yw rows z0 z1
//       one wave -> "predicate masks"
//
// g++ -std=c++17 -fsanitize=address,undefined tools/scan_interior_check.cpp -o scan_interior_check
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../cluster_tools_amd/csrc/ctg_plan.h"

using namespace ctg;

constexpr int WAVES = 8;   // waves of a workgroup (ctg_scan.hip)

// The x side of a wave as the kernel sees it: all 64 lanes in the array and
// owned, the x face of each owned (lane 63's through the halo column), the
// lane's and the halo column's load offsets unclamped.
static bool x_full(int64_t X, int64_t obx, int64_t oex, int64_t x0) {
    bool all = true;
    for (int lane = 0; lane < TILE_X; ++lane) {
        const int64_t x = x0 + lane;
        const bool inx = x < X;
        const bool own_x_lo = x >= obx && x < oex;
        const bool lane_xf = inx && x + 1 < X && x + 1 >= obx && x + 1 < oex;
        const bool lane_yz = inx && own_x_lo;
        const int64_t xcl = std::min(x, X - 1);
        all = all && lane_xf && lane_yz && xcl == x;
    }
    const int64_t xh = x0 + TILE_X, xhc = std::min(xh, X - 1);
    return all && xhc == xh;
}

// The y side: every row's bit of row_x and row_y, the wave's first row and the
// row offsets 0 .. rows (the halo row) unclamped.
static bool y_full(int64_t Y, int64_t oby, int64_t oey, int64_t yw, int rows) {
    uint32_t row_x = 0, row_y = 0;
    for (int r = 0; r < rows; ++r) {
        const int64_t y = yw + r;
        if (y < Y && y >= oby && y < oey) row_x |= 1u << r;
        if (y + 1 < Y && y + 1 >= oby && y + 1 < oey) row_y |= 1u << r;
    }
    const uint32_t all = (1u << rows) - 1u;
    const int64_t ywc = std::min(yw, Y - 1), rmaxc = Y - 1 - ywc;
    bool same = ywc == yw;
    for (int r = 0; r <= rows; ++r) same = same && std::min<int64_t>(r, rmaxc) == r;
    return row_x == all && row_y == all && same;
}

// The z side: every plane of [z0, z1) owned, with an owned plane above it that
// the prefetch reads (hz: no re-read of the last plane).
static bool z_full(int64_t Z, int64_t obz, int64_t oez, int64_t z0, int64_t z1) {
    bool all = true;
    for (int64_t z = z0; z < z1; ++z) {
        const bool hz = z + 1 < Z;
        const bool zlo = z >= obz && z < oez;
        const bool zup = hz && z + 1 >= obz && z + 1 < oez;
        all = all && hz && zlo && zup;
    }
    return all;
}

struct Sweep {
    int64_t waves = 0, interior = 0, launches = 0, mismatches = 0;
    void bad(const char* what, const int64_t* s, const int64_t* ob, const int64_t* oe, int rows, int depth, int64_t a,
             int64_t b) {
        if (++mismatches <= 10)
            fprintf(stderr,
                    "%s: shape %" PRId64 " %" PRId64 " %" PRId64 " own [%" PRId64 " %" PRId64 " %" PRId64 ") .. [%" PRId64
                    " %" PRId64 " %" PRId64 ") rows %d depth %d: %" PRId64 " != %" PRId64 "\n",
                    what, s[0], s[1], s[2], ob[0], ob[1], ob[2], oe[0], oe[1], oe[2], rows, depth, a, b);
    }
};

// one launch: every wave against the masks, then the closed-form count
// (xf: x_full of the launch's tile columns, the same for every row and layer)
static void check_launch(Sweep& S, const int64_t* shape, const int64_t* ob, const int64_t* oe, const ScanTilePlan& t,
                         const std::vector<char>& xf) {
    int64_t count = 0;
    const int64_t layers = t.main_layers + t.tail_layers;
    for (int64_t tz = 0; tz < layers; ++tz) {
        const bool tail = tz >= t.main_layers;
        const int64_t z0 = tail ? t.tail_z0 + (tz - t.main_layers) * t.tile_z_tail : tz * t.tile_z;
        const int64_t z1 = std::min(z0 + (tail ? t.tile_z_tail : t.tile_z), tail ? shape[0] : std::min(shape[0], t.tail_z0));
        const bool zf = z_full(shape[0], ob[0], oe[0], z0, z1);
        for (int64_t w = 0; w < t.nty * t.waves; ++w) {
            const int64_t yw = w * t.rows;
            const bool yf = y_full(shape[1], ob[1], oe[1], yw, (int)t.rows);
            for (int64_t tx = 0; tx < t.ntx; ++tx) {
                const int64_t x0 = tx * TILE_X;
                const bool masks = zf && yf && xf[tx];
                const bool pred = scan_wave_interior(shape, ob, oe, x0, yw, t.rows, z0, z1);
                ++S.waves;
                S.interior += pred;
                count += pred;
                if (pred != masks) S.bad("wave", shape, ob, oe, (int)t.rows, (int)t.tile_z, pred, masks);
            }
        }
    }
    ++S.launches;
    const int64_t closed = scan_interior_waves(shape, ob, oe, t);
    if (closed != count) S.bad("count", shape, ob, oe, (int)t.rows, (int)t.tile_z, closed, count);
    if (t.n_waves() != layers * t.nty * t.waves * t.ntx) S.bad("n_waves", shape, ob, oe, (int)t.rows, (int)t.tile_z, 0, 0);
}

// owned ranges [b, e) of an axis of n voxels: on the array's edges, one voxel
// off them, and on and one past the tile edges `edges`
static std::vector<std::pair<int64_t, int64_t>> own_ranges(int64_t n, std::vector<int64_t> edges) {
    std::vector<int64_t> bs{0, 1}, es{n, n - 1};
    for (int64_t e : edges) {
        bs.push_back(e);
        bs.push_back(e + 1);
        es.push_back(e);
        es.push_back(e + 1);
    }
    std::vector<std::pair<int64_t, int64_t>> out;
    for (int64_t b : bs)
        for (int64_t e : es)
            if (0 <= b && b < e && e <= n) {
                bool dup = false;
                for (auto& p : out) dup = dup || (p.first == b && p.second == e);
                if (!dup) out.push_back({b, e});
            }
    return out;
}

int main(int argc, char** argv) {
    if (argc == 15) {
        int64_t v[14];
        for (int i = 0; i < 14; ++i) v[i] = atoll(argv[i + 1]);
        const int64_t *shape = v, *ob = v + 3, *oe = v + 6;
        const int64_t x0 = v[9], yw = v[10], rows = v[11], z0 = v[12], z1 = v[13];
        printf("%d %d\n", (int)scan_wave_interior(shape, ob, oe, x0, yw, rows, z0, z1),
               (int)(x_full(shape[2], ob[2], oe[2], x0) && y_full(shape[1], ob[1], oe[1], yw, (int)rows) &&
                     z_full(shape[0], ob[0], oe[0], z0, z1)));
        return 0;
    }
    if (argc != 1) {
        fprintf(stderr, "usage: scan_interior_check [Z Y X obz oby obx oez oey oex x0 yw rows z0 z1]\n");
        return 2;
    }
    Sweep S;
    for (int64_t X : {63, 64, 65, 128, 129})
        for (int64_t Y : {31, 32, 33, 36, 37})
            for (int64_t Z : {1, 2, 3, 4, 5})
                for (int rows : {4, 1})
                    for (int depth : {1, 2, 4}) {
                        const int64_t shape[3] = {Z, Y, X};
                        const int64_t nz = (Z + depth - 1) / depth;
                        ScanTilePlan t{(X + TILE_X - 1) / TILE_X, (Y + rows * WAVES - 1) / (rows * WAVES), rows, WAVES,
                                       depth, nz, Z, depth, 0};
                        // ... and the last layer cut into one-plane tail tiles
                        ScanTilePlan tt = t;
                        tt.main_layers = nz - 1;
                        tt.tail_z0 = (nz - 1) * depth;
                        tt.tile_z_tail = 1;
                        tt.tail_layers = Z - tt.tail_z0;
                        for (auto& xr : own_ranges(X, {TILE_X})) {
                            std::vector<char> xf;
                            for (int64_t tx = 0; tx < t.ntx; ++tx) xf.push_back(x_full(X, xr.first, xr.second, tx * TILE_X));
                            for (auto& zr : own_ranges(Z, {(int64_t)depth}))
                                for (auto& yr : own_ranges(Y, {(int64_t)rows, (int64_t)rows * WAVES})) {
                                    const int64_t ob[3] = {zr.first, yr.first, xr.first};
                                    const int64_t oe[3] = {zr.second, yr.second, xr.second};
                                    check_launch(S, shape, ob, oe, t, xf);
                                    if (depth > 1 && nz >= 2) check_launch(S, shape, ob, oe, tt, xf);
                                }
                        }
                    }
    printf("waves %" PRId64 " interior %" PRId64 " launches %" PRId64 " mismatches %" PRId64 "\n", S.waves, S.interior,
           S.launches, S.mismatches);
    return S.mismatches ? 1 : 0;
}
