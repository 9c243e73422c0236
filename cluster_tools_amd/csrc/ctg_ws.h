// The seeded watershed of ctg_ws.hip: the minimum spanning forest of the box's
// 6-neighbour grid graph with every seeded voxel contracted into one root,
// grown by Boruvka rounds.  The edge order, a voxel's pick, a component's hook
// and the chase that flattens the forest are written once, for the device and
// for the host: plain C++17 with the HIP qualifiers only where hipcc compiles
// it, so a host program runs the same code on the CPU (tools/ws_check.cpp,
// tests/test_ws_host.py).
//
// The order.  k(h) is the order-preserving u32 image of a float32 height (-0
// taken as +0).  An edge joins two 6-neighbours u < v (box-linear C order)
// along axis a (z 0, y 1, x 2); its id is 3 * u + a, and edges are strictly
// ordered by (max(k(h_u), k(h_v)), min(k(h_u), k(h_v)), id): the first two as
// one 64-bit word (ws_edge_key), the id breaking what ties on it.
//
// parent[] holds one u32 per voxel of the box.  A box has at most 2^30 voxels,
// so an index needs 30 bits and bit 31 (WS_SEEDED) is free: an entry with the
// bit set names a seeded voxel, which is a root for good -- a seeded voxel's
// own entry is itself with the bit, and a seedless component that hooks to a
// seeded one copies the entry, bit included.  Without the bit an entry names a
// voxel of the same seedless component, a root holding its own index.  Between
// rounds the forest is flat: every entry is its component's root, so a voxel
// reads whether it is finished, and which component a neighbour is in, off one
// word.
//
// A round.  Every voxel of a seedless component offers its smallest edge that
// leaves the component (ws_voxel_pick); the component's smallest is found by
// an atomic minimum on the 64-bit key and then one on the id among the offers
// that tie on it.  The component's root then hooks (ws_hook): below the seeded
// root on the other side, or below the other component's root -- unless that
// component picked the same edge and has the larger root, in which case this
// one stays.  Under a strict order those mutual picks are the only cycles, so
// the hooks form a forest; ws_chase flattens it.  Every seedless component
// with an edge that leaves it hooks or is hooked to, so their number at least
// halves per round (ctg_plan.h: ws_round_cap).
//
// Across workgroups: within one launch parent[] is either read only (pick,
// hook), written only at the thread's own entry (apply), or touched with
// agent-scope atomic loads and stores alone (the chase, where an entry only
// ever moves up its own chain, so an out-of-date value is an earlier ancestor
// and costs steps, not correctness -- ctg_uf.h's argument).  The words the
// atomic minima write are read back in the next launch.  Every loop is
// capped; past the cap the kernels raise the call's error word.
#pragma once
#include <cstdint>

#ifndef CTG_HD
#ifdef __HIPCC__
#define CTG_HD __host__ __device__
#else
#define CTG_HD
#endif
#endif

namespace ctg {

constexpr uint32_t WS_SEEDED = 0x80000000u;   // a parent entry that names a seeded voxel
constexpr uint32_t WS_INDEX = 0x3FFFFFFFu;    // the voxel an entry names
constexpr uint32_t WS_NO_EDGE = 0xFFFFFFFFu;  // no edge id: 3 * 2^30 stays below it
constexpr uint64_t WS_NO_KEY = ~0ull;         // no edge key: only a NaN maps to an all-ones word
constexpr int WS_CHASE_STEPS = 64;            // entries one chase follows before it gives the rest to the next launch

// the order-preserving u32 image of a float32's bits
CTG_HD inline uint32_t ws_key_bits(uint32_t b) {
    if (b == 0x80000000u) b = 0u;   // -0 is +0
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
CTG_HD inline uint32_t ws_key(float h) {
    uint32_t b;
    __builtin_memcpy(&b, &h, 4);
    return ws_key_bits(b);
}
CTG_HD inline uint64_t ws_edge_key(uint32_t ka, uint32_t kb) {
    return ka > kb ? ((uint64_t)ka << 32) | kb : ((uint64_t)kb << 32) | ka;
}
// lower: the smaller box-linear index of the edge's two ends
CTG_HD inline uint32_t ws_edge_id(uint32_t lower, int axis) { return 3u * lower + (uint32_t)axis; }

struct WsEdge {
    uint64_t key;   // WS_NO_KEY: no edge
    uint32_t id;
};
CTG_HD inline bool ws_edge_less(const WsEdge& a, const WsEdge& b) {
    return a.key != b.key ? a.key < b.key : a.id < b.id;
}

struct WsBox {
    uint32_t n[3];   // the box (z, y, x)
    int two_d;       // no z edges: every slice floods on its own
};
// the box-linear distance between the two ends of an edge along axis a
CTG_HD inline uint32_t ws_axis_step(const WsBox& B, int a) { return a == 2 ? 1u : a == 1 ? B.n[2] : B.n[1] * B.n[2]; }

// The smallest edge that leaves the seedless component `root` at its voxel v.
// par(i): the flat entry of voxel i; key(i): k of its height.
template <class Par, class Key>
CTG_HD inline WsEdge ws_voxel_pick(const WsBox& B, uint32_t v, uint32_t root, Par&& par, Key&& key) {
    const uint32_t c[3] = {v / (B.n[1] * B.n[2]), (v / B.n[2]) % B.n[1], v % B.n[2]};
    const uint32_t kv = key(v);
    WsEdge best{WS_NO_KEY, WS_NO_EDGE};
    for (int a = B.two_d ? 1 : 0; a < 3; ++a) {
        const uint32_t step = ws_axis_step(B, a);
        for (int up = 0; up < 2; ++up) {
            if (up ? c[a] + 1 >= B.n[a] : c[a] == 0) continue;
            const uint32_t u = up ? v + step : v - step;
            if (par(u) == root) continue;   // (a seeded entry carries WS_SEEDED: never equal)
            const WsEdge e{ws_edge_key(kv, key(u)), ws_edge_id(up ? v : u, a)};
            if (ws_edge_less(e, best)) best = e;
        }
    }
    return best;
}

// What the seedless root r, whose component picked the edge `id`, hangs below:
// a parent entry, r itself where it stays.  par(i): the flat entry of voxel i;
// picked(i): the edge id the seedless root i picked, WS_NO_EDGE for none.
template <class Par, class Picked>
CTG_HD inline uint32_t ws_hook(const WsBox& B, uint32_t r, uint32_t id, Par&& par, Picked&& picked) {
    const uint32_t lo = id / 3u, hi = lo + ws_axis_step(B, (int)(id % 3u));
    const uint32_t pl = par(lo);
    const uint32_t other = pl == r ? par(hi) : pl;   // the entry of the end outside r's component
    if (other & WS_SEEDED) return other;
    return picked(other) == id && r < other ? r : other;
}

// The root of the chain above entry x, as an entry: at most WS_CHASE_STEPS
// loads.  *done is cleared where the chase stopped short of a root.
template <class Load>
CTG_HD inline uint32_t ws_chase(const uint32_t* parent, uint32_t x, Load&& load, bool* done) {
    for (int step = 0; step < WS_CHASE_STEPS; ++step) {
        if (x & WS_SEEDED) return x;
        const uint32_t p = load(&parent[x]);
        if (p == x) return x;
        x = p;
    }
    if (!(x & WS_SEEDED) && load(&parent[x]) != x) *done = false;
    return x;
}

}  // namespace ctg
