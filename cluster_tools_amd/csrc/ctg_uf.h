// The union-find of ctg_cc.hip (connected components of a thresholded block,
// and the merge of block-offset ids) and the bit helpers that read the x-runs
// of a row off its 64-bit foreground mask.  Written once, for the device and
// for the host: plain C++17 with the HIP qualifiers only where hipcc compiles
// it, so a host program runs the same code on the CPU (tools/cc_check.cpp,
// tests/test_cc_host.py).
//
// parent[] holds one u32 per node: the index of another node of the same set
// that is not larger, a root holding its own index.  Every union keeps the
// smaller index as the root, so the root of a set is its smallest member.
//
// Why the lock-free form is safe across workgroups.  The only store to
// parent[] is min(&parent[hi], lo) with lo < hi, so an entry only ever
// decreases, stays below or at its own index, and always names a member of the
// entry's set.  A reader that sees an out-of-date value (another XCD's L2, a
// store still in flight) therefore sees an earlier ancestor: following it
// still ends at a member of the set, and costs at most another round of the
// loop.  A union that finds parent[hi] no longer a root (the min returned
// something else than hi) goes on with what the entry held and lo -- both are
// members of the two sets being united -- until a min hits a root.  The
// device reads parent[] with relaxed agent-scope atomic loads and writes it
// with device-scope atomic mins alone, never with plain accesses: a CU's L1 is
// not refreshed by another CU's stores, and the L2s of two XCDs are not
// coherent.  Phases (tile, seams, flatten, number) are separate launches.
//
// Every loop is capped: a chain visits each node at most once, so `cap` = the
// number of nodes bounds the steps of a find and the rounds of a union.  Past
// the cap *over is set and the loop ends; the kernels raise a word of the
// call's error block and the host returns an error status.
#pragma once
#include <cstdint>

#ifdef __HIPCC__
#define CTG_HD __host__ __device__
#else
#define CTG_HD
#endif

namespace ctg {

constexpr uint32_t UF_NONE = 0xFFFFFFFFu;   // a background voxel's entry: no node

// ---------------------------------------------------------------------------
// runs of a row: bit x of m is voxel x of the row
// ---------------------------------------------------------------------------
// the first voxel of every run
CTG_HD inline uint64_t run_starts(uint64_t m) { return m & ~(m << 1); }
// the first voxel of the run that holds x (bit x of m is set)
CTG_HD inline int run_head(uint64_t m, int x) {
    return 63 - __builtin_clzll(run_starts(m) & (~0ull >> (63 - x)));
}
// Where the runs of row m touch the runs of an earlier row m2, one bit per
// touching pair of runs.  Straight (x over x): the first voxel of each run of
// m & m2 -- two runs overlap in one interval.
CTG_HD inline uint64_t contact_same(uint64_t m, uint64_t m2) { return run_starts(m & m2); }
// Diagonal only (x over x - 1, for neighbour rows dilated by one): x starts a
// run of m, x - 1 ends a run of m2, and the two runs do not overlap -- a pair
// that overlaps is in contact_same already.
CTG_HD inline uint64_t contact_up(uint64_t m, uint64_t m2) { return m & ~(m << 1) & (m2 << 1) & ~m2; }
// ... and x over x + 1: x ends a run of m, x + 1 starts a run of m2
CTG_HD inline uint64_t contact_down(uint64_t m, uint64_t m2) { return m & ~(m >> 1) & (m2 >> 1) & ~m2; }

// ---------------------------------------------------------------------------
// find and union.  load(p) returns *p; amin(p, v) stores min(*p, v) and
// returns what *p held (atomic on the device, plain on the host).
// ---------------------------------------------------------------------------
template <class Load>
CTG_HD inline uint32_t uf_find(const uint32_t* parent, uint32_t x, uint32_t cap, Load&& load, int* over) {
    for (uint32_t step = 0; step < cap; ++step) {
        const uint32_t p = load(&parent[x]);
        if (p == x) return x;
        x = p;
    }
    *over = 1;
    return x;
}

template <class Load, class Min>
CTG_HD inline void uf_union(uint32_t* parent, uint32_t a, uint32_t b, uint32_t cap, Load&& load, Min&& amin,
                            int* over) {
    for (uint32_t round = 0; round < cap; ++round) {
        a = uf_find(parent, a, cap, load, over);
        b = uf_find(parent, b, cap, load, over);
        if (*over || a == b) return;
        const uint32_t hi = a > b ? a : b, lo = a > b ? b : a;
        const uint32_t old = amin(&parent[hi], lo);
        if (old == hi) return;   // hi was a root and now hangs below lo
        a = old;                 // hi had been linked meanwhile: unite what it named with lo
        b = lo;
    }
    *over = 1;
}

}  // namespace ctg
