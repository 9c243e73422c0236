// The host layer's decisions as pure functions: tile depths, the channel
// classification, the choice between the record-sort paths and the key range
// of the bucket sort.  Plain C++17 -- no HIP, no getenv: the environment
// switches are read by the callers and passed in as values -- so a host
// program can exercise them without a GPU (tools/plan_check.cpp,
// tests/test_plan.py).
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdlib>

#include "../../include/ctg.h"

namespace ctg {

constexpr int TILE_X = 64;             // one wave row

inline int bits_for(uint64_t v) {
    int b = 1;
    while (b < 64 && (v >> b)) ++b;
    return b;
}

// ---------------------------------------------------------------------------
// face-scan tile depths (whole arrays)
// ---------------------------------------------------------------------------
struct TileDepths {
    int tile_z;          // z-planes per workgroup
    int tile_z_narrow;   // z-planes per workgroup of the narrow-tile launch
};

// shape (z, y, x); rows_wide / rows_narrow: y rows of a wide / narrow tile
inline TileDepths scan_tile_depths(const int64_t* shape, int64_t rows_wide, int64_t rows_narrow) {
    // planes per workgroup of the narrow-tile launch (fragmented volumes):
    // shallower tiles split fewer edges at table flushes (profiles/r4/tz)
    constexpr int NARROW_TILE_Z = 16;
    // planes per workgroup: 32, fewer where that leaves < ~1024 workgroups,
    // 64 (128) where even 64 (128)-plane tiles give >= 32 K workgroups (A/B with the 5/8
    // table fill, 32 vs 64 planes: 512^3 step 1.027 -> 1.014 ms, configs[4]
    // 32.2 -> 30.0 ms with records 148 M -> 134 M; 2048^3 scan 30.4 vs 30.9 ms
    // favours 64)
    const int64_t cols = ((shape[2] + TILE_X - 1) / TILE_X) * ((shape[1] + rows_wide - 1) / rows_wide);
    int tz = cols * ((shape[0] + 63) / 64) >= 32768 ? 64 : 32;
    // 128 where even 128-plane tiles leave >= 6 K workgroups (2048^3: scan
    // 29.76 -> 29.35 ms, records 28.1 M -> 27.3 M, step 33.65 -> 33.08 ms,
    // profiles/r4/ablate; the 513- and 1025-plane z-slabs of 2048^2 over 4 /
    // 2 ranks, 10 K / 18 K workgroups: 8.02 -> 7.84 and 15.41 -> 15.18 ms
    // against 32 / 64 planes, profiles/r6/r; the 257-plane slab of 8 ranks,
    // 6 K workgroups, with its one-plane last layer as tail tiles: 4.23 ->
    // 4.18 ms, profiles/r6/w)
    if (cols * ((shape[0] + 127) / 128) >= 6144) tz = 128;
    while (tz > 8 && cols * ((shape[0] + tz - 1) / tz) < 1024) tz /= 2;
    // narrow tiles 16 planes deep, deeper where that would launch more than
    // 64 K workgroups: both widths are launched and one exits at once, and
    // at 2048^3 the exiting launch of 16-plane narrow tiles (524 K
    // workgroups) cost 0.22 ms per call
    const int64_t cols_n = ((shape[2] + TILE_X - 1) / TILE_X) * ((shape[1] + rows_narrow - 1) / rows_narrow);
    int tzn = std::min(tz, NARROW_TILE_Z);
    while (tzn < tz && cols_n * ((shape[0] + tzn - 1) / tzn) > 65536) tzn *= 2;
    return {tz, tzn};
}

// ---------------------------------------------------------------------------
// affinity channels
// ---------------------------------------------------------------------------
struct ChannelClass {
    uint32_t lr_mask = 0;         // bit c: channel c is long-range (|offset|_1 > 1)
    bool long_range = false;      // some channel is
    int nn_ch[3] = {-1, -1, -1};  // first channel of the nearest-neighbour offset -e_a (a = z, y, x), or -1
    int n_loop = 0;               // the channels that are none of nn_ch, in order
    int loop_ch[CTG_MAX_CHANNELS] = {};
    bool nn_all() const { return nn_ch[0] >= 0 && nn_ch[1] >= 0 && nn_ch[2] >= 0; }
};

inline ChannelClass classify_channels(const int (*offsets)[3], int n_channels) {
    ChannelClass cc;
    for (int c = 0; c < n_channels; ++c) {
        const int* o = offsets[c];
        if (std::abs(o[0]) + std::abs(o[1]) + std::abs(o[2]) > 1) cc.lr_mask |= 1u << c;
        // a repeated nearest-neighbour offset: the first channel is the face
        // channel, the others stay in the channel loop.  With exactly three
        // channels and all three axes present every axis has one channel, so
        // first match and last match coincide (the nn3 form)
        for (int a = 0; a < 3; ++a)
            if (cc.nn_ch[a] < 0 && o[a] == -1 && o[(a + 1) % 3] == 0 && o[(a + 2) % 3] == 0) cc.nn_ch[a] = c;
    }
    cc.long_range = cc.lr_mask != 0;
    for (int c = 0; c < n_channels; ++c)
        if (c != cc.nn_ch[0] && c != cc.nn_ch[1] && c != cc.nn_ch[2]) cc.loop_ch[cc.n_loop++] = c;
    return cc;
}

struct ChannelPlan {
    // the three nearest-neighbour channels are present, so every RAG edge gets
    // a sample of one of them (the adjacency proof) and no separate markers
    // are pushed
    bool skip_adj_marks;
    // exactly the three nearest-neighbour channels (any order), every sample
    // an adjacency proof: the face-scan form of the affinity scan (MODE_AFF_NN,
    // ctg_scan.hip)
    bool nn3;
    // long-range calls with the Bloom filter: the nearest-neighbour channels
    // as faces (their samples flag adjacency), the rest looped
    bool nn_mix;
};

// adj_filter: the call filters by adjacency (no CTG_NO_ADJ_FILTER); have_bloom:
// the Bloom prefilter of the RAG edges was built; skip_adj_switch: CTG_SKIP_ADJ
// (0 keeps the markers); nn_switch: CTG_NN3 (false keeps the channel loop)
inline ChannelPlan plan_channels(const ChannelClass& cc, int n_channels, bool adj_filter, bool have_bloom,
                                 bool skip_adj_switch, bool nn_switch) {
    ChannelPlan p{};
    p.skip_adj_marks = n_channels > 0 && cc.nn_all() && adj_filter && (!cc.long_range || have_bloom) && skip_adj_switch;
    const bool faces = p.skip_adj_marks && nn_switch;
    p.nn3 = faces && n_channels == 3 && !cc.long_range;
    p.nn_mix = faces && cc.long_range && have_bloom;
    return p;
}

// ---------------------------------------------------------------------------
// record sort
// ---------------------------------------------------------------------------
// The wide digits pay off for small sorts (launch / look-back bound: 1.9 M
// records at 512^3: 0.185 -> 0.151 ms; 27.8 M at 2048^3: 1.88 -> 1.49 ms) and
// lose for very large ones (298 M records of configs[4]:
// 14.1 -> 18.7 ms, the 1024-way scatter coalesces worse), so they are used up
// to this many records.
constexpr int64_t SORT_WIDE_DIGITS_MAX = (int64_t)(64 << 20);
// The pair path's bucket sort pays up to ~30 M records (1024^3 3-channel: 1.09 -> 1.00 ms at
// 15.6 M; 2048^3: equal at 28 M) and loses on configs[4]'s 190 M (9.5 -> 12.8 ms: buckets of
// ~46 K records go to the segmented sort's slower large-segment path): up to
// ~32 M records (configs[4]'s 138 M: onesweep 6.7 ms against 9.3 ms for the bucket pass with
// the in-LDS sort of ~34 K-record buckets split into sub-buckets; profiles/r4/g)
constexpr int64_t BUCKET_PAIRS_MAX = (int64_t)(32 << 20);

struct SortSwitches {
    bool packed = true;        // CTG_SORT_PACKED
    bool bucket = true;        // CTG_BUCKET_SORT
    int bucket_pairs = -1;     // CTG_BUCKET_SORT_PAIRS: 0 / 1 forces it, -1 by the record count
    // CTG_GROUP_SORT=0: the (key, slot) scan records take the bucket / onesweep paths
    bool group = true;
    // CTG_GROUP_FIRST=1: records whose key and slot pack into one word take the
    // group sort too (hand-written end to end) instead of the packed-key bucket
    // sort + rocPRIM's segmented radix sort of the bucket-local bits; measured
    // 1.4 % slower at 512^3 (sort 0.130 -> 0.147 ms, profiles/r6/gf), so off
    bool group_first = false;
};

enum class SortPath {
    BucketKeys,            // packed keys: MSD bucket pass + segmented sort of the key bits
    OnesweepKeys,          // packed keys: rocPRIM onesweep, wide digits
    BucketPairs,           // (key, index) pairs: MSD bucket pass + segmented sort
    OnesweepPairsWide,     // (key, index) pairs: rocPRIM onesweep, wide digits
    OnesweepPairsDefault,  // (key, index) pairs: rocPRIM's default digits
};

struct RecordSortPlan {
    bool packed;      // the slot rides in the low ib bits of the sort key (unless the group sort takes the records)
    bool try_group;   // offer the records to the group sort first (it may decline)
    SortPath path;    // the path when the group sort is not tried or declines
};

// has_keys: packed (u << 32) | v keys (else (u, v) pairs); has_regions: scan
// records in their regions; ub / nb / ib: bits of the key's u field, of the
// largest label and of the record slot; spread: the keys' top bits are label
// bits (no block tag)
inline RecordSortPlan plan_record_sort(bool has_keys, bool has_regions, int64_t n, int ub, int nb, int ib, bool spread,
                                       const SortSwitches& sw) {
    RecordSortPlan p{};
    // Scan records whose slot fits beside the 2*nb key bits sort as bare u64
    // keys (slot in the low ib bits): 16 instead of 24 bytes per record and
    // pass; the reduction reads the slots from the sorted keys (CTG_SORT_PACKED=0 disables).
    // at most 63 bits: with the record slot packed up to bit 63 exactly, the
    // sorted order came out wrong (tests/test_gpu_blocks.py::
    // test_blocks_independent_of_workspace_history), so one bit stays free
    p.packed = has_keys && has_regions && sw.packed && ub + nb + ib <= 63 && n <= SORT_WIDE_DIGITS_MAX;
    // the bucket passes need keys spread over their top bits: block-tagged keys
    // (ctg_rag_blocks) put the block id there and fill a few huge
    // buckets (configs[0] device time 3.9 -> 6.7 ms), so they keep onesweep
    // (key, slot) scan records: the group sort reads the record regions itself
    // (no pack pass) and writes the run table and the slot permutation
    p.try_group = has_keys && has_regions && (!p.packed || sw.group_first) && spread && sw.group;
    const bool bucket_pairs = sw.bucket_pairs >= 0 ? sw.bucket_pairs == 1 : n <= BUCKET_PAIRS_MAX;
    if (p.packed) p.path = spread && sw.bucket ? SortPath::BucketKeys : SortPath::OnesweepKeys;
    else if (spread && bucket_pairs) p.path = SortPath::BucketPairs;
    else p.path = n <= SORT_WIDE_DIGITS_MAX ? SortPath::OnesweepPairsWide : SortPath::OnesweepPairsDefault;
    return p;
}

struct KeyRange {
    uint64_t kmin, kmax;
};

// every packed key lies in [(min_u << nb) << ib, ((max_v << nb | max_v) << ib) | slot bits]
inline KeyRange packed_key_range(uint64_t min_u, uint64_t max_v, int nb, int ib) {
    const uint64_t vmax = std::min<uint64_t>(max_v, (1ull << nb) - 1ull);
    const uint64_t kmax = (((vmax << nb) | vmax) << ib) | ((1ull << ib) - 1ull);
    const uint64_t kmin = std::min<uint64_t>((std::min<uint64_t>(min_u, vmax) << nb) << ib, kmax);
    return {kmin, kmax};
}

}  // namespace ctg
