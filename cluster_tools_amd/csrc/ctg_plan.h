// The host layer's decisions as pure functions: call boxes, tile depths, the
// batched-block plan, record-buffer and candidate-buffer sizes, the Bloom
// filter's size, the narrow-row mode, the channel classification, the
// adjacency rule of the reduce, the slab range and the segment plan of the
// multi-GPU exchange, the choice between the record-sort paths, the key range
// of the bucket sort and the bucket geometry of the bucket and group sorts.  Plain
// C++17 -- no HIP (the bucket arithmetic and the segment lookup the kernels
// share are marked CTG_HD),
// no getenv: the environment switches are
// read by the callers (scan_switches, sort_switches) and passed in as values --
// so a host program can exercise them without a GPU (tools/plan_check.cpp,
// tests/test_plan.py).
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <vector>

#include "../../include/ctg.h"

// the bucket arithmetic below is shared with the sort kernels (as ctg_uf.h)
#ifndef CTG_HD
#ifdef __HIPCC__
#define CTG_HD __host__ __device__
#else
#define CTG_HD
#endif
#endif

namespace ctg {

constexpr int TILE_X = 64;             // one wave row

inline int bits_for(uint64_t v) {
    int b = 1;
    while (b < 64 && (v >> b)) ++b;
    return b;
}
inline int bits_u(int64_t v) { return v <= 0 ? 0 : bits_for((uint64_t)v); }

// ---------------------------------------------------------------------------
// the box of a call
// ---------------------------------------------------------------------------
struct CallBox {
    enum Error { OK, OUTSIDE, TOO_LARGE } error;
    int64_t b[3], e[3];
    int64_t voxels;
};

// [b, e) of a call on an array of `shape`: begin / end default to the whole
// array and the box must lie inside it (checked on every axis first); then, with
// max_voxels > 0, it must hold fewer than max_voxels voxels
inline CallBox call_box(const int64_t* shape, const int64_t* begin, const int64_t* end, int64_t max_voxels) {
    CallBox c{};
    for (int k = 0; k < 3; ++k) {
        c.b[k] = begin ? begin[k] : 0;
        c.e[k] = end ? end[k] : shape[k];
        if (shape[k] < 0 || c.b[k] < 0 || c.e[k] > shape[k] || c.b[k] > c.e[k]) {
            c.error = CallBox::OUTSIDE;
            return c;
        }
    }
    c.voxels = (c.e[0] - c.b[0]) * (c.e[1] - c.b[1]) * (c.e[2] - c.b[2]);
    c.error = max_voxels > 0 && c.voxels >= max_voxels ? CallBox::TOO_LARGE : CallBox::OK;
    return c;
}

// What a dense-volume kernel reads of its box (thresholded components, the
// distance transform, the watershed): voxel (z, y, x) of the box is element
// base + z * s_z + y * s_y + x of the array.
struct VolBox {
    int64_t s_z, s_y;           // the array's strides in elements
    int64_t base;               // element offset of the box's first voxel
    uint32_t n[3];              // the box (z, y, x)
};

// c: a box of call_box on `shape` without error (an axis below 2^32)
inline VolBox vol_box(const int64_t* shape, const CallBox& c) {
    VolBox v{};
    v.s_z = shape[1] * shape[2];
    v.s_y = shape[2];
    v.base = c.b[0] * v.s_z + c.b[1] * v.s_y + c.b[2];
    for (int k = 0; k < 3; ++k) v.n[k] = (uint32_t)(c.e[k] - c.b[k]);
    return v;
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

// boundary maps of fragmented volumes scan with 1-row waves.  0: wide tiles;
// 1: narrow; 2: the sampled x-face density decides on the device.  The probe
// and the second launch cost ~0.1 ms, so volumes below 2^28 voxels (~645^3,
// steps of ~2 ms) keep the wide tiles.  nr_switch: CTG_NARROW_ROWS, 0 / 1
// forces a width (at any size), -1 unset
inline int narrow_rows_mode(bool boundary_map, int64_t V, int nr_switch) {
    if (!boundary_map || (V < (1ll << 28) && nr_switch < 0)) return 0;
    return nr_switch < 0 ? 2 : (nr_switch ? 1 : 0);
}

// ---------------------------------------------------------------------------
// face-scan interior waves (whole arrays)
// ---------------------------------------------------------------------------
// One axis of a wave's reach: voxels [a, b) and, at b, the upper neighbour of
// the last one.  Interior: every voxel is owned, and b exists and is owned.
CTG_HD constexpr bool scan_axis_interior(int64_t n, int64_t ob, int64_t oe, int64_t a, int64_t b) {
    return ob <= a && b < oe && b < n;
}
// A wave of the face scan holds rows [yw, yw + rows) (+ the halo row) of the
// columns [x0, x0 + TILE_X) (+ the halo column) and walks the planes [z0, z1)
// (+ the prefetched plane z1).  It is interior when all of that lies in the
// owned box [own_begin, own_end) of the array: then every ownership mask of the
// plane loop is full -- each lane, row and plane, and the x, y and z face above
// each -- and no load offset is clamped, so the loop may drop the masks and the
// clamps (ctg_scan.hip).  A wave that merely fills its tile is not interior:
// its last lane, row or plane may be the array's, with no neighbour above.
CTG_HD constexpr bool scan_wave_interior(const int64_t* shape, const int64_t* own_begin, const int64_t* own_end,
                                         int64_t x0, int64_t yw, int64_t rows, int64_t z0, int64_t z1) {
    return scan_axis_interior(shape[2], own_begin[2], own_end[2], x0, x0 + TILE_X) &&
           scan_axis_interior(shape[1], own_begin[1], own_end[1], yw, yw + rows) &&
           scan_axis_interior(shape[0], own_begin[0], own_end[0], z0, z1);
}

// The tiles of one whole-array launch (ctg_scan.hip: launch_scan_r): ntx x nty
// tiles of TILE_X columns and waves x rows rows a layer; main_layers layers of
// tile_z planes from plane 0, cut off at tail_z0, then tail_layers layers of
// tile_z_tail planes from tail_z0 (none: tail_z0 = Z).
struct ScanTilePlan {
    int64_t ntx, nty, rows, waves;
    int64_t tile_z, main_layers, tail_z0, tile_z_tail, tail_layers;
    constexpr int64_t n_waves() const { return ntx * nty * waves * (main_layers + tail_layers); }
};
// Interior waves of such a launch.  scan_wave_interior is a conjunction over
// the axes, so the count is the product of the per-axis counts.
inline int64_t scan_interior_waves(const int64_t* shape, const int64_t* own_begin, const int64_t* own_end,
                                   const ScanTilePlan& t) {
    int64_t nx = 0, ny = 0, nz = 0;
    for (int64_t tx = 0; tx < t.ntx; ++tx)
        nx += scan_axis_interior(shape[2], own_begin[2], own_end[2], tx * TILE_X, tx * TILE_X + TILE_X);
    for (int64_t w = 0; w < t.nty * t.waves; ++w)
        ny += scan_axis_interior(shape[1], own_begin[1], own_end[1], w * t.rows, w * t.rows + t.rows);
    const int64_t zlim = std::min(shape[0], t.tail_z0);
    for (int64_t tz = 0; tz < t.main_layers; ++tz)
        nz += scan_axis_interior(shape[0], own_begin[0], own_end[0], tz * t.tile_z,
                                 std::min(tz * t.tile_z + t.tile_z, zlim));
    for (int64_t tz = 0; tz < t.tail_layers; ++tz)
        nz += scan_axis_interior(shape[0], own_begin[0], own_end[0], t.tail_z0 + tz * t.tile_z_tail,
                                 std::min(t.tail_z0 + tz * t.tile_z_tail + t.tile_z_tail, shape[0]));
    return nx * ny * nz;
}

// What ctg_last_scan reports of a workspace's last whole-array face scan
// (ctg.h: the CTG_SCAN_* words): per tile width, the waves launched and how
// many of them take the interior plane loop.  Host values only.
struct ScanReport {
    int64_t waves[2] = {0, 0};      // [0] wide tiles, [1] narrow tiles; 0: no such launch
    int64_t interior[2] = {0, 0};
};

// ---------------------------------------------------------------------------
// batched blocks (ctg_rag_blocks)
// ---------------------------------------------------------------------------
// one array of a batched call: the host's ctg_block_desc in device memory plus
// the tile bookkeeping of the launch
struct BlockGeom {
    int64_t label_offset;    // element offset of the array in the labels arena
    int64_t data_offset;     // element offset in the data arena (affinities: channel 0 of C x V)
    int32_t shape[3];
    int32_t own_begin[3], own_end[3];
    int32_t graph_begin[3], graph_end[3];
    int32_t ntx, nty, ntz;   // tiles along x, y, z
};

struct BlockPlan {
    // BOX_OUTSIDE / ARRAY_OUTSIDE: of block bad_block, the first such block (its
    // box is checked before its place in the arenas); TOO_MANY_TILES: every
    // block is fine but one of the two launches would pass 2^31 - 1 tiles
    enum Error { OK, BOX_OUTSIDE, ARRAY_OUTSIDE, TOO_MANY_TILES } error = OK;
    int bad_block = -1;
    int64_t own_voxels = 0, voxels = 0;   // over all blocks: owned boxes, arrays
    int tile_z = 0;                       // planes per workgroup: one tile deep for the usual <= 128-plane blocks
    // keys carry the block in the bits of u from tag_shift up (32: no tag);
    // label_hi_mask: the bits a label must not have
    int tag_bits = 0, tag_shift = 32;
    uint32_t label_hi_mask = 0;
    std::vector<BlockGeom> geom;
    std::vector<uint32_t> prefix;    // tiles of the scan launch before block b
    std::vector<uint32_t> uprefix;   // tiles of the node launch (64 x unique_rows x 16 voxels of the owned box)
};

// has_data: a data arena is given (else data offsets are not looked at and are
// 0 in the geometry); max_x: the widest array the scan takes; scan_rows /
// unique_rows: y rows of a scan / node tile; tile_z_switch: CTG_TILE_Z, 0 unset
inline BlockPlan plan_blocks(const ctg_block_desc* blocks, int n_blocks, bool has_data, int n_channels,
                             int64_t labels_len, int64_t data_len, int64_t max_x, int scan_rows, int unique_rows,
                             int tile_z_switch) {
    BlockPlan p;
    const int nch = has_data ? std::max(1, n_channels) : 0;
    int64_t zmax = 1;
    for (int b = 0; b < n_blocks; ++b) {
        const ctg_block_desc& d = blocks[b];
        int64_t V = 1, ov = 1;
        p.bad_block = b;
        for (int k = 0; k < 3; ++k) {
            V *= d.shape[k];
            if (d.shape[k] < 0 || d.shape[k] > (k == 2 ? max_x : 0x7FFFFFFF) || d.own_begin[k] < 0 ||
                d.own_end[k] > d.shape[k] || d.graph_begin[k] < 0 || d.graph_end[k] > d.shape[k]) {
                p.error = BlockPlan::BOX_OUTSIDE;
                return p;
            }
        }
        if (d.label_offset < 0 || d.label_offset + V > labels_len ||
            (has_data && (d.data_offset < 0 || d.data_offset + V * nch > data_len))) {
            p.error = BlockPlan::ARRAY_OUTSIDE;
            return p;
        }
        for (int k = 0; k < 3; ++k) ov *= std::max<int64_t>(0, d.own_end[k] - d.own_begin[k]);
        p.own_voxels += ov;
        p.voxels += V;
        zmax = std::max(zmax, d.shape[0]);
    }
    p.bad_block = -1;
    p.tile_z = tile_z_switch > 0 ? tile_z_switch : (int)std::min<int64_t>(zmax, 128);
    p.tag_bits = bits_u(n_blocks - 1);
    p.tag_shift = 32 - p.tag_bits;
    p.label_hi_mask = p.tag_bits ? ~((1u << p.tag_shift) - 1u) : 0u;
    p.geom.resize(n_blocks);
    p.prefix.assign(n_blocks + 1, 0);
    p.uprefix.assign(n_blocks + 1, 0);
    for (int b = 0; b < n_blocks; ++b) {
        const ctg_block_desc& d = blocks[b];
        BlockGeom& g = p.geom[b];
        g.label_offset = d.label_offset;
        g.data_offset = has_data ? d.data_offset : 0;
        int64_t oe[3];
        for (int k = 0; k < 3; ++k) {
            g.shape[k] = (int32_t)d.shape[k];
            g.own_begin[k] = (int32_t)d.own_begin[k];
            g.own_end[k] = (int32_t)d.own_end[k];
            g.graph_begin[k] = (int32_t)d.graph_begin[k];
            g.graph_end[k] = (int32_t)d.graph_end[k];
            oe[k] = std::max<int64_t>(0, d.own_end[k] - d.own_begin[k]);
        }
        g.ntx = (int32_t)((d.shape[2] + TILE_X - 1) / TILE_X);
        g.nty = (int32_t)((d.shape[1] + scan_rows - 1) / scan_rows);
        g.ntz = (int32_t)((d.shape[0] + p.tile_z - 1) / p.tile_z);
        const int64_t nt = (int64_t)g.ntx * g.nty * g.ntz;
        const int64_t ut = ((oe[2] + 63) / 64) * ((oe[1] + unique_rows - 1) / unique_rows) * ((oe[0] + 15) / 16);
        if ((int64_t)p.prefix[b] + nt > 0x7FFFFFFFll || (int64_t)p.uprefix[b] + ut > 0x7FFFFFFFll) {
            p.error = BlockPlan::TOO_MANY_TILES;
            return p;
        }
        p.prefix[b + 1] = p.prefix[b] + (uint32_t)nt;
        p.uprefix[b + 1] = p.uprefix[b] + (uint32_t)ut;
    }
    return p;
}

// ---------------------------------------------------------------------------
// records: the face scan flushes one record per (tile, edge)
// ---------------------------------------------------------------------------
// The scan reserves record slots from NREG region counters (region r owns
// slots [r*rcap, (r+1)*rcap)) instead of one global counter: same-address
// device atomics serialize (~25 ns each), and one counter per flush across
// every workgroup of the chip was a measurable queue.
constexpr int NREG = 64;

struct RegionPrefix {          // exclusive prefix of the region counts (host-computed)
    uint32_t off[NREG + 1];
};

// record slots a scan of V voxels starts with (cap: the slots the workspace
// holds already), a multiple of NREG
inline int64_t record_slots_first(int64_t cap, int64_t V) {
    const int64_t need = std::max<int64_t>(cap, std::max<int64_t>(1 << 16, V / 24));
    return (need + NREG - 1) / NREG * NREG;
}
// ... and after an overflow, from the fullest region's count
inline int64_t record_slots_regrow(uint64_t fullest) { return ((int64_t)(fullest * 5 / 4) + 1024) * NREG; }

struct RegionFold {
    RegionPrefix pre;
    uint64_t total, fullest;
};
// the NREG region counts of a scan -> their exclusive prefix (32 bits: the
// caller refuses totals of 2^32), their sum and their maximum
inline RegionFold fold_regions(const unsigned long long* rcount) {
    RegionFold f{};
    for (int r = 0; r < NREG; ++r) {
        f.pre.off[r] = (uint32_t)f.total;
        f.total += rcount[r];
        f.fullest = std::max<uint64_t>(f.fullest, rcount[r]);
    }
    f.pre.off[NREG] = (uint32_t)f.total;
    return f;
}

// unique-label candidates (per tile and flush, so a label repeats): the buffer
// a pass over n voxels starts with, and after a pass that counted m > capacity
// candidates; bound: what the regrown buffer never needs to pass
inline int64_t candidate_cap_first(int64_t n) {
    return std::max<int64_t>(1, std::min<int64_t>(n, std::max<int64_t>(1 << 16, n / 8)));
}
inline int64_t candidate_cap_regrow(int64_t m, int64_t bound) { return std::min<int64_t>(bound, m + 1024); }

// 64-byte blocks of the Bloom filter of n_edges RAG edges: 24 bits per stored
// direction (48 per edge; 32: +3 % records, 12-channel scan +0.5 ms,
// profiles/r4/tz), a power of two, 128 at least
inline uint32_t bloom_blocks(int64_t n_edges) {
    const int64_t bits = n_edges * 48;
    uint32_t blocks = 128;
    while ((int64_t)blocks * 512 < bits) blocks *= 2;
    return blocks;
}

// ---------------------------------------------------------------------------
// applying an assignment (ctg_take.hip)
// ---------------------------------------------------------------------------
// voxels a workgroup of the apply kernel takes: 256 lanes x 2 voxels x 8 steps
constexpr int64_t TAKE_CHUNK = 4096;

// slots of the hash table of n (key, value) pairs: a power of two of at least
// 2 n, so linear probing always meets a free slot, and at least 64
inline uint64_t take_capacity(int64_t n) {
    uint64_t cap = 64;
    while (cap < 2 * (uint64_t)std::max<int64_t>(n, 0)) cap *= 2;
    return cap;
}

// Partial counters per segment for the nonzero voxels: a wave adds its count
// once, and adds to one address queue up behind each other (about 12 ns each:
// 2^20 waves of a 1024^3 volume took 12.8 ms on one counter, DESIGN.md 5
// "Write"), so the workgroups of a segment spread over this many counters,
// which the host sums.  One where the segments are many -- and then short.
inline int take_count_slots(int64_t n_seg) { return n_seg <= 4096 ? 64 : 1; }

struct TakeChunks {
    // BAD_SEGMENTS: seg_begin does not ascend from 0 to n; TOO_MANY_CHUNKS: the
    // launch would pass 2^31 - 1 workgroups
    enum Error { OK, BAD_SEGMENTS, TOO_MANY_CHUNKS } error = OK;
    std::vector<uint32_t> prefix;   // chunks of the launch before segment k; n_seg + 1 entries
};

// The workgroups of one apply launch over the segments [seg_begin[k],
// seg_begin[k + 1]) of a flat array of n voxels: segment k gets
// ceil(length / chunk) of them, none where it is empty.  seg_begin null: one
// segment [0, n) (n_seg is not looked at).
inline TakeChunks take_chunk_prefix(const int64_t* seg_begin, int64_t n_seg, int64_t n, int64_t chunk) {
    TakeChunks t;
    const int64_t whole[2] = {0, n};
    if (!seg_begin) {
        seg_begin = whole;
        n_seg = 1;
    }
    if (n_seg < 0 || n < 0 || (n_seg == 0 && n != 0) || (n_seg > 0 && (seg_begin[0] != 0 || seg_begin[n_seg] != n))) {
        t.error = TakeChunks::BAD_SEGMENTS;
        return t;
    }
    t.prefix.assign((size_t)n_seg + 1, 0);
    for (int64_t k = 0; k < n_seg; ++k) {
        const int64_t len = seg_begin[k + 1] - seg_begin[k];
        if (len < 0) {
            t.error = TakeChunks::BAD_SEGMENTS;
            return t;
        }
        const int64_t c = (len + chunk - 1) / chunk;
        if ((int64_t)t.prefix[k] + c > 0x7FFFFFFFll) {
            t.error = TakeChunks::TOO_MANY_CHUNKS;
            return t;
        }
        t.prefix[k + 1] = t.prefix[k] + (uint32_t)c;
    }
    return t;
}

// ---------------------------------------------------------------------------
// thresholded components (ctg_cc.hip)
// ---------------------------------------------------------------------------
// a labelling tile: TILE_X x CC_TILE_Y x CC_TILE_Z voxels, a wave per row
constexpr int CC_TILE_Y = 8, CC_TILE_Z = 16;
constexpr int CC_ROWS = CC_TILE_Y * CC_TILE_Z;
// nodes a wave of the numbering pass takes, 64 a step.  2048: the one-workgroup scan of the
// segments' root counts took 0.31 ms of a 512^3 call with 512
constexpr int64_t CC_SEG = 2048;
// node indices are u32 and 0xFFFFFFFF marks the background: boxes and label
// counts stay below 2^32
constexpr int64_t CC_MAX_NODES = 1ll << 32;
inline bool cc_nodes_fit(uint64_t n) { return n < (uint64_t)CC_MAX_NODES; }
inline int64_t cc_segments(int64_t nodes) { return (nodes + CC_SEG - 1) / CC_SEG; }

// The earlier rows (dz, dy) of a tile that a row is united with, and whether
// the neighbour row is dilated by one in x.  Connectivity c joins voxels with
// 0 < |dz| + |dy| + |dx| <= c: 1: the two straight rows, undilated; 2: those
// dilated, the two diagonal rows undilated; 3: all four dilated.
struct CcRows {
    int n;
    int dz[4], dy[4], dil[4];
};
constexpr CcRows cc_neighbor_rows(int c) {
    return c <= 1 ? CcRows{2, {0, -1, 0, 0}, {-1, 0, 0, 0}, {0, 0, 0, 0}}
         : c == 2 ? CcRows{4, {0, -1, -1, -1}, {-1, 0, -1, 1}, {1, 1, 0, 0}}
                  : CcRows{4, {0, -1, -1, -1}, {-1, 0, -1, 1}, {1, 1, 1, 1}};
}

struct CcGrid {
    int64_t nt[3];     // tiles along z, y, x
    int64_t tiles;
    // voxels on the low x, y, z face of a tile that has a tile below it on that
    // axis: one seam thread each (a voxel on two faces is counted on both and
    // taken by the first)
    int64_t seam[3];
    int64_t seam_threads;
    int64_t segs;      // waves of the numbering pass
};
// n: the box (z, y, x)
inline CcGrid cc_grid(const int64_t* n) {
    CcGrid g{};
    g.nt[0] = (n[0] + CC_TILE_Z - 1) / CC_TILE_Z;
    g.nt[1] = (n[1] + CC_TILE_Y - 1) / CC_TILE_Y;
    g.nt[2] = (n[2] + TILE_X - 1) / TILE_X;
    g.tiles = g.nt[0] * g.nt[1] * g.nt[2];
    const bool some = g.tiles > 0;
    g.seam[0] = some ? (g.nt[2] - 1) * n[0] * n[1] : 0;
    g.seam[1] = some ? (g.nt[1] - 1) * n[0] * n[2] : 0;
    g.seam[2] = some ? (g.nt[0] - 1) * n[1] * n[2] : 0;
    g.seam_threads = g.seam[0] + g.seam[1] + g.seam[2];
    g.segs = cc_segments(n[0] * n[1] * n[2]);
    return g;
}

// Seam thread i of a box with n1 x n2 voxels per plane: first the x faces
// (every 64th column), then the y faces, then the z faces.  take: false for a
// voxel that an earlier face holds already.
struct CcSeamVoxel {
    bool take;
    int64_t z, y, x;
};
constexpr CcSeamVoxel cc_seam_voxel(const CcGrid& g, int64_t n1, int64_t n2, int64_t i) {
    if (i < g.seam[0]) {
        const int64_t k = i % (g.nt[2] - 1), r = i / (g.nt[2] - 1);
        return {true, r / n1, r % n1, (k + 1) * TILE_X};
    }
    i -= g.seam[0];
    if (i < g.seam[1]) {
        const int64_t x = i % n2, r = i / n2;
        return {!(x && x % TILE_X == 0), r / (g.nt[1] - 1), (r % (g.nt[1] - 1) + 1) * CC_TILE_Y, x};
    }
    i -= g.seam[1];
    const int64_t x = i % n2, r = i / n2, y = r % n1;
    return {!((x && x % TILE_X == 0) || (y && y % CC_TILE_Y == 0)), (r / n1 + 1) * CC_TILE_Z, y, x};
}
// Whether the voxel at (z, y, x) takes its neighbour at offset (dz, dy, dx): a
// neighbour of connectivity c that lies across a low face of the voxel's tile.
// Of every neighbour pair that spans two tiles, one voxel sits on the low face
// between them, so these are all the unions the tiles left out.
constexpr bool cc_seam_partner(int c, int64_t z, int64_t y, int64_t x, int dz, int dy, int dx) {
    const int norm = (dz != 0) + (dy != 0) + (dx != 0);
    if (norm == 0 || norm > c) return false;
    return (dx == -1 && x && x % TILE_X == 0) || (dy == -1 && y && y % CC_TILE_Y == 0) ||
           (dz == -1 && z && z % CC_TILE_Z == 0);
}

// ---------------------------------------------------------------------------
// the exact Euclidean distance transform (ctg_edt.hip)
// ---------------------------------------------------------------------------
// offsets travel as u16 and 0xFFFF marks "no seed": an axis stays below 2^15
constexpr int64_t EDT_MAX_AXIS = 32768;
constexpr int64_t EDT_MAX_VOXELS = 1ll << 32;
constexpr int EDT_ROW_WORDS = (int)(EDT_MAX_AXIS / 64);   // 64-bit seed words of the longest row
constexpr int EDT_ROW_SUPER = EDT_ROW_WORDS / 64;         // one bit per word above them
constexpr int EDT_X_WAVES = 4;                            // rows a workgroup of the x pass takes at a time
constexpr int64_t EDT_X_MAX_GRID = 8192;
// Envelope passes: a workgroup is one wave, a lane per column, and each lane
// keeps a stack of up to `line` 8-byte entries (ctg_edt.h).  Up to
// EDT_LDS_LINE entries the stack lives in LDS: 64 lanes x 32 x 8 B = 16 KiB a
// wave, ten waves in a CU's 160 KiB (with 64 entries and five waves the z pass
// of a sparse 64 x 1024 x 1024 box took 0.61 ms against 0.26 ms one line
// longer, in the buffer: DESIGN.md 5).  Longer lines keep it in a call-sized
// buffer laid out [depth][workgroup][lane], so lanes at equal depth coalesce;
// the grid shrinks until the buffer fits EDT_STACK_BYTES (the workgroups then
// stride over the column groups).
constexpr int EDT_LDS_LINE = 32;
constexpr int64_t EDT_LINE_MAX_GRID = 8192;
constexpr int64_t EDT_STACK_BYTES = 1ll << 30;
struct EdtLinePlan {
    int lds;              // 1: the stack in LDS; 0: in the workspace buffer
    int64_t groups;       // groups of 64 columns
    int64_t grid;         // workgroups, each striding over the groups
    int64_t stack_bytes;  // the workspace buffer (0 with lds)
};
// line: the line's length; outer: rows of columns (z for the y pass, y for the
// z pass); nx: columns per row
inline EdtLinePlan edt_line_plan(int64_t line, int64_t outer, int64_t nx) {
    EdtLinePlan p{};
    p.lds = line <= EDT_LDS_LINE;
    p.groups = outer * ((nx + TILE_X - 1) / TILE_X);
    const int64_t per_wg = line * TILE_X * 8;
    const int64_t cap = p.lds ? EDT_LINE_MAX_GRID
                              : std::max<int64_t>(1, std::min(EDT_LINE_MAX_GRID, EDT_STACK_BYTES / std::max<int64_t>(per_wg, 1)));
    p.grid = std::min(p.groups, cap);
    p.stack_bytes = p.lds ? 0 : p.grid * per_wg;
    return p;
}
// workgroups of the x pass over `rows` rows
inline int64_t edt_x_grid(int64_t rows) {
    return std::min<int64_t>((rows + EDT_X_WAVES - 1) / EDT_X_WAVES, EDT_X_MAX_GRID);
}
// Which passes a box of n (z, y, x) runs after the x pass, which always runs
// (it reads the source): the y pass writes offsets for a z pass to follow, or,
// with no z pass (2-D mode, or one slice), the result; a z pass over a box of
// one row per slice reads the x pass's output directly.
struct EdtPasses {
    bool y, z;   // y: the y pass runs (it always does unless the z pass reads the rows directly)
};
inline EdtPasses edt_passes(const int64_t* n, bool two_d) {
    const bool z = !two_d && n[0] > 1;
    return {!(z && n[1] == 1), z};
}

// ---------------------------------------------------------------------------
// the seeded watershed (ctg_ws.hip)
// ---------------------------------------------------------------------------
// an edge id is 3 * (box-linear index) + axis in 32 bits, and bit 31 of a parent
// entry is a flag (ctg_ws.h): a box holds at most 2^30 voxels
constexpr int64_t WS_MAX_VOXELS = 1ll << 30;
constexpr int WS_THREADS = 256;
// a thread per voxel up to this many workgroups, which then stride: a launch's
// counters take one atomic per workgroup
constexpr int64_t WS_MAX_GRID = 4096;
inline int64_t ws_grid(int64_t n) { return std::min<int64_t>((n + WS_THREADS - 1) / WS_THREADS, WS_MAX_GRID); }
// Rounds that suffice for U unseeded voxels: every round at least halves the
// seedless components that still have an edge leaving them, at most U at the
// start, so after ceil(log2(U + 1)) rounds none is left, and one more round
// finds nothing to pick and ends the flood.
inline int ws_round_cap(int64_t U) { return bits_u(U) + 1; }
// Chase launches that suffice after a round's hooks: a chain is shorter than
// 2^30 entries and a launch leaves every entry WS_CHASE_STEPS = 2^6 entries
// further up its chain, or at the root: five launches reach it, the sixth
// finds nothing short.
constexpr int WS_CHASE_LAUNCHES = 6;
struct WsPlan {
    int64_t voxels;
    int64_t grid;            // workgroups of every per-voxel launch
    int64_t parent_bytes;    // u32 per voxel: the forest
    int64_t key_bytes;       // u32 per voxel: k of the height
    int64_t best_bytes;      // u64 per voxel: a root's smallest (max, min) this round, then what it hooks below
    int64_t pick_bytes;      // u32 per voxel: a root's edge id
    int64_t slices;          // domains: 1, or the z-slices in 2-D mode
};
inline WsPlan ws_plan(const int64_t* n, bool two_d) {
    WsPlan p{};
    p.voxels = n[0] * n[1] * n[2];
    p.grid = ws_grid(p.voxels);
    p.parent_bytes = p.key_bytes = p.pick_bytes = p.voxels * 4;
    p.best_bytes = p.voxels * 8;
    p.slices = two_d ? n[0] : 1;
    return p;
}

// ---------------------------------------------------------------------------
// the multi-GPU exchange's count matrix: counts_all[(src * world + dst) * 2]
// rows and [.. + 1] nodes of src's table that dst owns
// ---------------------------------------------------------------------------
// The segments of one direction of a rank's exchange, in rank order of the
// other side: a pair with rows or nodes has a segment (its rows, row_words
// words each, then its node ids), a pair with neither has none, and the rank
// itself never has one.  Passed by value to the kernels (ctg_mgpu.hip).
struct ExchangeSegs {
    int64_t row0[CTG_MGPU_MAX_WORLD + 1];    // rows of the segments before segment i; [n]: all rows
    int64_t node0[CTG_MGPU_MAX_WORLD + 1];   // the same of the node ids
    int64_t w_off[CTG_MGPU_MAX_WORLD + 1];   // word offset of segment i in the buffer; [n]: its words
    // send side: where segment i's rows / node ids start in this rank's table
    int64_t e_start[CTG_MGPU_MAX_WORLD], n_start[CTG_MGPU_MAX_WORLD];
    int n;
    constexpr int64_t rows() const { return row0[n]; }
    constexpr int64_t nodes() const { return node0[n]; }
    constexpr int64_t words() const { return w_off[n]; }
};

// The segment that holds element i of a prefix table (prefix[s] <= i <
// prefix[s + 1]; an empty segment holds nothing), for 0 <= i < prefix[n].
// Linear: at most CTG_MGPU_MAX_WORLD segments, mostly a handful.
CTG_HD constexpr int seg_of(const int64_t* prefix, int n, int64_t i) {
    int s = 0;
    while (s + 1 < n && prefix[s + 1] <= i) ++s;
    return s;
}

// Everything the host derives from the count matrix for one rank
// (1 <= world <= CTG_MGPU_MAX_WORLD, 0 <= rank < world).
struct ExchangePlan {
    int64_t e_lo, e_cnt, n_lo, n_cnt;   // the own range: rows / node ids this rank keeps, in its table
    int64_t rows, nodes;                // of this rank's table, over all destinations
    ExchangeSegs send, recv;            // what leaves for / arrives from every other rank
    bool any;                           // some rank sends something: the same answer on every rank
    // the merge's row indices, run heads and output positions are u32
    constexpr bool too_large() const {
        return recv.rows() >= (1ll << 32) || e_cnt + recv.rows() >= (1ll << 32) || recv.nodes() >= (1ll << 32);
    }
};

inline ExchangePlan exchange_plan(const int64_t* counts_all, int world, int rank, int row_words = CTG_MGPU_ROW_WORDS) {
    ExchangePlan p{};
    auto push = [row_words](ExchangeSegs& S, int64_t rows, int64_t nodes, int64_t e_start, int64_t n_start) {
        S.e_start[S.n] = e_start;
        S.n_start[S.n] = n_start;
        ++S.n;
        S.row0[S.n] = S.row0[S.n - 1] + rows;
        S.node0[S.n] = S.node0[S.n - 1] + nodes;
        S.w_off[S.n] = S.w_off[S.n - 1] + rows * row_words + nodes;
    };
    for (int q = 0; q < world; ++q) {
        const int64_t* to = counts_all + ((int64_t)rank * world + q) * 2;     // this rank -> q
        const int64_t* from = counts_all + ((int64_t)q * world + rank) * 2;   // q -> this rank
        if (q == rank) {
            p.e_lo = p.rows, p.e_cnt = to[0];
            p.n_lo = p.nodes, p.n_cnt = to[1];
        } else {
            if (to[0] || to[1]) push(p.send, to[0], to[1], p.rows, p.nodes);
            if (from[0] || from[1]) push(p.recv, from[0], from[1], 0, 0);
        }
        p.rows += to[0];
        p.nodes += to[1];
    }
    for (int64_t i = 0; i < (int64_t)world * world && !p.any; ++i)
        p.any = i / world != i % world && (counts_all[2 * i] || counts_all[2 * i + 1]);
    return p;
}

// The z planes of a rank's slab: owned [z0, z1), read from read_begin -- as
// many halo planes below z0 as a face (1) or an offset reaches down.  up: the
// reach above, for which the layout has no halo.
struct SlabRange {
    int64_t down, up;
    int64_t read_begin, z0, z1;
};
inline SlabRange slab_range(int64_t Z, int world, int rank, const int64_t* offsets, int n_channels) {
    SlabRange r{1, 0, 0, Z * rank / world, Z * (rank + 1) / world};
    for (int c = 0; c < n_channels; ++c) {
        r.down = std::max<int64_t>(r.down, -offsets[3 * c]);
        r.up = std::max<int64_t>(r.up, offsets[3 * c]);
    }
    r.read_begin = r.z0 - std::min(r.down, r.z0);
    return r;
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

// What the reduce asks of a key before it is an edge.  0: nothing (boundary
// maps, graphs, and affinities whose nearest-neighbour channels prove every
// edge); 1: some record of the key carries the ADJ bit (also: drop the Bloom
// filter's false positives); 2: the same, decided after a merge
// (CTG_NO_ADJ_FILTER: a partial table)
inline int need_adj_whole(int n_channels, bool skip_adj_marks, bool adj_filter, bool have_bloom) {
    if (have_bloom) return 1;
    return n_channels > 0 && !skip_adj_marks ? (adj_filter ? 1 : 2) : 0;
}
// batched blocks.  boundary / graph: every key is a face of the block's graph
// box; affinities: keep the keys of the block's sub-graph (ADJ marks)
inline int need_adj_blocks(int n_channels) { return n_channels > 0 ? 1 : 0; }

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

// ---------------------------------------------------------------------------
// bucket geometry of the packed-key bucket sort (ctg_sort.hip: bucket_sort_keys)
// ---------------------------------------------------------------------------
constexpr int BK_MAX_BITS = 12;  // at most 4096 buckets (LDS counters)

// bucket bits for n keys of key_bits bits: ~1 K keys per bucket
inline int bucket_bits(int64_t n, int key_bits) {
    int bb = 1;
    while (bb < BK_MAX_BITS && (n >> (bb + 10)) > 0) ++bb;
    return std::min(bb, key_bits);
}

// The bucket a key of either sort goes to, and the bucket bits of a key
// rebuilt from its bucket.  A key's bits above `shift` less those of the
// smallest key (bk0) are its bucket.  The index is formed modulo 2^32: the
// true difference (pk >> shift) - bk0 lies in [0, nbk) with nbk <= 2^16, so
// its low 32 bits are the difference itself however large pk >> shift and bk0
// are.  The way back is not modular: b + bk0 passes 2^32 for labels near 2^30
// and above (shift <= 29 at nb = 31), so the sum is formed in 64 bits.
CTG_HD inline uint32_t gs_bucket_of(uint64_t pk, int shift, uint64_t bk0) {
    return (uint32_t)(pk >> shift) - (uint32_t)bk0;
}
CTG_HD inline uint64_t gs_bucket_key(uint32_t b, uint64_t bk0, int shift) { return ((uint64_t)b + bk0) << shift; }

struct BucketKeysPlan {
    bool ok;        // false: an argument out of range (nothing else is set)
    int bb;         // bucket bits aimed at
    int shift;      // bucket = gs_bucket_of(key, shift, bk0)
    uint32_t nbk;   // <= 2^bb
    uint64_t bk0;
};

// n keys with key bits [lo_bit, hi_bit) (slot bits below), all in [kmin, kmax].
// 2^bb buckets over [kmin, kmax] (every key lies there), not over [0,
// 2^hi_bit): a z-slab's labels start far above 0, and buckets over the
// whole key domain put its keys in a few of them (rank 3 of 8 of the
// weak-scaling 512^3 slabs: sort + segment 0.10 -> 0.24 ms, the large
// segments of the segmented sort).  The smallest shift (down to lo_bit, where
// the buckets are the keys) at which 2^bb buckets still cover the range: runs
// of equal key bits never cross a bucket.
inline BucketKeysPlan plan_bucket_keys(int64_t n, int lo_bit, int hi_bit, uint64_t kmin, uint64_t kmax) {
    BucketKeysPlan p{};
    if (n <= 0 || n > 0xFFFFFFFFll || hi_bit > 64 || lo_bit < 0 || hi_bit <= lo_bit || kmin > kmax) return p;
    p.bb = bucket_bits(n, hi_bit - lo_bit);
    p.shift = hi_bit - p.bb;
    while (p.shift > lo_bit && (kmax >> (p.shift - 1)) - (kmin >> (p.shift - 1)) < (1ull << p.bb)) --p.shift;
    const uint64_t nbk = (kmax >> p.shift) - (kmin >> p.shift) + 1;
    if (nbk > (1ull << BK_MAX_BITS)) return p;   // kmax past 2^hi_bit: the counters would not hold it
    p.nbk = (uint32_t)nbk;
    p.bk0 = kmin >> p.shift;
    p.ok = true;
    return p;
}

// ---------------------------------------------------------------------------
// bucket geometry of the group sort (ctg_sort.hip: group_sort_runs)
// ---------------------------------------------------------------------------
constexpr int GS_CAP = 8192;       // items of one bucket in LDS (512 threads x 16: ctg_sort.hip)
constexpr int GS_TARGET = 3072;    // records per bucket aimed at
constexpr int GS_BB_MAX = 16;      // 64 K buckets
constexpr int GS_M = 1 << GS_BB_MAX;
constexpr int GS_GB = 11;          // group bits of the in-bucket counting sort

struct GroupSortPlan {
    // why the group sort declines (the caller sorts another way).  N_RANGE: no
    // record or 2^32 and more; KEY_BITS: ub + nb > 63 (bit 63 marks a run
    // head); ITEM_BITS: shift + ib > 64, the bucket-local key and the slot do
    // not fit one item; LOW_BITS: shift - min(GS_GB, shift) > 32, the key bits
    // below the group bits do not fit the 32-bit LDS words; BUCKET_CAP: not
    // the plan's -- the host read a bucket above GS_CAP from the device
    enum Why { OK = 0, N_RANGE = 1, KEY_BITS = 2, ITEM_BITS = 3, LOW_BITS = 4, BUCKET_CAP = 5 } why;
    int shift;                 // bucket = gs_bucket_of(packed key, shift, bk0); -1 before it is chosen
    uint32_t nbk;              // <= GS_M
    uint64_t bk0;              // bucket of the smallest key (a slab's labels start far above 0): up to 63 - shift bits
    uint64_t min_pk, max_pk;   // every packed key (u << nb) | v lies between them
    bool ok() const { return why == OK; }
};

// n records with keys (u, v), min_label <= u < v <= max_label, packed as
// (u << nb) | v (ub: bits of u); ib: slot bits of an item.
// Buckets of 2^shift packed keys from the smallest to the largest key: the
// largest shift whose buckets average at most GS_TARGET records, and at most
// GS_M buckets.  The range starts at the smallest u, not at 0: a z-slab of
// rank r of N holds labels from about r/N of the volume's label range, and
// buckets over [0, max] put its records in the top (N - r)/N of them -- past
// GS_CAP per bucket (the onesweep fallback, twice the sort time) from rank 3
// of 8 on.
inline GroupSortPlan plan_group_sort(int64_t n, int nb, int ub, int ib, uint64_t min_label, uint64_t max_label) {
    GroupSortPlan p{};
    p.shift = -1;
    p.why = GroupSortPlan::N_RANGE;
    if (n <= 0 || n > 0xFFFFFFFFll) return p;
    const int kb = ub + nb;
    p.why = GroupSortPlan::KEY_BITS;
    if (kb > 63) return p;
    const uint64_t umax = (1ull << ub) - 1ull;
    p.max_pk = (std::min<uint64_t>(max_label, umax) << nb) | max_label;
    p.min_pk = std::min<uint64_t>(std::min<uint64_t>(min_label, max_label), umax) << nb;
    const uint64_t lo = p.min_pk, hi = p.max_pk;
    auto nbk_at = [lo, hi](int sh) { return (hi >> sh) - (lo >> sh) + 1; };
    int shift = kb;
    while (shift > 0 && nbk_at(shift - 1) <= (uint64_t)GS_M && (double)n / (double)nbk_at(shift) > (double)GS_TARGET)
        --shift;
    while (nbk_at(shift) > (uint64_t)GS_M) ++shift;
    p.shift = shift;
    p.nbk = (uint32_t)nbk_at(shift);
    p.bk0 = lo >> shift;
    p.why = shift + ib > 64                       ? GroupSortPlan::ITEM_BITS
            : shift - std::min(GS_GB, shift) > 32 ? GroupSortPlan::LOW_BITS
                                                  : GroupSortPlan::OK;
    return p;
}

// What ctg_last_sort reports of a workspace's last record sort (ctg.h: the
// CTG_SORT_* words).  Host values only.
struct SortReport {
    int path = -1;      // SortPath, 5: the group sort, -1: no record
    int packed = 0;
    int group_tried = 0, group_done = 0;
    GroupSortPlan group{GroupSortPlan::OK, -1, 0, 0, 0, 0};   // as far as the group sort got
    int64_t largest = -1;   // the largest bucket the host read (-1: none read)
    int ib = 0, nb = 0, ub = 0;
    int64_t n = 0;
};

}  // namespace ctg
