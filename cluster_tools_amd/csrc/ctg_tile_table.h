// Tile-table scans: one workgroup walks a 64 x TILE_Y x TT_TILE_Z tile of a box
// of label voxels and gathers what it meets, per key, in an LDS hash table that
// it writes out as records.  The protocol ("Tile-table scans") is
// stated once, in tile_table_scan; k_overlap_scan, k_morph_scan, k_unique_tiles,
// k_unique_blocks and k_region_scan are policies over it.  The host half of such a scan --
// the record buffer that grows until it holds every record -- is
// scan_into_records.
#pragma once
#include <algorithm>

#include "ctg_internal.h"

namespace ctg {

constexpr int TT_THREADS = 256;   // 4 waves: a step of the walk takes 4 planes
constexpr int TT_TILE_Z = 16;
constexpr int TT_PROBES = 32;     // linear probes before a head gives up on a table (a set probes every slot)

inline dim3 grid_for(int64_t n) { return dim3((unsigned)((n + 255) / 256)); }

struct TileBox {            // the tile of this workgroup, in array indices
    int64_t Y, X;           // the array's rows per plane, voxels per row
    int64_t x0, y0, z0;     // the tile's first voxel
    int64_t ez, ey, ex;     // the box's end
};

// the tiles of the box [b, e), as a launch grid
inline hipError_t tile_grid(const int64_t* b, const int64_t* e, dim3* grid) {
    const int64_t gx = (e[2] - b[2] + WAVE - 1) / WAVE, gy = (e[1] - b[1] + TILE_Y - 1) / TILE_Y,
                  gz = (e[0] - b[0] + TT_TILE_Z - 1) / TT_TILE_Z;
    if (gx > 0x7FFFFFFFll || gy > 65535 || gz > 65535) return hipErrorInvalidValue;
    *grid = dim3((unsigned)gx, (unsigned)gy, (unsigned)gz);
    return hipSuccess;
}

#ifdef __HIPCC__
__device__ __forceinline__ TileBox tile_of_grid(int64_t Y, int64_t X, int64_t bz, int64_t by, int64_t bx, int64_t ez,
                                                int64_t ey, int64_t ex) {
    return TileBox{Y,  X,  bx + (int64_t)blockIdx.x * WAVE, by + (int64_t)blockIdx.y * TILE_Y,
                   bz + (int64_t)blockIdx.z * TT_TILE_Z, ez, ey, ex};
}

__device__ __forceinline__ uint32_t shfl_up1(uint32_t v) { return __shfl_up(v, 1, WAVE); }
__device__ __forceinline__ uint64_t shfl_up1(uint64_t v) { return shfl_up_u64(v); }
__device__ __forceinline__ uint32_t cas_key(uint32_t* p, uint32_t empty, uint32_t key) {
    return atomicCAS(p, empty, key);
}
__device__ __forceinline__ uint64_t cas_key(uint64_t* p, uint64_t empty, uint64_t key) {
    return atomicCAS((unsigned long long*)p, (unsigned long long)empty, (unsigned long long)key);
}
// rank of this lane among the set bits of m
__device__ __forceinline__ uint32_t ballot_rank(uint64_t m) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0));
}

// The scan of one tile by TT_THREADS threads.  A wave takes one row at a time,
// lane = x.  Equal consecutive keys of valid lanes collapse to their head lane
// (run length from the ballot of heads), and only heads touch the table: CAS on
// the key word, then the policy's adds.  A head that finds no slot within
// TT_PROBES, and the one key that looks like a free slot, write a record
// directly, one reservation per wave row.  After a step of 4 planes the table
// is written out if more than half full, and at tile end, with one reservation
// per flush.  Records past `cap` are dropped, but counted: the host runs again
// with room (scan_into_records).  The flush branch must be workgroup-uniform
// (it holds barriers): `used` is read after the barrier that follows every
// insert of the step, and a flush resets it between its two closing barriers.
// On the path without a flush no barrier separates that read from the next
// step's first insert; what keeps a fast wave's insert behind a slow wave's
// read is the global load every insert waits for.
//
// The policy P supplies what differs:
//   Key, EMPTY, CAP             the key type, its free-slot value, the table's entries
//   SET                         a set of keys: no payload and no Counters; every slot is probed, a
//                               head that still finds none is dropped, the flush ranks by one LDS add per key
//   HOLES                       valid lanes need not be a prefix of the row (an ignore label)
//   Key* keys                   the table's key words (LDS)
//   unsigned long long* count   the counter that record slots are reserved from
//   Counters* C                 n_direct and label_overflow (not SET)
//   load(p, in)                 what this lane reads at voxel p (in: inside the box along x), and of that:
//   valid(v, in), key(v),       whether the voxel counts, its key, and a counted voxel's label-overflow
//   overflow(v)                 bits -- all by value, so that they stay in registers as written
//   fold(v, valid, bound, lane) what a lane gathers from the other lanes of its run (Fold; NoFold: nothing):
//                               every lane of the wave calls it, before the heads part from the rest, so it
//                               may shuffle; bound is the ballot of the heads and the skipped lanes
//   head(run, lane, dy, lz, f)  what a head of `run` voxels at tile-local (lane, dy, lz) adds to its entry,
//   add(h, a)                   and the adding to entry h
//   put_direct(slot, key, run, z, y, x, f)   the record of a head that missed the table
//   put_flush(slot, e, key, t)  the record of entry e
//   clear(e)                    entry e back to free
struct NoFold {};   // the fold of a policy whose heads need nothing from their run's other lanes

template <class P>
__device__ __forceinline__ void tile_table_scan(const P& pol, const TileBox& t, int64_t cap) {
    using Key = typename P::Key;
    constexpr int CAP = P::CAP;
    static_assert((CAP & (CAP - 1)) == 0 && CAP % TT_THREADS == 0, "table capacity");
    __shared__ uint32_t used;
    __shared__ uint32_t wpos;
    __shared__ unsigned long long base;
    const int tid = threadIdx.x;
    for (int e = tid; e < CAP; e += TT_THREADS) pol.clear(e);
    if (tid == 0) used = 0;
    __syncthreads();
    const int lane = tid & (WAVE - 1), wave = tid >> 6;
    const int64_t x = t.x0 + lane;
    const bool in = x < t.ex;
    uint32_t over = 0;
    for (int zs = 0; zs < TT_TILE_Z; zs += TT_THREADS / WAVE) {
        const int lz = zs + wave;
        const int64_t z = t.z0 + lz;
        if (z < t.ez) {   // (wave-uniform, like the row bound below)
            for (int dy = 0; dy < TILE_Y; ++dy) {
                const int64_t y = t.y0 + dy;
                if (y >= t.ey) break;
                const auto v = pol.load((z * t.Y + y) * t.X + x, in);
                const bool valid = pol.valid(v, in);
                if (valid) over |= pol.overflow(v);
                const Key key = pol.key(v);
                const Key prev = shfl_up1(key);
                // (without holes, the lanes below a valid lane are valid too)
                const bool pvalid = !P::HOLES || __shfl_up((int)valid, 1, WAVE) != 0;
                const bool head = valid && (lane == 0 || !pvalid || prev != key);
                // a run ends before the next head or skipped lane
                const uint64_t bound = __ballot(head || !valid);
                const auto f = pol.fold(v, valid, bound, lane);
                bool direct = false;
                uint32_t run = 0;
                if (head) {
                    const uint64_t above = lane == WAVE - 1 ? 0ull : bound >> (lane + 1);
                    run = above ? (uint32_t)__ffsll((unsigned long long)above) : (uint32_t)(WAVE - lane);
                    direct = true;
                    if (key != P::EMPTY) {   // (the one key that looks like a free slot goes direct)
                        const auto a = pol.head(run, lane, dy, lz, f);
                        uint32_t h = hash_key(key) & (CAP - 1);
                        for (int q = 0; q < (P::SET ? CAP : TT_PROBES); ++q) {
                            Key cur = pol.keys[h];
                            if (cur == P::EMPTY) {
                                cur = cas_key(&pol.keys[h], P::EMPTY, key);
                                if (cur == P::EMPTY) {
                                    atomicAdd(&used, 1u);
                                    cur = key;
                                }
                            }
                            if (cur == key) {
                                pol.add(h, a);
                                direct = false;
                                break;
                            }
                            h = (h + 1) & (CAP - 1);
                        }
                    }
                }
                if constexpr (!P::SET) {
                    const uint64_t dm = __ballot(direct);
                    if (dm) {
                        const uint32_t n = (uint32_t)__popcll(dm);
                        const uint32_t rank = ballot_rank(dm);
                        unsigned long long b0 = 0;
                        if (lane == 0) {
                            b0 = atomicAdd(pol.count, (unsigned long long)n);
                            atomicAdd(&pol.C->n_direct, (unsigned long long)n);
                        }
                        b0 = bcast0_u64(b0);
                        if (direct && b0 + rank < (unsigned long long)cap) {
                            CTG_IDX(b0 + rank, cap);
                            pol.put_direct(b0 + rank, key, run, z, y, x, f);
                        }
                    }
                }
            }
        }
        __syncthreads();
        // (uniform: `used` is read after the barrier -- see above)
        if (used > CAP / 2 || zs + TT_THREADS / WAVE >= TT_TILE_Z) {
            if (tid == 0) {
                base = used ? atomicAdd(pol.count, (unsigned long long)used) : 0ull;
                wpos = 0;
            }
            __syncthreads();
            // compaction order is irrelevant (sorted afterwards)
            for (int e = tid; e < CAP; e += TT_THREADS) {
                const Key k = pol.keys[e];
                const bool live = k != P::EMPTY;
                // entry e leaves as record base + w, if the buffer holds that many
                const auto emit = [&](unsigned long long w) {
                    const unsigned long long slot = base + w;
                    if (slot < (unsigned long long)cap) {
                        CTG_IDX(slot, cap);
                        pol.put_flush(slot, e, k, t);
                    }
                    pol.clear(e);
                };
                if constexpr (P::SET) {
                    if (live) emit(atomicAdd(&wpos, 1u));
                } else {
                    const uint64_t m = __ballot(live);
                    if (m) {
                        const uint32_t rank = ballot_rank(m);
                        uint32_t w0 = 0;
                        if (lane == 0) w0 = atomicAdd(&wpos, (uint32_t)__popcll(m));
                        w0 = __shfl(w0, 0, WAVE);
                        if (live) emit((unsigned long long)w0 + rank);
                    }
                }
            }
            __syncthreads();
            if (tid == 0) used = 0;
            __syncthreads();
        }
    }
    if constexpr (!P::SET) {
        for (int o = 32; o > 0; o >>= 1) over |= (uint32_t)__shfl_xor((int)over, o, WAVE);
        if (lane == 0 && over) atomicOr(&pol.C->label_overflow, (unsigned long long)over);
    }
}
#endif   // __HIPCC__

// The host half: run a tile-table scan of a box of nb voxels into call-sized
// record buffers until they hold every record.  attempt(cap) makes buffers for
// cap records and launches the scan into them with w.counters; up to three
// attempts.  On success *overflow holds the scan's label-overflow bits (set:
// nothing else is valid, the caller relabels densely) and *m the records, whose
// direct share is w.counters_host->n_direct.  Marks phases 0 to 2.
template <class Attempt>
hipError_t scan_into_records(Workspace& w, int64_t nb, hipStream_t s, Attempt&& attempt, int64_t* m,
                             unsigned* overflow) {
    *overflow = 0;
    *m = 0;
    Ev ev{w, s};
    // a record per voxel at most; coarse labellings need a small fraction of that
    int64_t cap = std::min<int64_t>(nb, std::max<int64_t>(1 << 12, nb / 16));
    for (int a = 0; a < 3; ++a) {
        CTG_TRY(hipMemsetAsync(w.counters, 0, sizeof(Counters), s));
        ev.mark(0);
        CTG_TRY(attempt(cap));
        ev.mark(1);
        ev.mark(2);
        CTG_TRY(hipMemcpyAsync(w.counters_host, w.counters, sizeof(Counters), hipMemcpyDeviceToHost, s));
        CTG_TRY(hipStreamSynchronize(s));
        if (w.counters_host->label_overflow) {
            *overflow = (unsigned)w.counters_host->label_overflow;
            return hipSuccess;
        }
        *m = (int64_t)w.counters_host->n_records;
        if (*m <= cap) return hipSuccess;
        // which heads miss the table depends on the order of arrival, so a
        // second run may count a few more: the third gets a slot per voxel
        cap = a == 0 ? std::min<int64_t>(nb, *m + *m / 8 + 1024) : nb;
    }
    return hipErrorOutOfMemory;   // (unreachable: the third attempt holds every voxel)
}

}  // namespace ctg
