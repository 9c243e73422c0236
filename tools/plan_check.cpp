// Host driver of csrc/ctg_plan.h for tests/test_plan.py: reads one query per
// line from stdin and prints the plan's answer, one line each.
//
//   bits V                                   -> bits_for
//   tile Z Y X ROWS_WIDE ROWS_NARROW          -> tile_z tile_z_narrow
//   sort HAS_KEYS HAS_REGIONS N UB NB IB SPREAD PACKED BUCKET BUCKET_PAIRS GROUP GROUP_FIRST
//                                            -> packed try_group path
//   chan ADJ_FILTER HAVE_BLOOM SKIP_ADJ NN N  z y x ...   (N offsets)
//        -> lr_mask long_range nn_z nn_y nn_x skip_adj_marks nn3 nn_mix n_loop loop...
//   range MIN_U MAX_V NB IB                   -> kmin kmax
//   box SZ SY SX HAS_BEGIN bz by bx HAS_END ez ey ex MAX_VOXELS
//                                            -> error bz by bx ez ey ex voxels   (error: 0 ok, 1 outside, 2 too large)
//   volbox SZ SY SX bz by bx ez ey ex        -> s_z s_y base nz ny nx   (vol_box of call_box of the box)
//   blocks N HAS_DATA N_CHANNELS LABELS_LEN DATA_LEN MAX_X SCAN_ROWS UNIQUE_ROWS TILE_Z_SWITCH
//          then per block: label_offset data_offset shape[3] own_begin[3] own_end[3] graph_begin[3] graph_end[3]
//        -> error bad_block   (error: 1 box outside, 2 array outside), or
//           error own_voxels voxels tile_z tag_bits tag_shift label_hi_mask  prefix[N+1]  uprefix[N+1]
//           ntx nty ntz per block   (error: 0 ok, 3 too many tiles -- the tables up to that block)
//   recfirst CAP V                           -> record slots of the first scan
//   recgrow FULLEST                          -> record slots after an overflow
//   cand N                                   -> first candidate capacity
//   candgrow M BOUND                         -> regrown candidate capacity
//   bloom N_EDGES                            -> 64-byte blocks
//   narrow BOUNDARY_MAP V SWITCH             -> narrow-row mode
//   adj N_CHANNELS SKIP_MARKS ADJ_FILTER HAVE_BLOOM -> need_adj of a whole-array call
//   adjblocks N_CHANNELS                     -> need_adj of a batched call
//   fold r[NREG]                             -> total fullest off[NREG + 1]
//   xchg WORLD RANK ROW_WORDS RECEIVE counts[WORLD * WORLD * 2] -> rows nodes words   (of exchange_plan)
//   xplan WORLD RANK counts[WORLD * WORLD * 2]
//        -> e_lo e_cnt n_lo n_cnt rows nodes any too_large, then for the send and the receive table:
//           n  (row0 node0 w_off)[n + 1]  (e_start n_start)[n]
//   segof I N prefix[N + 1]                  -> seg_of
//   slab Z WORLD RANK N  z y x ...   (N offsets) -> down up read_begin z0 z1
//   gsort N NB UB IB MIN_LABEL MAX_LABEL     -> why shift nbk bk0 min_pk max_pk   (why: GroupSortPlan::Why; shift -1,
//                                               the rest 0 where it declined before choosing)
//   gskey PK SHIFT BK0                       -> gs_bucket_of(pk)  gs_bucket_key(that bucket)
//   bkeys N LO_BIT HI_BIT KMIN KMAX          -> ok bb shift nbk bk0
//
// g++ -std=c++17 -fsanitize=address,undefined tools/plan_check.cpp -o plan_check
#include <cinttypes>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../cluster_tools_amd/csrc/ctg_plan.h"

using namespace ctg;

static const char* path_name(SortPath p) {
    switch (p) {
    case SortPath::BucketKeys: return "bucket_keys";
    case SortPath::OnesweepKeys: return "onesweep_keys";
    case SortPath::BucketPairs: return "bucket_pairs";
    case SortPath::OnesweepPairsWide: return "onesweep_pairs_wide";
    case SortPath::OnesweepPairsDefault: return "onesweep_pairs_default";
    }
    return "?";
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd;
        if (!(in >> cmd)) continue;
        if (cmd == "bits") {
            uint64_t v;
            in >> v;
            printf("%d\n", bits_for(v));
        } else if (cmd == "tile") {
            int64_t shape[3], rw, rn;
            in >> shape[0] >> shape[1] >> shape[2] >> rw >> rn;
            const TileDepths t = scan_tile_depths(shape, rw, rn);
            printf("%d %d\n", t.tile_z, t.tile_z_narrow);
        } else if (cmd == "sort") {
            int has_keys, has_regions, ub, nb, ib, spread, packed, bucket, group, group_first;
            int64_t n;
            SortSwitches sw;
            in >> has_keys >> has_regions >> n >> ub >> nb >> ib >> spread >> packed >> bucket >> sw.bucket_pairs >>
                group >> group_first;
            sw.packed = packed;
            sw.bucket = bucket;
            sw.group = group;
            sw.group_first = group_first;
            const RecordSortPlan p = plan_record_sort(has_keys, has_regions, n, ub, nb, ib, spread, sw);
            printf("%d %d %s\n", (int)p.packed, (int)p.try_group, path_name(p.path));
        } else if (cmd == "chan") {
            int adj_filter, have_bloom, skip_sw, nn_sw, n;
            in >> adj_filter >> have_bloom >> skip_sw >> nn_sw >> n;
            int off[CTG_MAX_CHANNELS][3] = {};
            for (int c = 0; c < n && c < CTG_MAX_CHANNELS; ++c) in >> off[c][0] >> off[c][1] >> off[c][2];
            const ChannelClass cc = classify_channels(off, n);
            const ChannelPlan cp = plan_channels(cc, n, adj_filter, have_bloom, skip_sw, nn_sw);
            printf("%u %d %d %d %d %d %d %d %d", cc.lr_mask, (int)cc.long_range, cc.nn_ch[0], cc.nn_ch[1], cc.nn_ch[2],
                   (int)cp.skip_adj_marks, (int)cp.nn3, (int)cp.nn_mix, cc.n_loop);
            for (int i = 0; i < cc.n_loop; ++i) printf(" %d", cc.loop_ch[i]);
            printf("\n");
        } else if (cmd == "range") {
            uint64_t min_u, max_v;
            int nb, ib;
            in >> min_u >> max_v >> nb >> ib;
            const KeyRange r = packed_key_range(min_u, max_v, nb, ib);
            printf("%" PRIu64 " %" PRIu64 "\n", r.kmin, r.kmax);
        } else if (cmd == "box") {
            int64_t shape[3], b[3] = {}, e[3] = {}, max_voxels;
            int has_b, has_e;
            in >> shape[0] >> shape[1] >> shape[2] >> has_b >> b[0] >> b[1] >> b[2] >> has_e >> e[0] >> e[1] >> e[2] >>
                max_voxels;
            const CallBox c = call_box(shape, has_b ? b : nullptr, has_e ? e : nullptr, max_voxels);
            printf("%d %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 "\n", (int)c.error,
                   c.b[0], c.b[1], c.b[2], c.e[0], c.e[1], c.e[2], c.voxels);
        } else if (cmd == "volbox") {
            int64_t shape[3], b[3], e[3];
            in >> shape[0] >> shape[1] >> shape[2] >> b[0] >> b[1] >> b[2] >> e[0] >> e[1] >> e[2];
            const VolBox v = vol_box(shape, call_box(shape, b, e, 0));
            printf("%" PRId64 " %" PRId64 " %" PRId64 " %u %u %u\n", v.s_z, v.s_y, v.base, v.n[0], v.n[1], v.n[2]);
        } else if (cmd == "blocks") {
            int n, has_data, nch, rows, urows, tz;
            int64_t labels_len, data_len, max_x;
            in >> n >> has_data >> nch >> labels_len >> data_len >> max_x >> rows >> urows >> tz;
            std::vector<ctg_block_desc> d(n);
            for (ctg_block_desc& x : d) {
                in >> x.label_offset >> x.data_offset;
                for (int64_t* a : {x.shape, x.own_begin, x.own_end, x.graph_begin, x.graph_end}) in >> a[0] >> a[1] >> a[2];
            }
            const BlockPlan p = plan_blocks(d.data(), n, has_data, nch, labels_len, data_len, max_x, rows, urows, tz);
            if (p.error == BlockPlan::BOX_OUTSIDE || p.error == BlockPlan::ARRAY_OUTSIDE) {
                printf("%d %d\n", (int)p.error, p.bad_block);
                continue;
            }
            printf("%d %" PRId64 " %" PRId64 " %d %d %d %u ", (int)p.error, p.own_voxels, p.voxels, p.tile_z, p.tag_bits,
                   p.tag_shift, p.label_hi_mask);
            for (uint32_t v : p.prefix) printf(" %u", v);
            printf(" ");
            for (uint32_t v : p.uprefix) printf(" %u", v);
            printf(" ");
            for (const BlockGeom& g : p.geom) printf(" %d %d %d", g.ntx, g.nty, g.ntz);
            printf("\n");
        } else if (cmd == "recfirst") {
            int64_t cap, V;
            in >> cap >> V;
            printf("%" PRId64 "\n", record_slots_first(cap, V));
        } else if (cmd == "recgrow") {
            uint64_t mx;
            in >> mx;
            printf("%" PRId64 "\n", record_slots_regrow(mx));
        } else if (cmd == "cand") {
            int64_t n;
            in >> n;
            printf("%" PRId64 "\n", candidate_cap_first(n));
        } else if (cmd == "candgrow") {
            int64_t m, bound;
            in >> m >> bound;
            printf("%" PRId64 "\n", candidate_cap_regrow(m, bound));
        } else if (cmd == "bloom") {
            int64_t n;
            in >> n;
            printf("%u\n", bloom_blocks(n));
        } else if (cmd == "narrow") {
            int boundary, sw;
            int64_t V;
            in >> boundary >> V >> sw;
            printf("%d\n", narrow_rows_mode(boundary, V, sw));
        } else if (cmd == "adj") {
            int nch, skip, filter, bloom;
            in >> nch >> skip >> filter >> bloom;
            printf("%d\n", need_adj_whole(nch, skip, filter, bloom));
        } else if (cmd == "adjblocks") {
            int nch;
            in >> nch;
            printf("%d\n", need_adj_blocks(nch));
        } else if (cmd == "fold") {
            unsigned long long rc[NREG];
            for (unsigned long long& r : rc) in >> r;
            const RegionFold f = fold_regions(rc);
            printf("%" PRIu64 " %" PRIu64, f.total, f.fullest);
            for (uint32_t o : f.pre.off) printf(" %u", o);
            printf("\n");
        } else if (cmd == "xchg") {
            int world, rank, row_words, receive;
            in >> world >> rank >> row_words >> receive;
            std::vector<int64_t> c((size_t)world * world * 2);
            for (int64_t& v : c) in >> v;
            const ExchangePlan x = exchange_plan(c.data(), world, rank, row_words);
            printf("%" PRId64 " %" PRId64 " %" PRId64 "\n", x.rows, x.nodes, (receive ? x.recv : x.send).words());
        } else if (cmd == "xplan") {
            int world, rank;
            in >> world >> rank;
            std::vector<int64_t> c((size_t)world * world * 2);
            for (int64_t& v : c) in >> v;
            const ExchangePlan x = exchange_plan(c.data(), world, rank);
            printf("%" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 " %d %d", x.e_lo, x.e_cnt,
                   x.n_lo, x.n_cnt, x.rows, x.nodes, (int)x.any, (int)x.too_large());
            for (const ExchangeSegs* S : {&x.send, &x.recv}) {
                printf(" %d", S->n);
                for (int i = 0; i <= S->n; ++i) printf(" %" PRId64 " %" PRId64 " %" PRId64, S->row0[i], S->node0[i], S->w_off[i]);
                for (int i = 0; i < S->n; ++i) printf(" %" PRId64 " %" PRId64, S->e_start[i], S->n_start[i]);
            }
            printf("\n");
        } else if (cmd == "segof") {
            int n;
            int64_t i;
            in >> i >> n;
            std::vector<int64_t> prefix(n + 1);
            for (int64_t& v : prefix) in >> v;
            printf("%d\n", seg_of(prefix.data(), n, i));
        } else if (cmd == "slab") {
            int64_t Z;
            int world, rank, n;
            in >> Z >> world >> rank >> n;
            std::vector<int64_t> off(3 * (size_t)n + 1);
            for (int i = 0; i < 3 * n; ++i) in >> off[i];
            const SlabRange r = slab_range(Z, world, rank, off.data(), n);
            printf("%" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64 "\n", r.down, r.up, r.read_begin, r.z0, r.z1);
        } else if (cmd == "gsort") {
            int64_t n;
            int nb, ub, ib;
            uint64_t lo, hi;
            in >> n >> nb >> ub >> ib >> lo >> hi;
            const GroupSortPlan p = plan_group_sort(n, nb, ub, ib, lo, hi);
            printf("%d %d %u %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", (int)p.why, p.shift, p.nbk, p.bk0, p.min_pk,
                   p.max_pk);
        } else if (cmd == "gskey") {
            uint64_t pk, bk0;
            int shift;
            in >> pk >> shift >> bk0;
            const uint32_t b = gs_bucket_of(pk, shift, bk0);
            printf("%u %" PRIu64 "\n", b, gs_bucket_key(b, bk0, shift));
        } else if (cmd == "bkeys") {
            int64_t n;
            int lo_bit, hi_bit;
            uint64_t kmin, kmax;
            in >> n >> lo_bit >> hi_bit >> kmin >> kmax;
            const BucketKeysPlan p = plan_bucket_keys(n, lo_bit, hi_bit, kmin, kmax);
            printf("%d %d %d %u %" PRIu64 "\n", (int)p.ok, p.bb, p.shift, p.nbk, p.bk0);
        } else {
            fprintf(stderr, "plan_check: unknown query '%s'\n", cmd.c_str());
            return 2;
        }
    }
    return 0;
}
