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
//
// g++ -std=c++17 -fsanitize=address,undefined tools/plan_check.cpp -o plan_check
#include <cinttypes>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

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
        } else {
            fprintf(stderr, "plan_check: unknown query '%s'\n", cmd.c_str());
            return 2;
        }
    }
    return 0;
}
