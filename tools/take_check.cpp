// Host driver of csrc/ctg_take.h (the hash table of the sparse assignment: the
// same hash, insert and lookup the kernels run) and of the two plan functions
// of the apply call (csrc/ctg_plan.h) for tests/test_take_host.py: reads one
// query per line from stdin and prints the answer, one line each.
//
//   cap N                          -> take_capacity
//   slots N_SEG                    -> take_count_slots
//   chunks CHUNK N HAS_SEG N_SEG b[N_SEG + 1]
//                                  -> error prefix...   (error: 0 ok, 1 bad segments, 2 too many chunks)
//   build N k v k v ...            -> duplicates capacity   (the table stays for `look`; inserts run in the
//                                     order given, with a plain compare-and-store for the device's CAS)
//   look N q ...                   -> per query its value, or - where the table does not hold it
//
// g++ -std=c++17 -fsanitize=address,undefined tools/take_check.cpp -o take_check
#include <cinttypes>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../cluster_tools_amd/csrc/ctg_plan.h"
#include "../cluster_tools_amd/csrc/ctg_take.h"

using namespace ctg;

int main() {
    std::string line;
    std::vector<uint64_t> table;
    uint64_t cap = 0;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd;
        if (!(in >> cmd)) continue;
        if (cmd == "cap") {
            int64_t n;
            in >> n;
            printf("%" PRIu64 "\n", take_capacity(n));
        } else if (cmd == "slots") {
            int64_t n;
            in >> n;
            printf("%d\n", take_count_slots(n));
        } else if (cmd == "chunks") {
            int64_t chunk, n, n_seg;
            int has_seg;
            in >> chunk >> n >> has_seg >> n_seg;
            std::vector<int64_t> b((size_t)(has_seg ? n_seg + 1 : 0));
            for (int64_t& v : b) in >> v;
            const TakeChunks t = take_chunk_prefix(has_seg ? b.data() : nullptr, n_seg, n, chunk);
            printf("%d", (int)t.error);
            if (t.error == TakeChunks::OK)
                for (uint32_t p : t.prefix) printf(" %u", p);
            printf("\n");
        } else if (cmd == "build") {
            int64_t n;
            in >> n;
            cap = take_capacity(n);
            table.assign((size_t)take_table_words(cap), TAKE_FREE);
            table[2 * cap] = table[2 * cap + 1] = 0;
            int64_t dups = 0;
            for (int64_t i = 0; i < n; ++i) {
                uint64_t k, v;
                in >> k >> v;
                dups += take_insert(
                    table.data(), cap, k, v,
                    [](uint64_t* p, uint64_t expect, uint64_t want) {
                        const uint64_t cur = *p;
                        if (cur == expect) *p = want;
                        return cur;
                    },
                    [](uint64_t* p) { return (*p)++; });
            }
            printf("%" PRId64 " %" PRIu64 "\n", dups, cap);
        } else if (cmd == "look") {
            int64_t n;
            in >> n;
            if (table.empty()) {
                fprintf(stderr, "take_check: look before build\n");
                return 2;
            }
            for (int64_t i = 0; i < n; ++i) {
                uint64_t q, v = 0;
                in >> q;
                if (take_lookup(table.data(), cap, q, &v)) printf("%s%" PRIu64, i ? " " : "", v);
                else printf("%s-", i ? " " : "");
            }
            printf("\n");
        } else {
            fprintf(stderr, "take_check: unknown query '%s'\n", cmd.c_str());
            return 2;
        }
    }
    return 0;
}
