// The host-only plan of the Goldilocks stage-2 hints (csrc/hint_plan.h) in a program of its own, so that tests/test_hints_cpu.py can run it
// under the address and undefined-behaviour sanitizers.  Reads commands from the text file named on the command line and prints one JSON
// object per command:
//     plan n                       {"threads", "items", "chunk", "blocks", "totalsPerLane", "capacity", "capBits", "offTable", "offCnt",
//                                   "offStart", "offTotals", "offMissing", "words"}   the h1h2 fields are 0 for n > 2^30
//     home dim capacity w0 .. w(dim-1)   {"home": slot, "hash": the 64-bit hash}
// Exits non-zero when a command cannot be read.
#include <stdio.h>
#include <inttypes.h>
#include <string.h>
#include "hint_plan.h"

static bool rd(FILE *f, uint64_t *v) { return fscanf(f, "%" SCNu64, v) == 1; }

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    FILE *f = fopen(argv[1], "r");
    if (!f) return 2;
    char cmd[16];
    while (fscanf(f, "%15s", cmd) == 1) {
        if (!strcmp(cmd, "plan")) {
            uint64_t n;
            if (!rd(f, &n)) return 2;
            const uint64_t nb = hintplan::blocks(n);
            hintplan::H1H2Work w{};
            uint32_t bits = 0;
            if (n <= hintplan::H1H2_MAX_N) { w = hintplan::h1h2_work(n); bits = hintplan::h1h2_capacity_bits(n); }
            printf("{\"threads\": %d, \"items\": %d, \"chunk\": %d, \"blocks\": %" PRIu64 ", \"totalsPerLane\": %" PRIu64 ", \"capacity\": %" PRIu64
                   ", \"capBits\": %u, \"offTable\": %" PRIu64 ", \"offCnt\": %" PRIu64 ", \"offStart\": %" PRIu64 ", \"offTotals\": %" PRIu64
                   ", \"offMissing\": %" PRIu64 ", \"words\": %" PRIu64 "}\n", hintplan::SCAN_THREADS, hintplan::SCAN_ITEMS, hintplan::SCAN_CHUNK, nb,
                   hintplan::totals_per_lane(nb), w.capacity, bits, w.offTable, w.offCnt, w.offStart, w.offTotals, w.offMissing, w.words);
        } else if (!strcmp(cmd, "home")) {
            uint64_t dim, cap, w[3];
            if (!rd(f, &dim) || !rd(f, &cap) || (dim != 1 && dim != 3) || !cap || (cap & (cap - 1))) return 2;
            for (uint64_t k = 0; k < dim; k++) if (!rd(f, &w[k])) return 2;
            printf("{\"home\": %" PRIu64 ", \"hash\": %" PRIu64 "}\n", hintplan::h1h2_home(w, (uint32_t)dim, cap), hintplan::key_hash(w, (uint32_t)dim));
        } else return 2;
    }
    fclose(f);
    return 0;
}
