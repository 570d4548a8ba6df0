// The host-only planner of the lookup grand sum (csrc/logup_sum_plan.h) in a program of its own, so that tests/test_logup_sum_cpu.py can run
// it under the address and undefined-behaviour sanitizers.  Reads commands from the text file named on the command line and prints one
// JSON object per command:
//     plan n nTerms elemWords                      {"ok": 0, "why": "..."}   or   {"ok": 1, "threads", "items", "blocks", "launches",
//                                                  "depth", "width", "bytes"}
//     alias n words oBase oStride oCol rBase rStride k c0 .. ck-1
//                                                  {"ok": 0 | 1, "columns": 0 | 1}   may out = the word columns oCol .. of (oBase, oStride) lie
//                                                  beside a matrix (rBase, rStride) of which columns c0.. are read; the bases are byte
//                                                  addresses and are never dereferenced; "columns": every column passes check_columns
//     layout                                       {"size", "side", "k", "coef", "busId"}: sizeof and offsetof of pil2gl_logup_term
// Exits non-zero when a command cannot be read.
#include <stdio.h>
#include <stddef.h>
#include <inttypes.h>
#include <string.h>
#include <vector>
#include "logup_sum_plan.h"

static bool rd(FILE *f, uint64_t *v) { return fscanf(f, "%" SCNu64, v) == 1; }

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    FILE *f = fopen(argv[1], "r");
    if (!f) return 2;
    char cmd[16];
    while (fscanf(f, "%15s", cmd) == 1) {
        uint64_t a[8];
        const int want = !strcmp(cmd, "plan") ? 3 : !strcmp(cmd, "alias") ? 8 : !strcmp(cmd, "layout") ? 0 : -1;
        if (want < 0) return 2;
        for (int k = 0; k < want; k++) if (!rd(f, &a[k])) return 2;
        if (!strcmp(cmd, "layout")) {
            printf("{\"size\": %zu, \"side\": %zu, \"k\": %zu, \"coef\": %zu, \"busId\": %zu}\n", sizeof(pil2gl_logup_term), offsetof(pil2gl_logup_term, side),
                   offsetof(pil2gl_logup_term, k), offsetof(pil2gl_logup_term, coef), offsetof(pil2gl_logup_term, busId));
            continue;
        }
        if (!strcmp(cmd, "alias")) {
            if (a[7] > 64 || (a[1] != 1 && a[1] != 4)) return 2;
            std::vector<uint64_t> cols(a[7]);
            for (uint64_t &c : cols) if (!rd(f, &c)) return 2;
            const uint64_t n = a[0], oStride = a[3], oCol = a[4], rStride = a[6];
            const uint32_t width = logupplan::out_width((uint32_t)a[1]);
            const uint64_t oCols[3] = { oCol, oCol + 1, oCol + 2 };
            const bool columns = !tupleside::check_columns(n, oStride, oCols, width) && !tupleside::check_columns(n, rStride, cols.empty() ? nullptr : cols.data(), cols.size());
            const multcolumn::ReadMatrix r{ (const void *)(uintptr_t)a[5], rStride, cols.data(), cols.size() };
            const bool ok = columns && logupplan::out_allowed((const void *)(uintptr_t)a[2], oStride, oCol, width, r, n, (uint32_t)a[1]);
            printf("{\"ok\": %d, \"columns\": %d}\n", ok ? 1 : 0, columns ? 1 : 0);
            continue;
        }
        if (const char *why = logupplan::check(a[0], a[1], (uint32_t)a[2])) { printf("{\"ok\": 0, \"why\": \"%s\"}\n", why); continue; }
        const logupplan::Plan p = logupplan::plan(a[0], (uint32_t)a[2]);
        printf("{\"ok\": 1, \"threads\": %u, \"items\": %u, \"blocks\": %u, \"launches\": %u, \"depth\": %u, \"width\": %u, \"bytes\": %" PRIu64 "}\n", p.threads, p.items,
               p.blocks, p.launches, p.depth, logupplan::out_width((uint32_t)a[2]), p.bytes);
    }
    fclose(f);
    return 0;
}
