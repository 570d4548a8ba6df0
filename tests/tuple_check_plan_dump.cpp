// The host-only planner of the lookup and permutation checks (csrc/tuple_check_plan.h) in a program of its own, so that
// tests/test_tuple_check_cpu.py can run it under the address and undefined-behaviour sanitizers.  Reads commands from the text file named
// on the command line and prints one JSON object per command:
//     plan n k elemWords mode           {"ok": 0, "why": "..."}   or   {"ok": 1, "rows", "capacity", "capBits", "blocks", "offHeader",
//                                        "offSlots", "offMinF", "offCounts", "bytes"}
//     columns n stride k c0 .. ck-1     {"ok": 0 | 1}     (k = 0 with no column passes a null list)
//     span n stride top words           {"bytes": n}
//     home k elemWords capacity w ...   {"home": slot}    (k elemWords words follow)
// Exits non-zero when a command cannot be read.
#include <stdio.h>
#include <inttypes.h>
#include <string.h>
#include <vector>
#include "tuple_check_plan.h"

static bool rd(FILE *f, uint64_t *v) { return fscanf(f, "%" SCNu64, v) == 1; }

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    FILE *f = fopen(argv[1], "r");
    if (!f) return 2;
    char cmd[16];
    while (fscanf(f, "%15s", cmd) == 1) {
        uint64_t a[4];
        const int want = !strcmp(cmd, "plan") ? 4 : !strcmp(cmd, "columns") ? 3 : !strcmp(cmd, "span") ? 4 : !strcmp(cmd, "home") ? 3 : -1;
        if (want < 0) return 2;
        for (int k = 0; k < want; k++) if (!rd(f, &a[k])) return 2;
        if (!strcmp(cmd, "columns")) {
            if (a[2] > 64) return 2;
            std::vector<uint64_t> cols(a[2]);
            for (uint64_t &c : cols) if (!rd(f, &c)) return 2;
            printf("{\"ok\": %d}\n", tupleside::check_columns(a[0], a[1], cols.empty() ? nullptr : cols.data(), a[2]) ? 0 : 1);
            continue;
        }
        if (!strcmp(cmd, "span")) { printf("{\"bytes\": %" PRIu64 "}\n", tupleside::span_bytes(a[0], a[1], a[2], (uint32_t)a[3])); continue; }
        if (!strcmp(cmd, "home")) {
            if (a[0] > tupleside::MAX_K || a[1] > 4) return 2;
            std::vector<uint64_t> words(a[0] * a[1]);
            for (uint64_t &w : words) if (!rd(f, &w)) return 2;
            printf("{\"home\": %" PRIu64 "}\n", indextable::home(words.data(), a[0], (uint32_t)a[1], a[2]));
            continue;
        }
        if (const char *why = tuplecheckplan::check(a[0], a[1], (uint32_t)a[2], (uint32_t)a[3])) { printf("{\"ok\": 0, \"why\": \"%s\"}\n", why); continue; }
        const tuplecheckplan::Plan p = tuplecheckplan::plan(a[0]);
        printf("{\"ok\": 1, \"rows\": %" PRIu64 ", \"capacity\": %" PRIu64 ", \"capBits\": %u, \"blocks\": %u, \"offHeader\": %" PRIu64
               ", \"offSlots\": %" PRIu64 ", \"offMinF\": %" PRIu64 ", \"offCounts\": %" PRIu64 ", \"bytes\": %" PRIu64 "}\n",
               p.rows, p.capacity, p.capBits, p.blocks, p.offHeader, p.offSlots, p.offMinF, p.offCounts, p.bytes);
    }
    fclose(f);
    return 0;
}
