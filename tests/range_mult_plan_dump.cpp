// The host-only planner of the range-check multiplicities (csrc/range_mult_plan.h) in a program of its own, so that
// tests/test_range_mult_cpu.py can run it under the address and undefined-behaviour sanitizers.  Reads commands from the text file named
// on the command line and prints one JSON object per command:
//     plan n size nF elemWords path               {"ok": 0, "why": "..."}   or   {"ok": 1, "path", "threads", "blocks", "launches",
//                                                  "ldsCounters", "offHeader", "offCounters", "bytes"}
//     rows n size row0                            {"ok": 0 | 1}   do the table's rows [row0, row0 + size) lie within n rows
//     lo L                                        {"p": lo mod p, "r": [four 64-bit limbs of lo mod r]}   L a signed 64-bit integer
//     alias n words mBase mStride mCol rBase rStride k c0 .. ck-1
//                                                  {"ok": 0 | 1, "columns": 0 | 1}   mult_column_plan.h's m_allowed, as this unit calls it
// Exits non-zero when a command cannot be read.
#include <stdio.h>
#include <inttypes.h>
#include <string.h>
#include <vector>
#include "range_mult_plan.h"

static bool rd(FILE *f, uint64_t *v) { return fscanf(f, "%" SCNu64, v) == 1; }

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    FILE *f = fopen(argv[1], "r");
    if (!f) return 2;
    char cmd[16];
    while (fscanf(f, "%15s", cmd) == 1) {
        if (!strcmp(cmd, "lo")) {
            int64_t lo;
            if (fscanf(f, "%" SCNd64, &lo) != 1) return 2;
            uint64_t r[4];
            rangemultplan::lo_mod_r(lo, r);
            printf("{\"p\": %" PRIu64 ", \"r\": [%" PRIu64 ", %" PRIu64 ", %" PRIu64 ", %" PRIu64 "]}\n", rangemultplan::lo_mod_p(lo), r[0], r[1], r[2], r[3]);
            continue;
        }
        uint64_t a[8];
        const int want = !strcmp(cmd, "plan") ? 5 : !strcmp(cmd, "rows") ? 3 : !strcmp(cmd, "alias") ? 8 : -1;
        if (want < 0) return 2;
        for (int k = 0; k < want; k++) if (!rd(f, &a[k])) return 2;
        if (!strcmp(cmd, "rows")) { printf("{\"ok\": %d}\n", rangemultplan::check_rows(a[0], a[1], a[2]) ? 0 : 1); continue; }
        if (!strcmp(cmd, "alias")) {
            if (a[7] > 64) return 2;
            std::vector<uint64_t> cols(a[7]);
            for (uint64_t &c : cols) if (!rd(f, &c)) return 2;
            const uint64_t n = a[0], mStride = a[3], mCol = a[4], rStride = a[6];
            const bool columns = !tupleside::check_columns(n, mStride, &mCol, 1) && !tupleside::check_columns(n, rStride, cols.empty() ? nullptr : cols.data(), cols.size());
            const multcolumn::ReadMatrix r{ (const void *)(uintptr_t)a[5], rStride, cols.data(), cols.size() };
            const bool ok = columns && multcolumn::m_allowed((const void *)(uintptr_t)a[2], mStride, mCol, r, n, (uint32_t)a[1]);
            printf("{\"ok\": %d, \"columns\": %d}\n", ok ? 1 : 0, columns ? 1 : 0);
            continue;
        }
        if (const char *why = rangemultplan::check(a[0], a[1], a[2], (uint32_t)a[3], (uint32_t)a[4])) { printf("{\"ok\": 0, \"why\": \"%s\"}\n", why); continue; }
        const rangemultplan::Plan p = rangemultplan::plan(a[0], a[1], a[2], (uint32_t)a[4]);
        printf("{\"ok\": 1, \"path\": %u, \"threads\": %u, \"blocks\": %u, \"launches\": %u, \"ldsCounters\": %u, \"offHeader\": %" PRIu64 ", \"offCounters\": %" PRIu64
               ", \"bytes\": %" PRIu64 "}\n", p.path, p.threads, p.blocks, p.launches, p.ldsCounters, p.offHeader, p.offCounters, p.bytes);
    }
    fclose(f);
    return 0;
}
