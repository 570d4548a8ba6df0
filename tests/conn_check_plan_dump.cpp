// The host-only planner of the connection check (csrc/conn_check_plan.h) in a program of its own, so that tests/test_conn_check_cpu.py
// can run it under the address and undefined-behaviour sanitizers.  Reads commands from the text file named on the command line and
// prints one JSON object per command:
//     plan N nCols elemWords            {"ok": 0, "why": "..."}   or   {"ok": 1, "cells", "capacity", "capBits", "loBits", "hiBits",
//                                        "lanesPerCell", "buildBlocks", "checkBlocks", "tableElems", "offHeader", "offTable", "offHi", "offLo", "bytes"}
//     columns stride offset nCols       {"ok": 0 | 1}
//     span N nCols stride offset words  {"bytes": n}
// Exits non-zero when a command cannot be read.
#include <stdio.h>
#include <inttypes.h>
#include <string.h>
#include "conn_check_plan.h"

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    FILE *f = fopen(argv[1], "r");
    if (!f) return 2;
    char cmd[16];
    while (fscanf(f, "%15s", cmd) == 1) {
        uint64_t a[5];
        const int want = !strcmp(cmd, "plan") ? 3 : !strcmp(cmd, "columns") ? 3 : !strcmp(cmd, "span") ? 5 : -1;
        if (want < 0) return 2;
        for (int k = 0; k < want; k++) if (fscanf(f, "%" SCNu64, &a[k]) != 1) return 2;
        if (!strcmp(cmd, "columns")) { printf("{\"ok\": %d}\n", conncheckplan::check_columns(a[0], a[1], a[2]) ? 0 : 1); continue; }
        if (!strcmp(cmd, "span")) { printf("{\"bytes\": %" PRIu64 "}\n", conncheckplan::span_bytes(a[0], a[1], a[2], a[3], (uint32_t)a[4])); continue; }
        if (const char *why = conncheckplan::check(a[0], a[1], (uint32_t)a[2])) { printf("{\"ok\": 0, \"why\": \"%s\"}\n", why); continue; }
        const conncheckplan::Plan p = conncheckplan::plan(a[0], a[1], (uint32_t)a[2]);
        printf("{\"ok\": 1, \"cells\": %" PRIu64 ", \"capacity\": %" PRIu64 ", \"capBits\": %u, \"loBits\": %u, \"hiBits\": %u, \"lanesPerCell\": %u, "
               "\"buildBlocks\": %u, \"checkBlocks\": %u, \"tableElems\": %" PRIu64 ", \"offHeader\": %" PRIu64 ", \"offTable\": %" PRIu64
               ", \"offHi\": %" PRIu64 ", \"offLo\": %" PRIu64 ", \"bytes\": %" PRIu64 "}\n",
               p.cells, p.capacity, p.capBits, p.loBits, p.hiBits, p.lanesPerCell, p.buildBlocks, p.checkBlocks, p.tableElems, p.offHeader, p.offTable,
               p.offHi, p.offLo, p.bytes);
    }
    fclose(f);
    return 0;
}
