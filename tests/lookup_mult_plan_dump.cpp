// The host-only planner of the lookup multiplicities (csrc/lookup_mult_plan.h) in a program of its own, so that
// tests/test_lookup_mult_cpu.py can run it under the address and undefined-behaviour sanitizers.  Reads commands from the text file named
// on the command line and prints one JSON object per command:
//     plan n k nF elemWords                       {"ok": 0, "why": "..."}   or   {"ok": 1, "capacity", "capBits", "blocks", "launches",
//                                                  "offHeader", "offSlots", "bytes"}
//     alias n words mBase mStride mCol rBase rStride k c0 .. ck-1
//                                                  {"ok": 0 | 1, "columns": 0 | 1}   may m = column mCol of (mBase, mStride) lie beside a
//                                                  matrix (rBase, rStride) of which columns c0.. are read; the bases are byte addresses and
//                                                  are never dereferenced; "columns": both strides and all columns pass check_columns
//     buffers dev n words scratch scratchBytes planBytes mBase mStride mCol k nSides, then for each side: base stride sel selStride selCol c0 .. ck-1
//                                                  {"why": "..."}   mult_column_plan.h's check_buffers over the sides as a unit fills them in
//                                                  (sel 0: no selector); "" when nothing is refused; this unit's subjects ("t, every f")
// Exits non-zero when a command cannot be read.
#include <stdio.h>
#include <inttypes.h>
#include <string.h>
#include <vector>
#include "lookup_mult_plan.h"

static bool rd(FILE *f, uint64_t *v) { return fscanf(f, "%" SCNu64, v) == 1; }

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    FILE *f = fopen(argv[1], "r");
    if (!f) return 2;
    char cmd[16];
    while (fscanf(f, "%15s", cmd) == 1) {
        uint64_t a[11];
        const int want = !strcmp(cmd, "plan") ? 4 : !strcmp(cmd, "alias") ? 8 : !strcmp(cmd, "buffers") ? 11 : -1;
        if (want < 0) return 2;
        for (int k = 0; k < want; k++) if (!rd(f, &a[k])) return 2;
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
        if (!strcmp(cmd, "buffers")) {
            const uint64_t k = a[9], nSides = a[10];
            if (k > 16 || nSides > 1 + multcolumn::MAX_SIDES) return 2;
            std::vector<uint64_t> cols(nSides * k);
            std::vector<pil2gl_tuple_side> sides(nSides);                        // Reads points into them
            multcolumn::Reads all;
            for (uint64_t s = 0; s < nSides; s++) {
                uint64_t w[5];
                for (uint64_t &x : w) if (!rd(f, &x)) return 2;
                for (uint64_t j = 0; j < k; j++) if (!rd(f, &cols[s * k + j])) return 2;
                sides[s] = pil2gl_tuple_side{ (const uint64_t *)(uintptr_t)w[0], w[1], cols.data() + s * k, (const uint64_t *)(uintptr_t)w[2], w[3], w[4] };
                all.add(sides[s], k);
            }
            char why[128];
            const char *msg = multcolumn::check_buffers(all, multcolumn::Out{ (uint64_t *)(uintptr_t)a[6], a[7], a[8] }, a[1], (uint32_t)a[2], a[0] != 0,
                                                        (const void *)(uintptr_t)a[3], a[4], a[5], "t, every f", "t, an f", why);
            printf("{\"why\": \"%s\"}\n", msg ? msg : "");
            continue;
        }
        if (const char *why = lookupmultplan::check(a[0], a[1], a[2], (uint32_t)a[3])) { printf("{\"ok\": 0, \"why\": \"%s\"}\n", why); continue; }
        const lookupmultplan::Plan p = lookupmultplan::plan(a[0], a[2]);
        printf("{\"ok\": 1, \"capacity\": %" PRIu64 ", \"capBits\": %u, \"blocks\": %u, \"launches\": %u, \"offHeader\": %" PRIu64 ", \"offSlots\": %" PRIu64
               ", \"bytes\": %" PRIu64 "}\n", p.capacity, p.capBits, p.blocks, p.launches, p.offHeader, p.offSlots, p.bytes);
    }
    fclose(f);
    return 0;
}
