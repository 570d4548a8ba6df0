// The host-only header the sMap units' planners share (csrc/smap_plan.h) in a program of its own, so that tests/test_wtns_exec_cpu.py
// can run it under the address and undefined-behaviour sanitizers.  Reads commands from the text file named on the command line and
// prints one JSON object per command:
//     consts                                          {"threads": T, "maxBlocks": B}
//     blocks ITEMS                                    {"blocks": n}
//     meets aOffset aBytes bOffset bBytes             {"meets": 0 | 1}      two ranges of one 64-byte buffer
//     narrow colsU32 colLen nRows nCols nW v v v ...  {"ok": 1, "words": [...]}      or      {"ok": 0, "cell": c, "value": v}
// narrow's values are the source as it lies in memory: nRows nCols of them (u64 rows), or with colsU32 nCols colLen (u32 columns).  Source
// and packed table are exactly sized: an access past either is the sanitizer's to find.  Exits non-zero when a command cannot be read.
#include <stdio.h>
#include <inttypes.h>
#include <string.h>
#include <vector>
#include "smap_plan.h"

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    FILE *f = fopen(argv[1], "r");
    if (!f) return 2;
    char cmd[16];
    static char buf[64];
    while (fscanf(f, "%15s", cmd) == 1) {
        uint64_t a[5];
        const int want = !strcmp(cmd, "consts") ? 0 : !strcmp(cmd, "blocks") ? 1 : !strcmp(cmd, "meets") ? 4 : !strcmp(cmd, "narrow") ? 5 : -1;
        if (want < 0) return 2;
        for (int k = 0; k < want; k++) if (fscanf(f, "%" SCNu64, &a[k]) != 1) return 2;
        if (want == 0) printf("{\"threads\": %u, \"maxBlocks\": %u}\n", smapplan::THREADS, smapplan::MAX_BLOCKS);
        if (want == 1) printf("{\"blocks\": %u}\n", smapplan::blocks(a[0]));
        if (want == 4) printf("{\"meets\": %d}\n", (int)smapplan::meets(buf + a[0], a[1], buf + a[2], a[3]));
        if (want != 5) continue;
        const bool colsU32 = a[0] != 0;
        const uint64_t colLen = a[1], nRows = a[2], nCols = a[3], nW = a[4], count = colsU32 ? nCols * colLen : nRows * nCols;
        std::vector<uint64_t> src64(colsU32 ? 0 : count);
        std::vector<uint32_t> src32(colsU32 ? count : 0);
        for (uint64_t k = 0; k < count; k++) {
            uint64_t v;
            if (fscanf(f, "%" SCNu64, &v) != 1) return 2;
            if (colsU32) src32[k] = (uint32_t)v; else src64[k] = v;
        }
        std::vector<uint64_t> out(smapplan::packed_words(nRows * nCols), ~0ull);      // every word must be written
        uint64_t cell = 0, value = 0;
        if (!smapplan::narrow(colsU32 ? (const void *)src32.data() : (const void *)src64.data(), colsU32, colLen, nRows, nCols, nW, out.data(), &cell, &value)) {
            printf("{\"ok\": 0, \"cell\": %" PRIu64 ", \"value\": %" PRIu64 "}\n", cell, value);
            continue;
        }
        printf("{\"ok\": 1, \"words\": [");
        for (size_t k = 0; k < out.size(); k++) printf("%s%" PRIu64, k ? ", " : "", out[k]);
        printf("]}\n");
    }
    fclose(f);
    return 0;
}
