// The host-only planner of the clustered logUp sum (csrc/logup_cluster_plan.h) in a program of its own, so that
// tests/test_logup_cluster_cpu.py can run it under the address and undefined-behaviour sanitizers.  Reads commands from the text file named
// on the command line and prints one JSON object per command:
//     plan n nF nR nIm elemWords                   {"ok": 0, "why": "..."}   or   {"ok": 1, "threads", "items", "blocks", "launches",
//                                                  "depth", "width", "bytes"}
//     call n words tBase tStride oBase oStride oCol nIm (imBase imStride imCol) x nIm
//                                                  {"ok": 0 | 1, "why": "..."}   check_call of the resident form with ONE f term of k = 2, the
//                                                  columns 0 and 1 of (tBase, tStride), in cluster 0, every further cluster id given to a
//                                                  range-less copy of that term; the bases are byte addresses and are never dereferenced
//     apart n words aBase aStride aCol bBase bStride bCol        {"apart": 0 | 1}   outputs_apart
//     groups n words oBase oStride oCol nIm (imBase imStride imCol) x nIm        {"group": [..], "words": [..]}   out_groups
//     layout                                       sizeof and offsetof of pil2gl_logup_im_col
// Exits non-zero when a command cannot be read.
#include <stdio.h>
#include <stddef.h>
#include <inttypes.h>
#include <string.h>
#include "logup_cluster_plan.h"

static bool rd(FILE *f, uint64_t *v) { return fscanf(f, "%" SCNu64, v) == 1; }

static bool rd_im(FILE *f, uint64_t nIm, pil2gl_logup_im_col *im) {
    for (uint64_t c = 0; c < nIm; c++) {
        uint64_t v[3];
        for (int k = 0; k < 3; k++) if (!rd(f, &v[k])) return false;
        im[c].base = (uint64_t *)(uintptr_t)v[0]; im[c].stride = v[1]; im[c].col = v[2];
    }
    return true;
}

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    FILE *f = fopen(argv[1], "r");
    if (!f) return 2;
    char cmd[16];
    while (fscanf(f, "%15s", cmd) == 1) {
        uint64_t a[8];
        const int want = !strcmp(cmd, "plan") ? 5 : !strcmp(cmd, "call") ? 8 : !strcmp(cmd, "apart") ? 8 : !strcmp(cmd, "groups") ? 6 : !strcmp(cmd, "layout") ? 0 : -1;
        if (want < 0) return 2;
        for (int k = 0; k < want; k++) if (!rd(f, &a[k])) return 2;
        if (!strcmp(cmd, "layout")) {
            typedef pil2gl_logup_im_col T;
            printf("{\"size\": %zu, \"base\": %zu, \"stride\": %zu, \"col\": %zu}\n", sizeof(T), offsetof(T, base), offsetof(T, stride), offsetof(T, col));
            continue;
        }
        if (!strcmp(cmd, "call")) {
            const uint64_t nIm = a[7];
            if ((a[1] != 1 && a[1] != 4) || nIm < 1 || nIm > logupclusterplan::MAX_IM) return 2;
            pil2gl_logup_im_col im[logupclusterplan::MAX_IM];
            if (!rd_im(f, nIm, im)) return 2;
            const uint64_t cols[2] = { 0, 1 };
            pil2gl_logup_term t[logupclusterplan::MAX_IM] = {};
            uint64_t cluster[logupclusterplan::MAX_IM];
            for (uint64_t u = 0; u < nIm; u++) {
                t[u].side.base = (const uint64_t *)(uintptr_t)a[2]; t[u].side.stride = a[3]; t[u].side.hostCols = cols; t[u].k = 2;
                cluster[u] = u;
            }
            const uint64_t ch[4] = { 1, 2, 3, 4 };
            char why[96];
            const char *msg = logupclusterplan::check_call(t, nIm, nullptr, 0, cluster, im, nIm, ch, ch, (const uint64_t *)(uintptr_t)a[4], a[5], a[6], a[0],
                                                           (uint32_t)a[1], true, why);
            printf("{\"ok\": %d, \"why\": \"%s\"}\n", msg ? 0 : 1, msg ? msg : "");
            continue;
        }
        if (!strcmp(cmd, "apart")) {
            if (a[1] != 1 && a[1] != 4) return 2;
            printf("{\"apart\": %d}\n", (int)logupclusterplan::outputs_apart((const void *)(uintptr_t)a[2], a[3], a[4], (const void *)(uintptr_t)a[5], a[6], a[7],
                                                                              logupplan::out_width((uint32_t)a[1]), a[0], (uint32_t)a[1]));
            continue;
        }
        if (!strcmp(cmd, "groups")) {
            const uint64_t nIm = a[5];
            if ((a[1] != 1 && a[1] != 4) || nIm < 1 || nIm > logupclusterplan::MAX_IM) return 2;
            pil2gl_logup_im_col im[logupclusterplan::MAX_IM];
            if (!rd_im(f, nIm, im)) return 2;
            const logupclusterplan::OutGroups g = logupclusterplan::out_groups(im, nIm, (const uint64_t *)(uintptr_t)a[2], a[3], a[4], a[0], (uint32_t)a[1]);
            printf("{\"group\": [");
            for (uint64_t o = 0; o <= nIm; o++) printf("%s%u", o ? ", " : "", g.group[o]);
            printf("], \"words\": [");
            for (uint64_t o = 0; o <= nIm; o++) printf("%s%" PRIu64, o ? ", " : "", g.words[o]);
            printf("]}\n");
            continue;
        }
        if (const char *why = logupclusterplan::check(a[0], a[1], a[2], a[3], (uint32_t)a[4])) { printf("{\"ok\": 0, \"why\": \"%s\"}\n", why); continue; }
        const logupclusterplan::Plan p = logupclusterplan::plan(a[0], (uint32_t)a[4]);
        printf("{\"ok\": 1, \"threads\": %u, \"items\": %u, \"blocks\": %u, \"launches\": %u, \"depth\": %u, \"width\": %u, \"bytes\": %" PRIu64 "}\n", p.threads, p.items,
               p.blocks, p.launches, p.depth, logupplan::out_width((uint32_t)a[4]), p.bytes);
    }
    fclose(f);
    return 0;
}
