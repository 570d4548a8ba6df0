// The host-only planner of the grand product (csrc/grand_prod_plan.h) in a program of its own, so that tests/test_grand_prod_cpu.py can run it
// under the address and undefined-behaviour sanitizers.  Reads commands from the text file named on the command line and prints one JSON
// object per command:
//     plan n nTerms sumK elemWords                 {"ok": 0, "why": "..."}   or   {"ok": 1, "threads", "items", "blocks", "launches",
//                                                  "depth", "width", "bytes"}
//     call n words dev nTerms k stride selStride idStride base step oBase oStride oCol
//                                                  {"ok": 0, "why": ".."} or {"ok": 1, "sumK", "jobBytes", "lastStart", "lastCol", "den"}:
//                                                  check_call() on nTerms terms of k columns each -- term u's matrix at byte address base +
//                                                  u step with columns stride - 1, stride - 2, .. (its selector at the same address when
//                                                  selStride > 0, its id column likewise when idStride > 0, each in its last column; den = u
//                                                  mod 2) -- and, when it passes, pack() into the job of the field.  The addresses are never
//                                                  dereferenced.
//     layout                                       sizeof and offsetof of pil2gl_grand_prod_term, and the sizes of the packed terms and jobs
// Exits non-zero when a command cannot be read.
#include <stdio.h>
#include <stddef.h>
#include <inttypes.h>
#include <string.h>
#include <vector>
#include "grand_prod_plan.h"

static bool rd(FILE *f, uint64_t *v) { return fscanf(f, "%" SCNu64, v) == 1; }

template <uint32_t W, uint32_t POWERS>
static void pack_and_print(const pil2gl_grand_prod_term *terms, uint32_t nTerms, uint64_t n, uint64_t sumK) {
    grandprodplan::Job<W, POWERS> J{};
    uint64_t pw[POWERS][W], ch[W];
    for (uint32_t e = 0; e < POWERS; e++) for (uint32_t w = 0; w < W; w++) pw[e][w] = 100 * e + w;
    for (uint32_t w = 0; w < W; w++) ch[w] = 7 + w;
    grandprodplan::pack<W, POWERS>(terms, nTerms, pw, ch, ch, n, J);
    const grandprodplan::Term<W> &L = J.t[nTerms - 1];
    printf("{\"ok\": 1, \"sumK\": %" PRIu64 ", \"jobBytes\": %zu, \"lastStart\": %u, \"lastCol\": %u, \"den\": %u}\n", sumK, sizeof J, (unsigned)L.start,
           J.cols[L.start + L.k - 1], (unsigned)L.den);
}

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    FILE *f = fopen(argv[1], "r");
    if (!f) return 2;
    char cmd[16];
    while (fscanf(f, "%15s", cmd) == 1) {
        uint64_t a[13];
        const int want = !strcmp(cmd, "plan") ? 4 : !strcmp(cmd, "call") ? 13 : !strcmp(cmd, "layout") ? 0 : -1;
        if (want < 0) return 2;
        for (int k = 0; k < want; k++) if (!rd(f, &a[k])) return 2;
        if (!strcmp(cmd, "layout")) {
            typedef pil2gl_grand_prod_term T;
            printf("{\"size\": %zu, \"side\": %zu, \"k\": %zu, \"den\": %zu, \"id\": %zu, \"idStride\": %zu, \"idCol\": %zu, \"idCoef\": %zu, \"glTerm\": %zu, \"frTerm\": %zu, "
                   "\"glJob\": %zu, \"frJob\": %zu}\n", sizeof(T), offsetof(T, side), offsetof(T, k), offsetof(T, den), offsetof(T, id), offsetof(T, idStride), offsetof(T, idCol),
                   offsetof(T, idCoef), sizeof(grandprodplan::Term<3>), sizeof(grandprodplan::Term<4>), sizeof(grandprodplan::GlJob), sizeof(grandprodplan::FrJob));
            continue;
        }
        if (!strcmp(cmd, "call")) {
            const uint64_t n = a[0], nTerms = a[3], k = a[4], stride = a[5], selStride = a[6], idStride = a[7], base = a[8], step = a[9];
            const uint32_t words = (uint32_t)a[1];
            if (nTerms > 64 || k > 64 || (words != 1 && words != 4)) return 2;
            std::vector<uint64_t> cols(k ? k : 1);
            for (uint64_t j = 0; j < k; j++) cols[j] = stride - 1 - j;             // wraps for stride <= j: a column past the stride, refused
            std::vector<pil2gl_grand_prod_term> terms(nTerms ? nTerms : 1);
            for (uint64_t u = 0; u < nTerms; u++) {
                pil2gl_grand_prod_term &t = terms[u];
                memset(&t, 0, sizeof t);
                const uint64_t *m = (const uint64_t *)(uintptr_t)(base + u * step);
                t.side = pil2gl_tuple_side{ m, stride, cols.data(), selStride ? m : nullptr, selStride, selStride ? selStride - 1 : 0 };
                t.k = k; t.den = u % 2;
                if (idStride) { t.id = m; t.idStride = idStride; t.idCol = idStride - 1; }
                t.idCoef[0] = 5; t.idCoef[1] = 6; t.idCoef[2] = 7; t.idCoef[3] = 8;
            }
            const uint64_t ch[4] = { 1, 2, 3, 4 };
            char why[96];
            const char *msg = grandprodplan::check_call(terms.data(), nTerms, ch, ch, ch, (const uint64_t *)(uintptr_t)a[10], a[11], a[12], n, words, a[2] != 0, why);
            if (msg) { printf("{\"ok\": 0, \"why\": \"%s\"}\n", msg); continue; }
            if (words == 1) pack_and_print<3, tupleside::MAX_K - 1>(terms.data(), (uint32_t)nTerms, n, nTerms * k);
            else pack_and_print<4, 1>(terms.data(), (uint32_t)nTerms, n, nTerms * k);
            continue;
        }
        if (const char *why = grandprodplan::check(a[0], a[1], a[2], (uint32_t)a[3])) { printf("{\"ok\": 0, \"why\": \"%s\"}\n", why); continue; }
        const grandprodplan::Plan p = grandprodplan::plan(a[0], (uint32_t)a[3]);
        printf("{\"ok\": 1, \"threads\": %u, \"items\": %u, \"blocks\": %u, \"launches\": %u, \"depth\": %u, \"width\": %u, \"bytes\": %" PRIu64 "}\n", p.threads, p.items,
               p.blocks, p.launches, p.depth, grandprodplan::out_width((uint32_t)a[3]), p.bytes);
    }
    fclose(f);
    return 0;
}
