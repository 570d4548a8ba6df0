// The host-only planner of the plookup argument (csrc/plookup_plan.h) in a program of its own, so that tests/test_plookup_cpu.py can run it
// under the address and undefined-behaviour sanitizers.  Reads commands from the text file named on the command line and prints one JSON
// object per command:
//     plan n kF kT elemWords                       {"ok": 0, "why": "..."}   or   {"ok": 1, "threads", "items", "blocks", "launches",
//                                                  "depth", "width", "bytes"}
//     call prod n words dev kF kT hDim stride selStride hStride base step oBase oStride oCol oCol2
//                                                  {"ok": 0, "why": ".."} or {"ok": 1, "jobBytes", "kF", "kT", "lastColF", "lastColT", "selColT",
//                                                  "h2Col", "hDim"}: check_call() of the product (prod = 1) or of the fold (prod = 0) -- f's
//                                                  matrix at byte address base with its columns stride - 1, stride - 2, .., t's at base +
//                                                  step with columns 0, 1, .., both of `stride`; selF at base + 2 step and selT at base + 3
//                                                  step when selStride > 0, each in its last column; h1 and h2 columns 0 and hWidth of the
//                                                  matrix (base + 4 step, hStride); the product's out = (oBase, oStride, oCol), the fold's
//                                                  outF that and outT = (oBase, oStride, oCol2) -- and, when it passes, pack() into the job
//                                                  of the field.  The addresses are never dereferenced.
//     layout                                       the sizes of the packed side, the packed column and the two jobs
// Exits non-zero when a command cannot be read.
#include <stdio.h>
#include <stddef.h>
#include <inttypes.h>
#include <string.h>
#include <vector>
#include "plookup_plan.h"

static bool rd(FILE *f, uint64_t *v) { return fscanf(f, "%" SCNu64, v) == 1; }

// the words of an h element as the job says them: the Fr job has no such field, its kernels know one element
template <uint32_t W, uint32_t POWERS> static uint32_t hdim_of(const plookupplan::Job<W, POWERS, true> &J) { return J.hDim; }
template <uint32_t W, uint32_t POWERS> static uint32_t hdim_of(const plookupplan::Job<W, POWERS, false> &) { return 1; }

template <uint32_t W, uint32_t POWERS, bool HOST>
static void pack_and_print(const pil2gl_tuple_side &f, uint64_t kF, const pil2gl_tuple_side &t, uint64_t kT, const plookupplan::Column *h, uint32_t hDim, uint64_t n) {
    plookupplan::Job<W, POWERS, HOST> J{};
    uint64_t pw[POWERS][W], ch[W];
    for (uint32_t e = 0; e < POWERS; e++) for (uint32_t w = 0; w < W; w++) pw[e][w] = 100 * e + w;
    for (uint32_t w = 0; w < W; w++) ch[w] = 7 + w;
    plookupplan::pack<W, POWERS, HOST>(f, kF, t, kT, h, h ? h + 1 : nullptr, hDim, pw, ch, ch, ch, ch, ch, n, J);
    printf("{\"ok\": 1, \"jobBytes\": %zu, \"kF\": %u, \"kT\": %u, \"lastColF\": %u, \"lastColT\": %u, \"selColT\": %u, \"h2Col\": %u, \"hDim\": %u}\n", sizeof J, J.f.k, J.t.k,
           J.f.cols[J.f.k - 1], J.t.cols[J.t.k - 1], J.t.selCol, J.h2.col, hdim_of(J));
}

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    FILE *f = fopen(argv[1], "r");
    if (!f) return 2;
    char cmd[16];
    while (fscanf(f, "%15s", cmd) == 1) {
        uint64_t a[16];
        const int want = !strcmp(cmd, "plan") ? 4 : !strcmp(cmd, "call") ? 16 : !strcmp(cmd, "layout") ? 0 : -1;
        if (want < 0) return 2;
        for (int k = 0; k < want; k++) if (!rd(f, &a[k])) return 2;
        if (!strcmp(cmd, "layout")) {
            printf("{\"side\": %zu, \"column\": %zu, \"glJob\": %zu, \"frJob\": %zu}\n", sizeof(plookupplan::Side), sizeof(plookupplan::HCol), sizeof(plookupplan::GlJob),
                   sizeof(plookupplan::FrJob));
            continue;
        }
        if (!strcmp(cmd, "call")) {
            const bool prod = a[0] != 0;
            const uint64_t n = a[1], kF = a[4], kT = a[5], stride = a[7], selStride = a[8], hStride = a[9], base = a[10], step = a[11];
            const uint32_t words = (uint32_t)a[2], hDim = (uint32_t)a[6];
            if (kF > 64 || kT > 64 || (words != 1 && words != 4)) return 2;
            std::vector<uint64_t> colsF(kF ? kF : 1), colsT(kT ? kT : 1);
            for (uint64_t j = 0; j < kF; j++) colsF[j] = stride - 1 - j;           // wraps for stride <= j: a column past the stride, refused
            for (uint64_t j = 0; j < kT; j++) colsT[j] = j;
            auto at = [&](uint64_t i) { return base ? (const uint64_t *)(uintptr_t)(base + i * step) : nullptr; };
            const pil2gl_tuple_side sf{ at(0), stride, colsF.data(), selStride ? at(2) : nullptr, selStride, selStride ? selStride - 1 : 0 };
            const pil2gl_tuple_side st{ at(1), stride, colsT.data(), selStride ? at(3) : nullptr, selStride, selStride ? selStride - 1 : 0 };
            const uint32_t hWidth = words == 1 ? hDim : 1;
            const plookupplan::Column h[2] = { { at(4), hStride, 0 }, { at(4), hStride, hWidth } };
            const plookupplan::Column out[2] = { { (const uint64_t *)(uintptr_t)a[12], a[13], a[14] }, { (const uint64_t *)(uintptr_t)a[12], a[13], a[15] } };
            const uint64_t c[4] = { 1, 2, 3, 4 };
            const uint64_t *const ch[4] = { c, c, c, c };
            char why[96];
            const char *msg = plookupplan::check_call(&sf, kF, &st, kT, prod ? h : nullptr, prod ? 2 : 0, hDim, ch, prod ? 4 : 2, out, prod ? 1 : 2, n, words, a[3] != 0, why);
            if (msg) { printf("{\"ok\": 0, \"why\": \"%s\"}\n", msg); continue; }
            if (words == 1) pack_and_print<3, tupleside::MAX_K - 1, true>(sf, kF, st, kT, prod ? h : nullptr, hDim, n);
            else pack_and_print<4, 1, false>(sf, kF, st, kT, prod ? h : nullptr, hDim, n);
            continue;
        }
        if (const char *why = plookupplan::check(a[0], a[1], a[2], (uint32_t)a[3])) { printf("{\"ok\": 0, \"why\": \"%s\"}\n", why); continue; }
        const plookupplan::Plan p = plookupplan::plan(a[0], (uint32_t)a[3]);
        printf("{\"ok\": 1, \"threads\": %u, \"items\": %u, \"blocks\": %u, \"launches\": %u, \"depth\": %u, \"width\": %u, \"bytes\": %" PRIu64 "}\n", p.threads, p.items,
               p.blocks, p.launches, p.depth, plookupplan::out_width((uint32_t)a[3]), p.bytes);
    }
    fclose(f);
    return 0;
}
