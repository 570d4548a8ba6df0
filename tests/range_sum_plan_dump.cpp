// The host-only planner of the range-check grand sum (csrc/range_sum_plan.h) in a program of its own, so that tests/test_range_sum_cpu.py
// can run it under the address and undefined-behaviour sanitizers.  Reads commands from the text file named on the command line and prints
// one JSON object per command:
//     plan n nF nR elemWords                       {"ok": 0, "why": "..."}   or   {"ok": 1, "threads", "items", "blocks", "launches",
//                                                  "depth", "width", "bytes"}
//     call n words oBase oStride oCol mBase mStride mCol lo size row0
//                                                  {"ok": 0 | 1, "why": "..."}   check_call of the resident form with no f term and one range; lo
//                                                  as a two's-complement word; the bases are byte addresses and are never dereferenced
//     c0 lo busId a0 a1 a2 b0 b1 b2                {"c0": [w0, w1, w2]}   alpha field(lo) + busId + beta over Goldilocks, canonical words in
//     words elemWords mStride mCol size row0       {"words": ..}   the 64-bit words of a host m matrix that are staged
//     layout                                       sizeof and offsetof of pil2gl_range_term
// Exits non-zero when a command cannot be read.
#include <stdio.h>
#include <stddef.h>
#include <inttypes.h>
#include <string.h>
#include "range_sum_plan.h"

static bool rd(FILE *f, uint64_t *v) { return fscanf(f, "%" SCNu64, v) == 1; }

static const uint64_t GLP = 0xFFFFFFFF00000001ull;
static uint64_t gl_mul(uint64_t a, uint64_t b) { return (uint64_t)((unsigned __int128)a * b % GLP); }
static uint64_t gl_add(uint64_t a, uint64_t b) { return (uint64_t)(((unsigned __int128)a + b) % GLP); }

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    FILE *f = fopen(argv[1], "r");
    if (!f) return 2;
    char cmd[16];
    while (fscanf(f, "%15s", cmd) == 1) {
        uint64_t a[11];
        const int want = !strcmp(cmd, "plan") ? 4 : !strcmp(cmd, "call") ? 11 : !strcmp(cmd, "c0") ? 8 : !strcmp(cmd, "words") ? 5 : !strcmp(cmd, "layout") ? 0 : -1;
        if (want < 0) return 2;
        for (int k = 0; k < want; k++) if (!rd(f, &a[k])) return 2;
        if (!strcmp(cmd, "layout")) {
            typedef pil2gl_range_term T;
            printf("{\"size\": %zu, \"m\": %zu, \"mStride\": %zu, \"mCol\": %zu, \"lo\": %zu, \"rangeSize\": %zu, \"row0\": %zu, \"coef\": %zu, \"busId\": %zu}\n", sizeof(T),
                   offsetof(T, m), offsetof(T, mStride), offsetof(T, mCol), offsetof(T, lo), offsetof(T, size), offsetof(T, row0), offsetof(T, coef), offsetof(T, busId));
            continue;
        }
        if (!strcmp(cmd, "call")) {
            if (a[1] != 1 && a[1] != 4) return 2;
            pil2gl_range_term r{};
            r.m = (const uint64_t *)(uintptr_t)a[5]; r.mStride = a[6]; r.mCol = a[7]; r.lo = (int64_t)a[8]; r.size = a[9]; r.row0 = a[10];
            const uint64_t ch[4] = { 1, 2, 3, 4 };
            char why[96];
            const char *msg = rangesumplan::check_call(nullptr, 0, &r, 1, ch, ch, (const uint64_t *)(uintptr_t)a[2], a[3], a[4], a[0], (uint32_t)a[1], true, why);
            printf("{\"ok\": %d, \"why\": \"%s\"}\n", msg ? 0 : 1, msg ? msg : "");
            continue;
        }
        if (!strcmp(cmd, "c0")) {
            pil2gl_range_term r{};
            r.lo = (int64_t)a[0]; r.busId[0] = a[1];
            uint64_t c0[3];
            rangesumplan::gl_c0(r, a + 2, a + 5, gl_mul, gl_add, c0);
            printf("{\"c0\": [%" PRIu64 ", %" PRIu64 ", %" PRIu64 "]}\n", c0[0], c0[1], c0[2]);
            continue;
        }
        if (!strcmp(cmd, "words")) {
            pil2gl_range_term r{};
            r.mStride = a[1]; r.mCol = a[2]; r.size = a[3]; r.row0 = a[4];
            printf("{\"words\": %" PRIu64 "}\n", rangesumplan::m_words(r, (uint32_t)a[0]));
            continue;
        }
        if (const char *why = rangesumplan::check(a[0], a[1], a[2], (uint32_t)a[3])) { printf("{\"ok\": 0, \"why\": \"%s\"}\n", why); continue; }
        const rangesumplan::Plan p = rangesumplan::plan(a[0], (uint32_t)a[3]);
        printf("{\"ok\": 1, \"threads\": %u, \"items\": %u, \"blocks\": %u, \"launches\": %u, \"depth\": %u, \"width\": %u, \"bytes\": %" PRIu64 "}\n", p.threads, p.items,
               p.blocks, p.launches, p.depth, logupplan::out_width((uint32_t)a[3]), p.bytes);
    }
    fclose(f);
    return 0;
}
