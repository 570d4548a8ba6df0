// The host-only planner of the multiplicity sessions (csrc/mult_session_plan.h) in a program of its own, so that
// tests/test_mult_session_cpu.py can run it under the address and undefined-behaviour sanitizers.  Reads commands from the text file named
// on the command line and prints one JSON object per command:
//     lookup nT k elemWords                       {"ok": 0, "why": ".."} or {"ok": 1, "capBits", "capacity", "blocks", "offSlots", "bytes"}
//     range size elemWords path                   {"ok": 0, "why": ".."} or {"ok": 1, "path", "threads", "ldsCounters", "offCounters", "bytes"}
//     grid rows path                              {"blocks": workgroups of a count launch over one side of `rows` rows}
//     sides k nF  then nF times: rows stride col selStride selCol hasSel
//                                                  {"ok": 0 | 1, "why"}   check_add_sides: every side against its own rows (col repeated k times)
//     spans scratch scratchBytes planBytes count  then count times: base bytes
//                                                  {"ok": 0 | 1, "why"}   check_spans: addresses are numbers, never dereferenced
// Exits non-zero when a command cannot be read.
#include <stdio.h>
#include <inttypes.h>
#include <string.h>
#include <vector>
#include "mult_session_plan.h"

using namespace multsessionplan;

static bool rd(FILE *f, uint64_t *v) { return fscanf(f, "%" SCNu64, v) == 1; }
static void verdict(const char *why) {
    if (why) printf("{\"ok\": 0, \"why\": \"%s\"}\n", why);
    else printf("{\"ok\": 1, \"why\": \"\"}\n");
}

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    FILE *f = fopen(argv[1], "r");
    if (!f) return 2;
    char cmd[16];
    while (fscanf(f, "%15s", cmd) == 1) {
        uint64_t a[4];
        const int want = !strcmp(cmd, "lookup") ? 3 : !strcmp(cmd, "range") ? 3 : !strcmp(cmd, "grid") ? 2 : !strcmp(cmd, "sides") ? 2 : !strcmp(cmd, "spans") ? 4 : -1;
        if (want < 0) return 2;
        for (int k = 0; k < want; k++) if (!rd(f, &a[k])) return 2;
        if (!strcmp(cmd, "lookup")) {
            if (const char *why = check_lookup(a[0], a[1], (uint32_t)a[2])) { verdict(why); continue; }
            const LookupPlan p = plan_lookup(a[0]);
            printf("{\"ok\": 1, \"capBits\": %u, \"capacity\": %" PRIu64 ", \"blocks\": %u, \"offSlots\": %" PRIu64 ", \"bytes\": %" PRIu64 "}\n", p.capBits, p.capacity,
                   p.blocks, p.offSlots, p.bytes);
        } else if (!strcmp(cmd, "range")) {
            if (const char *why = check_range(a[0], (uint32_t)a[1], (uint32_t)a[2])) { verdict(why); continue; }
            const RangePlan p = plan_range(a[0], (uint32_t)a[2]);
            printf("{\"ok\": 1, \"path\": %u, \"threads\": %u, \"ldsCounters\": %u, \"offCounters\": %" PRIu64 ", \"bytes\": %" PRIu64 "}\n", p.path, p.threads,
                   p.ldsCounters, p.offCounters, p.bytes);
        } else if (!strcmp(cmd, "grid")) {
            printf("{\"blocks\": %u}\n", count_blocks(a[0], (uint32_t)a[1]));
        } else if (!strcmp(cmd, "sides")) {
            const uint64_t k = a[0], nF = a[1];
            if (k > 16 || nF > 64) return 2;
            std::vector<pil2gl_tuple_side> sides(nF);
            std::vector<uint64_t> rows(nF);
            std::vector<std::vector<uint64_t>> cols(nF);
            for (uint64_t s = 0; s < nF; s++) {
                uint64_t w[6];
                for (uint64_t &x : w) if (!rd(f, &x)) return 2;
                rows[s] = w[0];
                cols[s].assign(k, w[2]);
                sides[s] = pil2gl_tuple_side{ (const uint64_t *)16, w[1], cols[s].data(), w[5] ? (const uint64_t *)32 : nullptr, w[3], w[4] };
            }
            char why[80];
            verdict(check_add_sides(sides.data(), rows.data(), nF, k, why));
        } else {
            if (a[3] > 2 + 2 * MAX_SIDES) return 2;
            Spans all;
            for (uint64_t i = 0; i < a[3]; i++) {
                uint64_t base, bytes;
                if (!rd(f, &base) || !rd(f, &bytes)) return 2;
                all.r[all.count++] = Spans::Span{ (const void *)(uintptr_t)base, bytes };
            }
            char why[128];
            verdict(check_spans(all, (const void *)(uintptr_t)a[0], a[1], a[2], why));
        }
    }
    fclose(f);
    return 0;
}
