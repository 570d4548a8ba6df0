// The host-only planner of the recursion witness expansion (csrc/wtns_plan.h) in a program of its own, so that
// tests/test_wtns_exec_cpu.py can run it under the address and undefined-behaviour sanitizers.  Reads cases from the text file named on
// the command line -- per case `nWitness nAdds`, then nAdds lines `a b ca cb` -- plans each with exactly sized buffers and prints one JSON
// object per case:
//     {"ok": 1, "nLevels": L, "levelStart": [...], "adds": [a, b, dst, pos, ...], "coefs": [...]}      or      {"ok": 0, "error": "..."}
// Exits non-zero when a case cannot be read or a plan breaks its own invariants.
#include <stdio.h>
#include <inttypes.h>
#include <vector>
#include "wtns_plan.h"

static void list32(const char *name, const std::vector<uint32_t> &v) {
    printf("\"%s\": [", name);
    for (size_t i = 0; i < v.size(); i++) printf("%s%u", i ? ", " : "", v[i]);
    printf("]");
}

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    FILE *f = fopen(argv[1], "r");
    if (!f) return 2;
    uint64_t nWitness, nAdds;
    int rc = 0;
    while (fscanf(f, "%" SCNu64 " %" SCNu64, &nWitness, &nAdds) == 2) {
        std::vector<uint64_t> tab(4 * nAdds);                       // exactly sized: a read past the table is the sanitizer's to find
        for (uint64_t k = 0; k < 4 * nAdds; k++) if (fscanf(f, "%" SCNu64, &tab[k]) != 1) return 2;
        if (const char *m = wtnsplan::check_sizes(nWitness, nAdds)) { printf("{\"ok\": 0, \"error\": \"%s\"}\n", m); continue; }
        std::vector<uint32_t> level;
        uint32_t nLevels = 0;
        char err[200];
        if (!wtnsplan::levels(tab.data(), 4, nAdds, nWitness, level, &nLevels, err, sizeof err)) { printf("{\"ok\": 0, \"error\": \"%s\"}\n", err); continue; }
        std::vector<uint32_t> recs(4 * nAdds), start(nLevels + 1);
        std::vector<uint64_t> coefs(2 * nAdds);
        wtnsplan::emit(tab.data(), 4, nAdds, nWitness, level, nLevels, nAdds ? tab.data() + 2 : nullptr, 4, 1, recs.data(), coefs.data(), start.data());
        if (!wtnsplan::check_level_starts(start.data(), nLevels, nAdds)) { fprintf(stderr, "level starts do not tile the additions\n"); rc = 1; }
        for (uint32_t l = 0; l < nLevels; l++) {
            if (start[l] == start[l + 1]) { fprintf(stderr, "an empty level\n"); rc = 1; }
            for (uint32_t k = start[l]; k < start[l + 1]; k++) {
                if (level[recs[4 * k + 3]] != l) { fprintf(stderr, "a record outside its level\n"); rc = 1; }
                if (k > start[l] && recs[4 * k + 3] <= recs[4 * k - 1]) { fprintf(stderr, "a level out of source order\n"); rc = 1; }
            }
        }
        printf("{\"ok\": 1, \"nLevels\": %u, ", nLevels);
        list32("levelStart", start); printf(", ");
        list32("adds", recs);
        printf(", \"coefs\": [");
        for (size_t i = 0; i < coefs.size(); i++) printf("%s%" PRIu64, i ? ", " : "", coefs[i]);
        printf("], \"blocks\": %u}\n", wtnsplan::blocks(nAdds));
    }
    fclose(f);
    return rc;
}
