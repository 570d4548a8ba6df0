// Host-only driver for the G1 commit batch's host code, built by tests/test_bn128_commit_cpu.py with the address and undefined-behaviour
// sanitizers: the batch planner's answers (csrc/bn_params.cpp) and, lane by lane, the mapping lane -> (k, i) -> element that the kernels
// run (csrc/bn_msm_batch.h), one JSON document on stdout.
//   usage: bn_msm_batch_dump <batches.txt>      lines of  "plan <K> <count>..."  or
//                                                        "map <rowStride> <K>" followed by K lines "<first> <rows> <m> <slot>..." (slot -1: empty)
#include <stdio.h>
#include <string.h>
#include <string>
#include <vector>
#include "bn_msm_batch.h"
#include "bn_params.h"

int main(int argc, char **argv) {
    if (argc != 2) { fprintf(stderr, "usage: bn_msm_batch_dump <batches.txt>\n"); return 2; }
    FILE *f = fopen(argv[1], "r");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    std::string plans, maps;
    char word[16];
    while (fscanf(f, "%15s", word) == 1) {
        char buf[160];
        if (!strcmp(word, "plan")) {
            unsigned K;
            if (fscanf(f, "%u", &K) != 1 || K < 1 || K > bnm::MSM_MAX_POLYS) { fprintf(stderr, "bad plan line\n"); return 2; }
            std::vector<uint64_t> counts(K);
            for (auto &c : counts) { unsigned long long v; if (fscanf(f, "%llu", &v) != 1) { fprintf(stderr, "bad plan line\n"); return 2; } c = v; }
            const bnp::BnMsmPlan p = bnp::bn_msm_batch_plan(K, counts.data());
            snprintf(buf, sizeof buf, "%s[%u, %u, %u, %u, %llu]", plans.empty() ? "" : ", ", p.c, p.nWindows, p.bucketsPerWindow, p.windowsPerPass,
                     (unsigned long long)p.scratchBytes);
            plans += buf;
        } else if (!strcmp(word, "map")) {
            bnm::MsmBatch B{};
            if (fscanf(f, "%u %u", &B.rowStride, &B.K) != 2 || B.K < 1 || B.K > bnm::MSM_MAX_POLYS) { fprintf(stderr, "bad map line\n"); return 2; }
            unsigned nSlots = 0;
            uint64_t total = 0;
            for (unsigned k = 0; k < B.K; k++) {
                unsigned long long first;
                if (fscanf(f, "%llu %u %u", &first, &B.rows[k], &B.m[k]) != 3 || B.m[k] < 1 || nSlots + B.m[k] > bnm::MSM_MAX_TOTAL_SLOTS) { fprintf(stderr, "bad polynomial\n"); return 2; }
                B.first[k] = first;
                for (unsigned j = 0; j < B.m[k]; j++) {
                    long long s;
                    if (fscanf(f, "%lld", &s) != 1) { fprintf(stderr, "bad slot\n"); return 2; }
                    B.slots[nSlots++] = s < 0 ? bnm::MSM_EMPTY_SLOT : (uint32_t)s;
                }
                total += bnm::msm_batch_count(B, k);
            }
            maps += maps.empty() ? "[" : ", [";
            for (uint64_t lane = 0; lane < total; lane++) {
                uint32_t k = 0, i = 0;
                uint64_t e = 0;
                if (!bnm::msm_batch_locate(B, lane, k, i)) { fprintf(stderr, "lane %llu has no point\n", (unsigned long long)lane); return 1; }
                const bool used = bnm::msm_batch_element(B, k, i, e);
                snprintf(buf, sizeof buf, "%s[%u, %u, %lld]", lane ? ", " : "", k, i, used ? (long long)e : -1ll);
                maps += buf;
            }
            uint32_t k, i;
            if (bnm::msm_batch_locate(B, total, k, i)) { fprintf(stderr, "a lane past the batch has a point\n"); return 1; }
            maps += "]";
        } else { fprintf(stderr, "bad line: %s\n", word); return 2; }
    }
    fclose(f);
    printf("{\"plans\": [%s],\n \"maps\": [%s]}\n", plans.c_str(), maps.c_str());
    return 0;
}
