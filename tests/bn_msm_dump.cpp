// Host-only driver for the G1 MSM's host code, built by tests/test_bn128_msm_cpu.py with the address and undefined-behaviour sanitizers:
// prints the Fq constants the kernels compile in (csrc/bn_fq_consts.h), the planner's answer for the sizes named on the command line
// (csrc/bn_params.cpp) and the signed digits of the scalars read from a file (csrc/bn_msm_recode.h), one JSON document on stdout.
//   usage: bn_msm_dump <scalars.txt> <n> [<n> ...]        scalars.txt: lines of "<c> <scalar as 64 hex digits, most significant first>"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include "bn_fq_consts.h"
#include "bn_msm_recode.h"
#include "bn_params.h"

static std::string hex(const bnq::Limbs &a) {
    char buf[80];
    std::string s;
    for (int i = 7; i >= 0; i--) { snprintf(buf, sizeof buf, "%08x", a.v[i]); s += buf; }
    return s;
}

int main(int argc, char **argv) {
    if (argc < 2) { fprintf(stderr, "usage: bn_msm_dump <scalars.txt> <n>...\n"); return 2; }
    printf("{\"q\": \"%s\", \"R\": \"%s\", \"R2\": \"%s\", \"R3\": \"%s\", \"n0inv\": %u,\n", hex(bnq::FQ_Q).c_str(), hex(bnq::FQ_R).c_str(),
           hex(bnq::FQ_R2).c_str(), hex(bnq::FQ_3R).c_str(), bnq::FQ_N0INV);
    printf(" \"plans\": {");
    for (int i = 2; i < argc; i++) {
        const unsigned long long n = strtoull(argv[i], nullptr, 10);
        const bnp::BnMsmPlan p = bnp::bn_msm_plan(n);
        printf("%s\"%llu\": [%u, %u, %u, %u, %llu]", i > 2 ? ", " : "", n, p.c, p.nWindows, p.bucketsPerWindow, p.windowsPerPass, (unsigned long long)p.scratchBytes);
    }
    printf("},\n \"digits\": [");
    FILE *f = fopen(argv[1], "r");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    unsigned c;
    char word[80];
    bool first = true;
    while (fscanf(f, "%u %79s", &c, word) == 2) {
        if (strlen(word) != 64 || c < bnm::MSM_MIN_C || c > bnm::MSM_MAX_C) { fprintf(stderr, "bad line\n"); fclose(f); return 2; }
        uint32_t s[8], carry = 0;
        for (int i = 0; i < 8; i++) { char part[9]; memcpy(part, word + 8 * (7 - i), 8); part[8] = 0; s[i] = (uint32_t)strtoul(part, nullptr, 16); }
        const unsigned nW = (bnm::MSM_SCALAR_BITS + 1 + c - 1) / c;
        std::vector<int32_t> d(nW);
        for (unsigned w = 0; w < nW; w++) d[w] = bnm::msm_next_digit(s, carry, c);
        printf("%s[", first ? "" : ", ");
        for (unsigned w = 0; w < nW; w++) printf("%s%d", w ? ", " : "", d[w]);
        printf("]");
        first = false;
    }
    fclose(f);
    printf("]}\n");
    return 0;
}
