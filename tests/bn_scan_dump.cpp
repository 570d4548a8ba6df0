// The host-only planner of the BN254 Fr grand product / grand sum / batch inverse (csrc/bn_scan_plan.h) in a program of its own, so that
// tests/test_bn128_hints_cpu.py can run it under the address and undefined-behaviour sanitizers: walks n over 1..2^14 and over
// 2^k - 1, 2^k, 2^k + 1 up to 2^28, checks every plan's invariants and prints one line per plan,
//     n inPlace nLevels L S scratchBytes | n_1 L_1 S_1 off_1 | ...
// and the verdicts of the column relation on a few chosen pairs.  Exits non-zero on a broken invariant.
#include <stdio.h>
#include "bn_scan_plan.h"
#include "bn_column.h"

static int bad(const char *what, uint64_t n) { fprintf(stderr, "n = %llu: %s\n", (unsigned long long)n, what); return 1; }

static int dump(uint64_t n, bool inPlace) {
    const bnscan::Plan p = bnscan::plan(n, inPlace);
    if (p.nLevels < 1 || p.nLevels > bnscan::MAX_LEVELS) return bad("level count", n);
    uint64_t cur = n, off = 0;
    for (uint32_t i = 0; i < p.nLevels; i++) {
        const bnscan::Level &l = p.lv[i];
        if (l.n != cur) return bad("a level's items are not the segments of the level below", n);
        if (l.L < 1 || l.S < 1 || (uint64_t)l.L * l.S < l.n || (l.S - 1) * l.L >= l.n) return bad("segments do not tile the items", n);
        if (l.S > bnscan::LANES) return bad("more segments than lanes", n);
        if (i) { if (l.off != off) return bad("offset", n); off += 2 * l.n; }
        if ((i + 1 == p.nLevels) != (l.S == 1 && l.n <= bnscan::TOP_MAX)) return bad("the last level, and only it, is one lane's", n);
        cur = l.S;
    }
    if (p.q0Off != off || p.elems != off + (inPlace ? n : 0)) return bad("working buffer", n);
    printf("%llu %d %u %u %llu %llu", (unsigned long long)n, inPlace ? 1 : 0, p.nLevels, p.lv[0].L, (unsigned long long)p.lv[0].S,
           (unsigned long long)bnscan::scratch_bytes(p));
    for (uint32_t i = 1; i < p.nLevels; i++)
        printf(" | %llu %u %llu %llu", (unsigned long long)p.lv[i].n, p.lv[i].L, (unsigned long long)p.lv[i].S, (unsigned long long)p.lv[i].off);
    printf("\n");
    return 0;
}

int main() {
    int rc = 0;
    for (uint64_t n = 1; n <= (1u << 14); n++) rc |= dump(n, false);
    for (uint32_t k = 1; k <= 28; k++)
        for (uint64_t n = (1ull << k) - 1; n <= (1ull << k) + 1 && n <= bncol::MAX_N; n++) { rc |= dump(n, false); rc |= dump(n, true); }
    // the column relation (bn_column.h): 0 apart, 1 same, 2 overlap
    const uintptr_t a = 1 << 20;
    printf("relation same %d\n", bncol::relation(a, 3, a, 3, 100));
    printf("relation same-pointer-other-stride %d\n", bncol::relation(a, 3, a, 2, 100));
    printf("relation interleaved %d\n", bncol::relation(a, 3, a + 32, 3, 100));
    printf("relation interleaved-later-row %d\n", bncol::relation(a, 3, a + 32 * 7, 3, 100));
    printf("relation shifted-rows %d\n", bncol::relation(a, 3, a + 32 * 6, 3, 100));
    printf("relation misaligned %d\n", bncol::relation(a, 3, a + 8, 3, 100));
    printf("relation apart %d\n", bncol::relation(a, 3, a + 32 * (99 * 3 + 1), 3, 100));
    printf("relation touching %d\n", bncol::relation(a, 3, a + 32 * (99 * 3 + 1) - 8, 3, 100));
    printf("relation other-strides %d\n", bncol::relation(a, 3, a + 32, 5, 100));
    printf("relation empty %d\n", bncol::relation(a, 1, a, 2, 0));
    printf("refusals %d %d %d %d %d\n", bncol::check_size(bncol::MAX_N) == nullptr, bncol::check_size(bncol::MAX_N + 1) != nullptr,
           bncol::check_stride(0) != nullptr, bncol::check_stride(1ull << 32) != nullptr, bncol::check_stride(0xFFFFFFFFull) == nullptr);
    return rc;
}
