// The host-only planner of the BN254 Fr plookup hint (csrc/bn_h1h2_plan.h) in a program of its own, so that tests/test_bn128_h1h2_cpu.py
// can run it under the address and undefined-behaviour sanitizers: walks n over 1..2^14 and over 2^k - 1, 2^k, 2^k + 1 up to 2^28, checks
// every plan's invariants and prints one line per plan,
//     n cap scanBlocks expandBlocks scratchBytes
// and the verdicts of the output rule on a few chosen pairs.  Exits non-zero on a broken invariant.
#include <stdio.h>
#include "bn_h1h2_plan.h"
#include "bn_column.h"

static int bad(const char *what, uint64_t n) { fprintf(stderr, "n = %llu: %s\n", (unsigned long long)n, what); return 1; }

static int dump(uint64_t n) {
    const bnh1h2::Plan p = bnh1h2::plan(n);
    if (p.cap & (p.cap - 1)) return bad("the capacity is no power of two", n);
    if (p.cap < 2 * n || (n > 1 && p.cap >= 4 * n) || p.cap < 2 || p.cap - 1 > 0xFFFFFFFFull) return bad("the capacity's range", n);
    if ((uint64_t)p.scanBlocks * bnh1h2::SCAN_CHUNK < n || (uint64_t)(p.scanBlocks - 1) * bnh1h2::SCAN_CHUNK >= n) return bad("scan chunks do not tile the groups", n);
    if ((uint64_t)p.expandBlocks * bnh1h2::EXPAND_ROWS < n || (uint64_t)(p.expandBlocks - 1) * bnh1h2::EXPAND_ROWS >= n) return bad("expand workgroups do not tile the rows", n);
    if ((uint64_t)p.rowBlocks * bnh1h2::THREADS < n || (uint64_t)(p.rowBlocks - 1) * bnh1h2::THREADS >= n) return bad("row workgroups do not tile the rows", n);
    if (p.tableOff != 0 || p.startOff < p.cap || p.totalsOff < p.startOff + n || p.missingOff < p.totalsOff + p.scanBlocks || p.words < p.missingOff + 2)
        return bad("the parts of the working buffer overlap", n);
    if ((p.startOff | p.totalsOff | p.missingOff | p.words) & 3) return bad("a part is not 16-byte aligned", n);
    if (bnh1h2::scratch_bytes(p) >= 20 * n + n / 512 + 64) return bad("the working buffer exceeds its stated bound", n);
    printf("%llu %llu %u %u %llu\n", (unsigned long long)n, (unsigned long long)p.cap, p.scanBlocks, p.expandBlocks,
           (unsigned long long)bnh1h2::scratch_bytes(p));
    return 0;
}

int main() {
    int rc = 0;
    for (uint64_t n = 1; n <= (1u << 14); n++) rc |= dump(n);
    for (uint32_t k = 15; k <= 28; k++)
        for (uint64_t n = (1ull << k) - 1; n <= (1ull << k) + 1 && n <= bncol::MAX_N; n++) rc |= dump(n);
    // an output against another column: 1 when they share no element by the rule (bn_column.h)
    const uintptr_t a = 1 << 20;
    auto apart = [](uintptr_t x, uint64_t xStride, uintptr_t y, uint64_t yStride, uint64_t n) { return bncol::relation(x, xStride, y, yStride, n) == bncol::APART; };
    printf("apart same %d\n", apart(a, 3, a, 3, 100));
    printf("apart same-pointer-other-stride %d\n", apart(a, 3, a, 2, 100));
    printf("apart interleaved %d\n", apart(a, 5, a + 32 * 2, 5, 100));
    printf("apart shifted-rows %d\n", apart(a, 3, a + 32 * 6, 3, 100));
    printf("apart misaligned %d\n", apart(a, 3, a + 8, 3, 100));
    printf("apart disjoint %d\n", apart(a, 3, a + 32 * (99 * 3 + 1), 3, 100));
    printf("apart other-strides %d\n", apart(a, 3, a + 32, 5, 100));
    printf("apart empty %d\n", apart(a, 1, a, 1, 0));
    printf("refusals %d %d %d %d %d\n", bncol::check_size(bncol::MAX_N) == nullptr, bncol::check_size(bncol::MAX_N + 1) != nullptr,
           bncol::check_stride(0) != nullptr, bncol::check_stride(1ull << 32) != nullptr, bncol::check_stride(0xFFFFFFFFull) == nullptr);
    return rc;
}
