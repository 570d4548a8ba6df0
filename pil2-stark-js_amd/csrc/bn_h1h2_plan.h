// Host-only half of the BN254 Fr plookup hint (bn_h1h2.hip): the one place that decides the table capacity, the launches' geometry and
// the layout of the working buffer from n.  No HIP header: it builds with the plain C++ compiler (tests/bn_h1h2_dump.cpp runs it under
// the sanitizers).  What the entries refuse about a column is bn_column.h's.
//
// The working buffer, in 32-bit words, every part starting on a multiple of 4 words (16 bytes):
//   table    cap slots, cap the power of two with 2 n <= cap < 4 n (n = 1: 2): an index into t, or EMPTY
//   start    n words: the counts cnt[i], turned in place into the group starts relative to their scan chunk
//   totals   ceil(n / SCAN_CHUNK) words: the chunks' totals, turned in place into the chunks' first positions
//   missing  one 64-bit cell: the lowest j whose f[j] is not in t, or UINT64_MAX
// A position of the merged sequence is below 2 n <= 2^29 and an index below n <= 2^28, so every one of them is a 32-bit word.
// Bytes: 4 cap + 4 n + 4 ceil(n / 2048) + 16, each part rounded up to 16: below 20 n + n / 512 + 64 for every n, and 3 GiB + 512 KiB + 16
// bytes at n = 2^28 (cap = 2 n there: the table 2 GiB, the starts 1 GiB) -- the 8-byte slots, counts and starts of the Goldilocks form
// would take 8 GiB.
#pragma once
#include <stdint.h>

namespace bnh1h2 {

constexpr uint32_t EMPTY = 0xFFFFFFFFu;
constexpr uint32_t THREADS = 256;
constexpr uint32_t SCAN_ITEMS = 8;                   // groups per lane of the local scan
constexpr uint32_t SCAN_CHUNK_BITS = 11;
constexpr uint32_t SCAN_CHUNK = 1u << SCAN_CHUNK_BITS;       // groups per workgroup of the local scan: THREADS * SCAN_ITEMS
constexpr uint32_t EXPAND_ROWS = 512;                // output rows per workgroup of the expand step: two a lane, 1024 positions
static_assert(SCAN_CHUNK == THREADS * SCAN_ITEMS, "a lane scans SCAN_ITEMS groups");
static_assert(EXPAND_ROWS == 2 * THREADS, "a lane expands two rows");

struct Plan {
    uint64_t cap;                                    // table slots
    uint32_t scanBlocks, expandBlocks, rowBlocks;    // workgroups of the local scan, of the expand step, of insert / count (a lane per row)
    uint64_t tableOff, startOff, totalsOff, missingOff, words;      // in 32-bit words
};

inline uint64_t up4(uint64_t w) { return (w + 3) & ~3ull; }

inline Plan plan(uint64_t n) {
    Plan p{};
    p.cap = 2;
    while (p.cap < 2 * n) p.cap <<= 1;
    p.scanBlocks = (uint32_t)((n + SCAN_CHUNK - 1) / SCAN_CHUNK);
    p.expandBlocks = (uint32_t)((n + EXPAND_ROWS - 1) / EXPAND_ROWS);
    p.rowBlocks = (uint32_t)((n + THREADS - 1) / THREADS);
    p.tableOff = 0;
    p.startOff = up4(p.cap);
    p.totalsOff = p.startOff + up4(n);
    p.missingOff = p.totalsOff + up4(p.scanBlocks);
    p.words = p.missingOff + 4;
    return p;
}

inline uint64_t scratch_bytes(const Plan &p) { return 4 * p.words; }

}  // namespace bnh1h2
