// Host-only half of the lookup and permutation checks (tuple_check.hip): what the entries refuse, the capacity of the hash table, the
// launch geometry, where every part of the working buffer lies, and the hash of a tuple as ONE function for host and device, so that a
// test can ask where a tuple lands (pil2gl_debug_tuple_home).  No HIP header: it builds with the plain C++ compiler
// (tests/tuple_check_plan_dump.cpp runs it under the sanitizers).  The grid and the overlap test are smap_plan.h's.
//
// The table: open addressing, linear probing over BOTH sides' selected rows, one 32-bit row index a slot (t row i as i, f row i as n + i,
// EMPTY = 2^32 - 1; 2 n <= 2^29 stays far below), capacity the smallest power of two >= 4 n = twice the 2 n rows that can be inserted and
// >= MIN_CAPACITY: the load factor never exceeds 1 / 2, whatever the data and the selectors.
// The working buffer, every part on 16 bytes:
//   HEADER_BYTES             the report's five words, the longest probe of the build, the judge's smallest failing row of f and of t
//   4 capacity               the slots
//   4 capacity               beside each slot the smallest selected row of f that holds the slot's tuple (EMPTY: none)
//   8 capacity               beside each slot the counter: cntT in the low half, cntF in the high half
#pragma once
#include <stdint.h>
#include "smap_plan.h"

#ifdef __HIPCC__
#define TUPLE_HD __host__ __device__
#else
#define TUPLE_HD
#endif

namespace tuplecheckplan {

using smapplan::THREADS;
constexpr uint64_t HEADER_BYTES = 64;
constexpr uint64_t MIN_CAPACITY = 16;
constexpr uint64_t MAX_N = 1ull << 28;
constexpr uint32_t MAX_K = 16;
constexpr uint32_t LAUNCHES = 3;                     // build, judge, finish
constexpr uint32_t REPORT_WORDS = 5;
constexpr uint64_t NONE = ~0ull;
// the header's words: the report first, as the caller gets it
enum : uint32_t { H_KIND = 0, H_ROW = 1, H_PARTNER = 2, H_CNT_F = 3, H_CNT_T = 4, H_PROBE = 5, H_FAIL_F = 6, H_FAIL_T = 7 };
enum : uint32_t { MODE_LOOKUP = 0, MODE_PERMUTATION = 1 };
// the kinds of report[0]
enum : uint64_t { CLEAN = 0, F_NOT_IN_T = 1, F_MORE_THAN_T = 2, T_MORE_THAN_F = 3 };

struct Plan {
    uint64_t rows, capacity;                         // rows = 2 n, the most the table can be asked to hold
    uint32_t capBits, blocks;
    uint64_t offHeader, offSlots, offMinF, offCounts, bytes;        // byte offsets into the working buffer
};

// 0, or a message for PIL2GL_EINVAL
inline const char *check(uint64_t n, uint64_t k, uint32_t elemWords, uint32_t mode) {
    if (elemWords != 1 && elemWords != 4) return "elemWords is 1 (Goldilocks) or 4 (BN254 Fr)";
    if (mode != MODE_LOOKUP && mode != MODE_PERMUTATION) return "mode is 0 (lookup) or 1 (permutation)";
    if (k < 1 || k > MAX_K) return "k must be 1 .. 16 columns";
    if (n > MAX_N) return "n must be at most 2^28 rows";
    return nullptr;
}

// the k columns of a tuple inside n <= MAX_N rows of `stride` elements; cols may be in any order and may repeat.  n stride <= 2^58 elements
// keeps span_bytes below 2^63 over either field
inline const char *check_columns(uint64_t n, uint64_t stride, const uint64_t *cols, uint64_t k) {
    if (stride >> 32) return "stride >= 2^32";
    if (n * stride > 1ull << 58) return "n stride above 2^58 elements";
    if (!cols) return "null cols";
    for (uint64_t j = 0; j < k; j++) if (cols[j] >= stride) return "a column >= stride";
    return nullptr;
}
// bytes from the matrix's first element to the end of the last one touched: n rows, highest column `top`
inline uint64_t span_bytes(uint64_t n, uint64_t stride, uint64_t top, uint32_t elemWords) {
    return n ? ((n - 1) * stride + top + 1) * 8 * elemWords : 0;
}
inline uint64_t top_column(const uint64_t *cols, uint64_t k) {
    uint64_t top = 0;
    for (uint64_t j = 0; j < k; j++) top = cols[j] > top ? cols[j] : top;
    return top;
}

// the arguments have passed check()
inline Plan plan(uint64_t n) {
    Plan p{};
    p.rows = 2 * n;
    p.capacity = MIN_CAPACITY;
    while (p.capacity < 2 * p.rows) p.capacity <<= 1;
    while ((1ull << p.capBits) < p.capacity) p.capBits++;
    p.blocks = smapplan::blocks(p.rows);
    uint64_t at = 0;
    p.offHeader = at; at += HEADER_BYTES;
    p.offSlots = at; at += 4 * p.capacity;
    p.offMinF = at; at += 4 * p.capacity;
    p.offCounts = at; at += 8 * p.capacity;
    p.bytes = n ? at : 0;
    return p;
}

// ---- the hash of a tuple: bn_h1h2.hip's mixing over the canonical elements' 32-bit limbs, low limb first, column after column (xor a
// limb, multiply, shift; murmur3's finaliser; 32-bit multiplies only).  Two lanes of it give 64 bits; the table has at most 2^30 slots.
struct TupleHash {
    uint32_t h = 0x9E3779B9u, g = 0x7F4A7C15u;
    TUPLE_HD inline void absorb(uint32_t w) {
        h = (h ^ w) * 0x85EBCA6Bu; h ^= h >> 15;
        g = (g ^ w) * 0xC2B2AE35u; g ^= g >> 13;
    }
    TUPLE_HD inline uint64_t finish() const {
        uint32_t a = h * 0xC2B2AE35u, b = g * 0x85EBCA6Bu;
        a ^= a >> 16; b ^= b >> 16;
        return ((uint64_t)b << 32) | a;
    }
};

// the home slot of a tuple given as k elemWords canonical 64-bit words; capacity a power of two
inline uint64_t home(const uint64_t *words, uint64_t k, uint32_t elemWords, uint64_t capacity) {
    TupleHash x;
    for (uint64_t i = 0; i < k * elemWords; i++) { x.absorb((uint32_t)words[i]); x.absorb((uint32_t)(words[i] >> 32)); }
    return x.finish() & (capacity - 1);
}

}  // namespace tuplecheckplan
