// Host-only half of the Goldilocks stage-2 hints (hints.hip): the geometry of the three-kernel scan of the running product / sum, the
// capacity of h1h2's hash table, the hash of a key as ONE function for host and device, so that a test can ask where a key lands
// (pil2gl_debug_h1h2_home), and where the parts of h1h2's working buffer lie.  No HIP header: it builds with the plain C++ compiler
// (tests/hint_plan_dump.cpp runs it under the sanitizers).
//
// The scan: a lane takes SCAN_ITEMS consecutive rows, a workgroup of SCAN_THREADS lanes SCAN_CHUNK rows; pass 1 leaves one total a block,
// pass 2 is ONE workgroup whose lane l walks the totals_per_lane(nb) block totals from l totals_per_lane(nb) on (lanes whose run starts at
// or past nb walk nothing), pass 3 adds a block's prefix to its rows.  h1h2's scan of the group starts has the same pass 1 and pass 3.
// The table of h1h2: open addressing, linear probing over t's n rows, one 64-bit row index a slot (EMPTY = 2^64 - 1), capacity the
// smallest power of two >= 2 n and >= 2: the load factor never exceeds 1 / 2.
// The working buffer of h1h2, in 64-bit words:  table[capacity] | cnt[n] | start[n] | totals[blocks(n)] | missing[1]
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define HINT_HD __host__ __device__
#else
#define HINT_HD
#endif

namespace hintplan {

constexpr int SCAN_THREADS = 256, SCAN_ITEMS = 8, SCAN_CHUNK = SCAN_THREADS * SCAN_ITEMS;
constexpr uint64_t H1H2_MAX_N = 1ull << 30;
constexpr uint64_t NONE = ~0ull;

// blocks of pass 1 (and of h1h2's scan of the starts); no n + SCAN_CHUNK - 1, which wraps for n near 2^64 and would let such a call pass
// the entries' grid check
inline uint64_t blocks(uint64_t n) { return n / SCAN_CHUNK + (n % SCAN_CHUNK ? 1 : 0); }
// block totals a lane of pass 2 walks
HINT_HD inline uint64_t totals_per_lane(uint64_t nb) { return (nb + SCAN_THREADS - 1) / SCAN_THREADS; }

// n <= H1H2_MAX_N
inline uint64_t h1h2_capacity(uint64_t n) {
    uint64_t cap = 2;
    while (cap < 2 * n) cap <<= 1;
    return cap;
}
inline uint32_t h1h2_capacity_bits(uint64_t n) {
    uint32_t bits = 0;
    while ((1ull << bits) < h1h2_capacity(n)) bits++;
    return bits;
}

// the hash of a key of dim canonical 64-bit words
HINT_HD inline uint64_t key_hash(const uint64_t *w, uint32_t dim) {
    uint64_t h = 0x9E3779B97F4A7C15ull;
    for (uint32_t k = 0; k < dim; k++) { h ^= w[k] + 0x9E3779B97F4A7C15ull + (h << 6) + (h >> 2); h *= 0xBF58476D1CE4E5B9ull; h ^= h >> 31; }
    return h;
}
// the home slot of a key; capacity a power of two
inline uint64_t h1h2_home(const uint64_t *w, uint32_t dim, uint64_t capacity) { return key_hash(w, dim) & (capacity - 1); }

// word offsets into h1h2's working buffer
struct H1H2Work { uint64_t capacity, offTable, offCnt, offStart, offTotals, offMissing, words; };
inline H1H2Work h1h2_work(uint64_t n) {
    H1H2Work w{};
    w.capacity = h1h2_capacity(n);
    w.offTable = 0;
    w.offCnt = w.capacity;
    w.offStart = w.offCnt + n;
    w.offTotals = w.offStart + n;
    w.offMissing = w.offTotals + blocks(n);
    w.words = w.offMissing + 1;
    return w;
}

}  // namespace hintplan
