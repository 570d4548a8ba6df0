// Host-only half of the BN254 Fr grand product, grand sum and batch inverse (bn_scan.hip): the one place that decides the segment length,
// the segments, the levels and the working buffer from n.  No HIP header: it builds with the plain C++ compiler (tests/bn_scan_dump.cpp
// runs it under the sanitizers).  What the entries refuse about a column is bn_column.h's.
//
// Both halves of every operator -- Montgomery's batch inversion and the running product / sum -- are the same shape: a vector of n items
// is cut into S segments of L items, a lane per segment; the S segment totals are the same problem one level up, until a level has at
// most TOP_MAX items, which one lane finishes alone (for the inversion: with the one Fermat ladder of the call).
//   n <= TOP_MAX   one level: S = 1, L = n
//   otherwise      S = min(LANES, ceil(n / SEG_MIN)) segments at most, L = ceil(n / S), S = ceil(n / L) again; the next level has S items
// A level hands at most LANES = 2^17 items up, so the levels above the first are small and their number stops growing at
// n = SEG_MIN^3 * TOP_MAX + 1 = 2^18 + 1: level counts 1..5 first occur at n = 1, 65, 1025, 16385, 262145.
// The working buffer, in elements of 32 bytes: for every level i >= 1 its n_i items (segment totals, inverted / scanned in place) and n_i
// more for the prefixes of its inversion; then, only for an inversion in place, n elements for the prefixes of level 0 (out of place they
// live in the destination).  Above level 0 that is below 2 * (2^17 + 2^13 + 2^9 + 2^5) elements, 8.6 MiB.
#pragma once
#include <stdint.h>

namespace bnscan {

constexpr uint32_t THREADS = 256;
constexpr uint32_t SEG_MIN = 16;                     // a cut level has at most ceil(n / 16) segments (L >= 16 unless LANES binds: then longer)
constexpr uint32_t TOP_MAX = 64;                     // a level this short is one lane's
constexpr uint64_t LANES = 1ull << 17;               // 256 CUs x 4 SIMDs x 64 lanes x 2 waves: segments are cut until there are this many
constexpr uint32_t MAX_LEVELS = 8;                   // 5 are the most the rule yields (2^17 -> 2^13 -> 2^9 -> 32 -> 1 segments)

enum Op : uint32_t { OP_BATCH_INVERSE = 0, OP_GPROD = 1, OP_GSUM = 2, OP_BATCH_INVERSE_IN_PLACE = 3, N_OPS };

struct Level {
    uint64_t n;                                      // items of this level (level 0: the caller's n; after it S of the level before)
    uint32_t L;                                      // items per segment
    uint64_t S;                                      // segments, ceil(n / L); the last level has one
    uint64_t off;                                    // level >= 1: where its n items start in the working buffer, in elements; n prefixes follow
};
struct Plan {
    uint32_t nLevels;
    Level lv[MAX_LEVELS];
    uint64_t q0Off;                                  // the level-0 prefixes of an inversion in place, in elements
    uint64_t elems;                                  // the working buffer, in elements
};

inline Plan plan(uint64_t n, bool inPlace) {
    Plan p{};
    uint64_t cur = n, off = 0;
    for (;;) {
        Level &l = p.lv[p.nLevels];
        l.n = cur;
        if (p.nLevels) { l.off = off; off += 2 * cur; }
        p.nLevels++;
        if (cur <= TOP_MAX || p.nLevels == MAX_LEVELS) {
            l.L = (uint32_t)(cur ? cur : 1); l.S = 1;
            break;
        }
        const uint64_t most = (cur + SEG_MIN - 1) / SEG_MIN, want = LANES < most ? LANES : most;
        l.L = (uint32_t)((cur + want - 1) / want);
        l.S = (cur + l.L - 1) / l.L;
        cur = l.S;
    }
    p.q0Off = off;
    p.elems = off + (inPlace ? n : 0);
    return p;
}

inline uint64_t scratch_bytes(const Plan &p) { return 32 * p.elems; }

}  // namespace bnscan
