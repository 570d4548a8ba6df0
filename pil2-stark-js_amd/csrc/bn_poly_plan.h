// Host-only half of the BN254 Fr polynomial division / evaluation (bn_poly.hip): the one place that decides the segment length, the
// segments per chain, the carry levels and the working buffer from (n, k).  No HIP header: it builds with the plain C++ compiler.
//
// The operation is d[i] = c[i] + beta d[i + k] (d[j] = 0 for j >= n): k independent chains of M = ceil(n / k) links.  A level of the plan
// cuts every chain into S segments of L links, a lane per segment; the S k segment values are the same problem with multiplier beta^L,
// which the next level takes, until a level has a lane per chain (S = 1).
//   lane per chain (S = 1)  when the chains are short (M <= SEG_MIN: a segment would be the whole chain) or there are enough of them to
//                           fill the chip (k >= LANES)
//   segmented               otherwise: S = min(ceil(LANES / k), ceil(M / SEG_MIN)) segments, L = ceil(M / S), S = ceil(M / L) again
// A level of S > 1 hands S k <= LANES + k items to the next, whose chains have S links: every level after the first is small, and the
// number of levels stops growing at n = SEG_MIN * LANES = 2^22 (k = 1).
#pragma once
#include <stdint.h>

namespace bnpoly {

constexpr uint32_t MAX_POINTS = 64;                  // evaluation points per call
constexpr uint32_t THREADS = 256;
constexpr uint32_t SEG_MIN = 32;                     // a chain this short is not cut; a cut one has at most ceil(M / 32) segments (L > 16)
constexpr uint64_t LANES = 1ull << 17;               // 256 CUs x 4 SIMDs x 64 lanes x 2 waves: segments are cut until there are this many
constexpr uint32_t MAX_LEVELS = 8;                   // 5 are the most the rule above yields (2^17 -> 2^12 -> 2^7 -> 4 -> 1 segments)
constexpr uint64_t BETA_ELEMS = (uint64_t)MAX_POINTS * MAX_LEVELS;      // the working buffer starts with the multipliers [point][level]

struct Level {
    uint64_t n;                                      // items of this level (level 0: the caller's n; after it S k of the level before)
    uint64_t M;                                      // links of the longest chain, ceil(n / k)
    uint64_t full;                                   // chains that have M links (the others have M - 1): n - (M - 1) k
    uint32_t L;                                      // links per segment
    uint64_t S;                                      // segments per chain
    uint64_t off;                                    // S > 1: where its S k segment values start, in elements after the multipliers
};
struct Plan {
    uint32_t nLevels;                                // the last one has S = 1; nLevels - 1 carry levels
    Level lv[MAX_LEVELS];
    uint64_t valueElems;                             // segment values of all levels (of one evaluation point)
};

inline Plan plan(uint64_t n, uint64_t k) {
    Plan p{};
    uint64_t cur = n, off = 0;
    const uint64_t smax = (LANES + k - 1) / k;
    for (;;) {
        Level &l = p.lv[p.nLevels++];
        l.n = cur;
        l.M = (cur + k - 1) / k;
        l.full = l.M ? cur - (l.M - 1) * k : 0;
        if (l.M <= SEG_MIN || smax < 2 || p.nLevels == MAX_LEVELS) {
            l.L = (uint32_t)(l.M ? l.M : 1); l.S = 1; l.off = 0;
            break;
        }
        const uint64_t most = (l.M + SEG_MIN - 1) / SEG_MIN, want = smax < most ? smax : most;
        l.L = (uint32_t)((l.M + want - 1) / want);
        l.S = (l.M + l.L - 1) / l.L;
        l.off = off;
        off += l.S * k;
        cur = l.S * k;
    }
    p.valueElems = off;
    return p;
}

// bytes of the working buffer a call needs: the multipliers, then the segment values of every point
inline uint64_t scratch_bytes(const Plan &p, uint32_t nPoints) { return 32 * (BETA_ELEMS + (uint64_t)nPoints * p.valueElems); }

}  // namespace bnpoly
