// Host-only half of the connection polynomials (conn_pols.hip): what the entries refuse, how many digit passes the sort takes, the launch
// geometry and where every part of the working buffer lies.  No HIP header: it builds with the plain C++ compiler.  What it shares with
// wtns_plan.h (workgroup size, the stride kernels' grid, the signal limit, the sMap's narrowing) is smap_plan.h's.
//
// The working buffer, every part on 16 bytes, cells = nRows nCols, T = nCols 2^loBits + 2^hiBits table elements:
//   16                       the first bad cell (8 bytes used)
//   8 elemWords T            the power tables: hi[t] = w^(t 2^loBits), then lo[j][t] = w^t ks'[j]
//   4 x r16(4 cells)         keys and cells of the two sort buffers; the keys of the buffer the last pass did not write become `pred`
//   1024 sortBlocks          the pass's histogram, [digit][workgroup], sortBlocks = ceil(cells / TILE)
//   r16(4 scanChunks)        its chunk totals, scanChunks = ceil(256 sortBlocks / SCAN_CHUNK)
// which stays below 16 cells + cells / 4 + cells / 16384 + 8 elemWords T + 2048 bytes: 16.26 bytes a cell and the two small tables.
#pragma once
#include <stdint.h>
#include "smap_plan.h"

namespace connplan {

using smapplan::THREADS;                             // lanes per workgroup of every kernel of conn_pols.hip; init, link, tables and fill take smapplan::blocks
constexpr uint32_t WAVES = THREADS / 64;
constexpr uint32_t ROUNDS = 16;                      // 64-cell rounds a wave walks in a sort pass
constexpr uint32_t TILE = THREADS * ROUNDS;          // cells per workgroup of a sort pass: wave v owns cells [v 64 ROUNDS, (v + 1) 64 ROUNDS) of it
constexpr uint32_t BINS = 256;                       // 8-bit digits
static_assert(BINS == THREADS, "lane t of a workgroup owns digit t");
constexpr uint32_t SCAN_ITEMS = 16;                  // histogram entries per lane of the scan
constexpr uint32_t SCAN_CHUNK = THREADS * SCAN_ITEMS;
constexpr uint32_t MAX_COLS = 64;                    // ks' travels as a kernel argument (2 KiB for Fr)
constexpr uint32_t MAX_N_BITS = 32;
constexpr uint64_t MAX_CELLS = 1ull << 32;           // cells stay below, as signals stay below smapplan::MAX_SIGNALS: 32-bit keys, cells and histogram counts

struct Plan {
    uint64_t cells;
    uint32_t passes, nBits, loBits, hiBits, sortBlocks, scanChunks, launches;
    uint64_t tableElems;                             // T
    uint64_t offBad, offHi, offLo, offKeys[2], offCells[2], offHist, offSums, bytes;      // byte offsets into the working buffer
};

inline uint64_t r16(uint64_t bytes) { return (bytes + 15) & ~15ull; }

// 0, or a message for PIL2GL_EINVAL
inline const char *check(uint64_t nRows, uint64_t nCols, uint64_t nW, uint64_t N, uint32_t elemWords) {
    if (elemWords != 1 && elemWords != 4) return "elemWords is 1 (Goldilocks) or 4 (BN254 Fr)";
    if (nCols > MAX_COLS) return "at most 64 columns";
    if (N == 0 || (N & (N - 1)) || N > (1ull << MAX_N_BITS)) return "N must be a power of two, at most 2^32";
    if (nRows > N) return "nRows must not exceed N";
    if (nW >= smapplan::MAX_SIGNALS) return "nW must stay below 2^32";
    if (nCols && nRows >= (MAX_CELLS + nCols - 1) / nCols) return "nRows nCols must stay below 2^32";
    return nullptr;
}

// the arguments have passed check()
inline Plan plan(uint64_t nRows, uint64_t nCols, uint64_t nW, uint64_t N, uint32_t elemWords) {
    Plan p{};
    p.cells = nRows * nCols;
    while ((1ull << p.nBits) < N) p.nBits++;
    p.loBits = (p.nBits + 1) / 2;
    p.hiBits = p.nBits - p.loBits;
    if (p.cells && nW > 1) {                         // keys are below nW: the digits above its highest one are all zero
        uint32_t bits = 0;
        while (bits < 32 && ((nW - 1) >> bits)) bits++;
        p.passes = (bits + 7) / 8;
    }
    p.sortBlocks = (uint32_t)((p.cells + TILE - 1) / TILE);
    p.scanChunks = (uint32_t)(((uint64_t)BINS * p.sortBlocks + SCAN_CHUNK - 1) / SCAN_CHUNK);
    p.tableElems = nCols ? (nCols << p.loBits) + (1ull << p.hiBits) : 0;
    // init, per pass (histogram, chunk totals, their scan, the chunks' scan, scatter), link; tables, fill
    p.launches = (p.cells ? 2 + 5 * p.passes : 0) + (nCols ? 2 : 0);
    uint64_t at = 0;
    p.offBad = at; at += 16;
    p.offHi = at; at += 8ull * elemWords << p.hiBits;
    p.offLo = at; at += nCols ? (8ull * elemWords * nCols) << p.loBits : 0;
    for (int b = 0; b < 2; b++) {
        p.offKeys[b] = at; at += r16(4 * p.cells);
        p.offCells[b] = at; at += r16(4 * p.cells);
    }
    p.offHist = at; at += 4ull * BINS * p.sortBlocks;
    p.offSums = at; at += r16(4ull * p.scanChunks);
    p.bytes = nCols ? at : 0;
    return p;
}

}  // namespace connplan
