// What the host-only planners of the units built on the resident sMap share (wtns_plan.h, conn_plan.h, conn_check_plan.h): the grid of their stride kernels,
// the signal limit, the overlap test of the entries, the 16-byte rule of staged parts and the narrowing of a host sMap into the packed
// 32-bit table the device reads.  No HIP header: it builds with the plain C++ compiler (tests/smap_plan_dump.cpp runs it under the
// sanitizers).  The device half is smap_cells.cuh.
#pragma once
#include <stdint.h>

namespace smapplan {

constexpr uint32_t THREADS = 256;                    // lanes per workgroup of every kernel of wtns_exec.hip and conn_pols.hip
constexpr uint32_t MAX_BLOCKS = 2048;                // a grid sized to the chip (8 workgroups a compute unit); the stride loops take the rest
constexpr uint64_t MAX_SIGNALS = 1ull << 32;         // nW = nWitness + nAdds stays below: the reference's sMap is Uint32Array, the device tables 32-bit

// workgroups of a launch over `items` lanes' worth of work
inline uint32_t blocks(uint64_t items) {
    const uint64_t want = (items + THREADS - 1) / THREADS;
    return (uint32_t)(want < MAX_BLOCKS ? (want ? want : 1) : MAX_BLOCKS);
}

// the byte ranges share a byte; an empty range meets nothing
inline bool meets(const void *a, uint64_t aBytes, const void *b, uint64_t bBytes) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return aBytes && bBytes && x < y + bBytes && y < x + aBytes;
}

// staged parts start on 16 bytes: a length in 64-bit words, rounded up to an even one
inline uint64_t pad16(uint64_t nWords) { return (nWords + 1) & ~1ull; }
// the words a packed table of `cells` 32-bit indices takes as a staged part
inline uint64_t packed_words(uint64_t cells) { return pad16((cells + 1) / 2); }

// A host sMap into the packed table: index (i, j) of nRows x nCols goes to 32-bit position i nCols + j of out (packed_words(nRows nCols)
// words, all written: the padding is zero).  src: rows of u64, row-major (an exec file's section), or with colsU32 nCols arrays of colLen
// u32 one after the other (the setups' sMap).  False at the first entry >= nW, in that order, with its position and value: the whole
// 64-bit value decides, not its low half.
inline bool narrow(const void *src, bool colsU32, uint64_t colLen, uint64_t nRows, uint64_t nCols, uint64_t nW, uint64_t *out, uint64_t *badCell,
                   uint64_t *badValue) {
    const uint64_t cells = nRows * nCols;
    for (uint64_t k = 0; k < packed_words(cells); k++) out[k] = 0;
    for (uint64_t c = 0, i = 0, j = 0; c < cells; c++) {
        const uint64_t v = colsU32 ? ((const uint32_t *)src)[j * colLen + i] : ((const uint64_t *)src)[c];
        if (v >= nW) { *badCell = c; *badValue = v; return false; }
        out[c >> 1] |= v << (32 * (c & 1));          // the low half first, as the device reads the word
        if (++j == nCols) { j = 0; i++; }
    }
    return true;
}

}  // namespace smapplan
