// Host-only half of the connection check (conn_check.hip): what the entries refuse, the capacity of the hash table, the launch geometry and
// where every part of the working buffer lies.  No HIP header: it builds with the plain C++ compiler (tests/conn_check_plan_dump.cpp runs
// it under the sanitizers).  The limits are conn_plan.h's, the grid and the overlap test smap_plan.h's, the table's capacity
// index_table_plan.h's.
//
// The table: one 32-bit cell index a slot (a cell stays below 2^32 - 1 = EMPTY), capacity for N nCols cells.
// The working buffer, every part on 16 bytes, cells = N nCols, T = nCols 2^loBits + 2^hiBits table elements:
//   HEADER_BYTES             the report's three words, the longest probe of the build, the check's smallest failing cell, the build's
//                            smallest cell that shares its identity with a smaller one (six u64, the rest unused)
//   4 capacity               the hash table
//   r16(8 elemWords 2^hiBits) + r16(8 elemWords nCols 2^loBits)     the power tables of conn_plan.h: hi[t] = w^(t 2^loBits), then
//                            lo[j][t] = w^t ks'[j]
#pragma once
#include <stdint.h>
#include "conn_plan.h"
#include "index_table_plan.h"

namespace conncheckplan {

using smapplan::THREADS;
constexpr uint64_t HEADER_BYTES = 64;
constexpr uint32_t LAUNCHES = 4;                     // tables, build, check, finish
// the header's words
enum : uint32_t { H_CELL = 0, H_PARTNER = 1, H_KIND = 2, H_PROBE = 3, H_FAIL = 4, H_DUP = 5 };
// the kinds of report[2]
enum : uint64_t { CLEAN = 0, NAMES_NO_CELL = 1, VALUES_DIFFER = 2, IDS_NOT_DISTINCT = 3 };

struct Plan {
    uint64_t cells, capacity;
    uint32_t capBits, nBits, loBits, hiBits, lanesPerCell, buildBlocks, checkBlocks;
    uint64_t tableElems;                             // T
    uint64_t offHeader, offTable, offHi, offLo, bytes;      // byte offsets into the working buffer
};

// 0, or a message for PIL2GL_EINVAL
inline const char *check(uint64_t N, uint64_t nCols, uint32_t elemWords) {
    if (elemWords != 1 && elemWords != 4) return "elemWords is 1 (Goldilocks) or 4 (BN254 Fr)";
    if (nCols > connplan::MAX_COLS) return "at most 64 columns";
    if (N == 0 || (N & (N - 1)) || N > (1ull << connplan::MAX_N_BITS)) return "N must be a power of two, at most 2^32";
    if (nCols && N >= (connplan::MAX_CELLS + nCols - 1) / nCols) return "N nCols must stay below 2^32";
    return nullptr;
}

// a column range of a row-major matrix: nCols adjacent columns from `offset` on, `stride` elements a row
inline const char *check_columns(uint64_t stride, uint64_t offset, uint64_t nCols) {
    return stride >> 32 || offset > stride || stride - offset < nCols ? "stride < offset + nCols (or stride >= 2^32)" : nullptr;
}
// bytes from the matrix's first element to the end of the range's last one
inline uint64_t span_bytes(uint64_t N, uint64_t nCols, uint64_t stride, uint64_t offset, uint32_t elemWords) {
    return N && nCols ? ((N - 1) * stride + offset + nCols) * 8 * elemWords : 0;
}

// the arguments have passed check()
inline Plan plan(uint64_t N, uint64_t nCols, uint32_t elemWords) {
    Plan p{};
    p.cells = N * nCols;
    while ((1ull << p.nBits) < N) p.nBits++;
    p.loBits = (p.nBits + 1) / 2;
    p.hiBits = p.nBits - p.loBits;
    const indextable::Capacity c = indextable::capacity_for(p.cells);
    p.capacity = c.slots; p.capBits = c.bits;
    p.lanesPerCell = elemWords == 4 ? 2 : 1;
    p.buildBlocks = smapplan::blocks(p.cells);
    p.checkBlocks = smapplan::blocks(p.cells * p.lanesPerCell);
    p.tableElems = nCols ? (nCols << p.loBits) + (1ull << p.hiBits) : 0;
    uint64_t at = 0;
    p.offHeader = at; at += HEADER_BYTES;
    p.offTable = at; at += 4 * p.capacity;
    p.offHi = at; at += connplan::r16(8ull * elemWords << p.hiBits);
    p.offLo = at; at += connplan::r16((8ull * elemWords * nCols) << p.loBits);
    p.bytes = nCols ? at : 0;
    return p;
}

}  // namespace conncheckplan
