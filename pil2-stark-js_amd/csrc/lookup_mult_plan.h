// Host-only half of the lookup multiplicities (lookup_mult.hip): what the entries refuse, the capacity of the hash table, the launch
// geometry, where the parts of the working buffer lie, and the aliasing rule of the output column m.  No HIP header: it builds with the
// plain C++ compiler (tests/lookup_mult_plan_dump.cpp runs it under the sanitizers).  The table's capacity is index_table_plan.h's, a
// side's limits, column and span checks tuple_side_plan.h's, the grid and the overlap test smap_plan.h's.
//
// The table: over t's selected rows ONLY (the f sides are counted, not inserted), capacity for n rows.  A slot is 8 bytes: the tuple's
// smallest selected row of t (n <= 2^28 stays far below EMPTY) and beside it the 32-bit counter (nF n <= 2^31).
// The working buffer, every part on 16 bytes:
//   HEADER_BYTES             the smallest failing (side << 32 | row), the matched rows, the longest probe of the build
//   8 capacity               the slots
#pragma once
#include <stdint.h>
#include "index_table_plan.h"
#include "tuple_side_plan.h"

namespace lookupmultplan {

using smapplan::THREADS;
using indextable::NONE;
constexpr uint64_t HEADER_BYTES = 64;
constexpr uint64_t SLOT_BYTES = 8;
constexpr uint32_t MAX_SIDES = 8;
constexpr uint32_t REPORT_WORDS = 4;
// the header's words
enum : uint32_t { H_FAIL = 0, H_MATCHED = 1, H_PROBE = 2, HEADER_WORDS_USED = 3 };
// the kinds of report[0]
enum : uint64_t { CLEAN = 0, F_NOT_IN_T = 1 };

struct Plan {
    uint64_t capacity;
    uint32_t capBits, blocks, launches;              // blocks: of every launch, each a lane per row of one side
    uint64_t offHeader, offSlots, bytes;             // byte offsets into the working buffer
};

// 0, or a message for PIL2GL_EINVAL
inline const char *check(uint64_t n, uint64_t k, uint64_t nF, uint32_t elemWords) {
    if (elemWords != 1 && elemWords != 4) return "elemWords is 1 (Goldilocks) or 4 (BN254 Fr)";
    if (k < 1 || k > tupleside::MAX_K) return "k must be 1 .. 16 columns";
    if (nF < 1 || nF > MAX_SIDES) return "nF must be 1 .. 8 sides of f";
    if (n > tupleside::MAX_N) return "n must be at most 2^28 rows";
    return nullptr;
}

// the arguments have passed check(): init, build, one count a side of f, write (the report's words are made on the host from the header)
inline Plan plan(uint64_t n, uint64_t nF) {
    Plan p{};
    const indextable::Capacity c = indextable::capacity_for(n);
    p.capacity = c.slots; p.capBits = c.bits;
    p.blocks = smapplan::blocks(n);
    p.launches = (uint32_t)(3 + nF);
    p.offHeader = 0;
    p.offSlots = HEADER_BYTES;
    p.bytes = n ? HEADER_BYTES + SLOT_BYTES * p.capacity : 0;
    return p;
}

// one matrix a call reads: its base, its stride, the columns read of it
struct ReadMatrix { const void *base; uint64_t stride; const uint64_t *cols; uint64_t k; };

// The aliasing rule of m, column mCol of (mBase, mStride): its span (from the matrix's first element to the end of row n - 1's element of
// column mCol) may meet the span of a matrix that is read only when it IS that matrix -- the same base and the same stride -- and mCol is
// none of the columns read of it.  The arguments have passed check_columns().
inline bool m_allowed(const void *mBase, uint64_t mStride, uint64_t mCol, const ReadMatrix &r, uint64_t n, uint32_t elemWords) {
    using namespace tupleside;
    if (!smapplan::meets(mBase, span_bytes(n, mStride, mCol, elemWords), r.base, span_bytes(n, r.stride, top_column(r.cols, r.k), elemWords))) return true;
    if (mBase != r.base || mStride != r.stride) return false;
    for (uint64_t j = 0; j < r.k; j++) if (r.cols[j] == mCol) return false;
    return true;
}

}  // namespace lookupmultplan
