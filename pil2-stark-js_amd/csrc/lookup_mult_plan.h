// Host-only half of the lookup multiplicities (lookup_mult.hip): what the entries refuse, the capacity of the hash table, the launch
// geometry and where the parts of the working buffer lie.  No HIP header: it builds with the
// plain C++ compiler (tests/lookup_mult_plan_dump.cpp runs it under the sanitizers).  The table's capacity is index_table_plan.h's, a
// side's limits, column and span checks tuple_side_plan.h's, the grid smap_plan.h's; the header's first two words, the report, the
// aliasing rule of m and the checks of a call's buffers are mult_column_plan.h's, shared with range_mult_plan.h.
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
#include "mult_column_plan.h"

namespace lookupmultplan {

using smapplan::THREADS;
using multcolumn::HEADER_BYTES;
using multcolumn::MAX_SIDES;
constexpr uint64_t SLOT_BYTES = 8;
// the header's words behind mult_column_plan.h's two
enum : uint32_t { H_PROBE = 2, HEADER_WORDS_USED = 3 };

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

}  // namespace lookupmultplan
