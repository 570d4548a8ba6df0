// Host-only half of the lookup and permutation checks (tuple_check.hip): what the entries refuse, the launch geometry and where every part
// of the working buffer lies.  No HIP header: it builds with the plain C++ compiler (tests/tuple_check_plan_dump.cpp runs it under the
// sanitizers).  The table's capacity and hash are index_table_plan.h's, a side's limits and checks tuple_side_plan.h's, the grid smap_plan.h's.
//
// The table: one over BOTH sides' selected rows, a 32-bit row index a slot (t row i as i, f row i as n + i; 2 n <= 2^29 stays far below
// EMPTY), capacity for the 2 n rows that can be inserted.
// The working buffer, every part on 16 bytes:
//   HEADER_BYTES             the report's five words, the longest probe of the build, the judge's smallest failing row of f and of t
//   4 capacity               the slots
//   4 capacity               beside each slot the smallest selected row of f that holds the slot's tuple (EMPTY: none)
//   8 capacity               beside each slot the counter: cntT in the low half, cntF in the high half
#pragma once
#include <stdint.h>
#include "index_table_plan.h"
#include "tuple_side_plan.h"

namespace tuplecheckplan {

using smapplan::THREADS;
using indextable::NONE;
constexpr uint64_t HEADER_BYTES = 64;
constexpr uint32_t LAUNCHES = 3;                     // build, judge, finish
constexpr uint32_t REPORT_WORDS = 5;
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
    if (k < 1 || k > tupleside::MAX_K) return "k must be 1 .. 16 columns";
    if (n > tupleside::MAX_N) return "n must be at most 2^28 rows";
    return nullptr;
}

// the arguments have passed check()
inline Plan plan(uint64_t n) {
    Plan p{};
    p.rows = 2 * n;
    const indextable::Capacity c = indextable::capacity_for(p.rows);
    p.capacity = c.slots; p.capBits = c.bits;
    p.blocks = smapplan::blocks(p.rows);
    uint64_t at = 0;
    p.offHeader = at; at += HEADER_BYTES;
    p.offSlots = at; at += 4 * p.capacity;
    p.offMinF = at; at += 4 * p.capacity;
    p.offCounts = at; at += 8 * p.capacity;
    p.bytes = n ? at : 0;
    return p;
}

}  // namespace tuplecheckplan
