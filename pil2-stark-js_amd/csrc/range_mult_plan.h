// Host-only half of the range-check multiplicities (range_mult.hip): what the entries refuse, which of the two count kernels a call takes,
// the launch geometry, where the parts of the working buffer lie, and the range's first element in either field.  No HIP header: it builds
// with the plain C++ compiler (tests/range_mult_plan_dump.cpp runs it under the sanitizers).  The header's two words, the report, the
// aliasing rule of m and the checks of a call's buffers are mult_column_plan.h's, shared with lookup_mult_plan.h; a side's limits, column
// and span checks are tuple_side_plan.h's.
//
// The table is implicit: the range [lo, lo + size) of one column, the counter of a value v is (v - lo) mod p|r.  Nothing is hashed, probed
// or built.  The working buffer, every part on 16 bytes:
//   HEADER_BYTES             the smallest failing (side << 32 | row), the matched rows
//   4 size                   the counters, 32 bits each (nF n <= 2^31)
// Two count kernels:
//   PATH_LDS     size <= LDS_THRESHOLD: a workgroup of LDS_THREADS lanes counts into `size` counters of its own in LDS and adds every
//                non-zero one to the global counters once, at its end.  At most LDS_BLOCKS workgroups, so that the flush stays small.
//   PATH_GLOBAL  larger ranges: lookup_mult's merged add (wave_merge.cuh) on the global counters, smap_plan.h's grid.
#pragma once
#include <stdint.h>
#include "mult_column_plan.h"

namespace rangemultplan {

using smapplan::THREADS;
using multcolumn::HEADER_BYTES;
using multcolumn::MAX_SIDES;
constexpr uint64_t MAX_SIZE = 1ull << 28;
constexpr uint32_t LDS_THREADS = 1024;               // lanes a workgroup of the LDS count kernel
constexpr uint32_t LDS_BLOCKS = 512;                 // its workgroups at most: two a compute unit
constexpr uint32_t LDS_MAX = 8192;                   // counters the LDS count kernel is built for: 32 KB a workgroup
constexpr uint32_t LDS_THRESHOLD = 8192;             // the largest size that takes it (DESIGN.md section 26 has the measurement)
static_assert(LDS_THRESHOLD <= LDS_MAX, "the threshold lies within what the kernel can hold");
enum : uint32_t { PATH_LDS = 0, PATH_GLOBAL = 1, PATH_AUTO = 2 };

struct Plan {
    uint32_t path, threads, blocks, launches, ldsCounters;       // blocks: of a count launch; ldsCounters: 0 on PATH_GLOBAL
    uint64_t offHeader, offCounters, bytes;                      // byte offsets into the working buffer
};

// 0, or a message for PIL2GL_EINVAL.  force: PATH_AUTO, or the path a test or the benchmark asks for
inline const char *check(uint64_t n, uint64_t size, uint64_t nF, uint32_t elemWords, uint32_t force = PATH_AUTO) {
    if (elemWords != 1 && elemWords != 4) return "elemWords is 1 (Goldilocks) or 4 (BN254 Fr)";
    if (nF < 1 || nF > MAX_SIDES) return "nF must be 1 .. 8 sides of f";
    if (n > tupleside::MAX_N) return "n must be at most 2^28 rows";
    if (size < 1 || size > MAX_SIZE) return "size must be 1 .. 2^28 values";
    if (n && size > n) return "the range has more values than m has rows: size > n";
    if (force > PATH_AUTO) return "the path is 0 (LDS), 1 (global) or 2 (the planner's choice)";
    if (force == PATH_LDS && size > LDS_MAX) return "the LDS path holds at most 8192 counters";
    return nullptr;
}

// the arguments have passed check(): init, one count a side of f, write (the report's words are made on the host from the header)
inline Plan plan(uint64_t n, uint64_t size, uint64_t nF, uint32_t force = PATH_AUTO) {
    Plan p{};
    p.path = force != PATH_AUTO ? force : size <= LDS_THRESHOLD ? PATH_LDS : PATH_GLOBAL;
    const bool lds = p.path == PATH_LDS;
    p.threads = lds ? LDS_THREADS : THREADS;
    const uint64_t want = (n + LDS_THREADS - 1) / LDS_THREADS;
    p.blocks = lds ? (uint32_t)(want < LDS_BLOCKS ? (want ? want : 1) : LDS_BLOCKS) : smapplan::blocks(n);
    p.launches = (uint32_t)(2 + nF);
    p.ldsCounters = lds ? (uint32_t)size : 0;
    p.offHeader = 0;
    p.offCounters = HEADER_BYTES;
    p.bytes = n ? (HEADER_BYTES + 4 * size + 15) & ~15ull : 0;
    return p;
}

// 0, or a message: the table's rows [row0, row0 + size) lie within m's n rows; n > 0
inline const char *check_rows(uint64_t n, uint64_t size, uint64_t row0) {
    return row0 > n || size > n - row0 ? "the table's rows end past m: row0 + size > n" : nullptr;
}

// lo as a field element, canonical: lo mod p as one word; lo mod r in normal form as four 64-bit limbs.  |lo| <= 2^63 is below both moduli
constexpr uint64_t GL_P = 0xFFFFFFFF00000001ull;
constexpr uint64_t FR_R[4] = { 0x43e1f593f0000001ull, 0x2833e84879b97091ull, 0xb85045b68181585dull, 0x30644e72e131a029ull };
inline uint64_t lo_mod_p(int64_t lo) { return lo >= 0 ? (uint64_t)lo : GL_P + (uint64_t)lo; }      // p - |lo|, in arithmetic mod 2^64
inline void lo_mod_r(int64_t lo, uint64_t out[4]) {
    if (lo >= 0) { out[0] = (uint64_t)lo; out[1] = out[2] = out[3] = 0; return; }
    const uint64_t mag = 0 - (uint64_t)lo;           // |lo|, 2^63 for INT64_MIN
    out[0] = FR_R[0] - mag;
    uint64_t borrow = FR_R[0] < mag;
    for (int i = 1; i < 4; i++) { out[i] = FR_R[i] - borrow; borrow = borrow && FR_R[i] == 0; }
}

}  // namespace rangemultplan
