// Host-only half of the multiplicity column m, what its producers share whatever table they count against (lookup_mult.hip a hash table,
// range_mult.hip an arithmetic progression): the header of the working buffer, the report's four words and how the header becomes them,
// the aliasing rule of m (which logup_sum_plan.h applies to its output column too), and the checks of a call's buffers.  No HIP header:
// it builds with the plain C++ compiler (the *_plan_dump.cpp programs of tests/ run it under the sanitizers).  A side's limits, column and
// span checks are tuple_side_plan.h's, the overlap test smap_plan.h's.  The device half is mult_column.cuh.
// Not here: the reports of tuple_check.hip and conn_check.hip, five words made on the device from two minima.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include "index_table_plan.h"
#include "tuple_side_plan.h"

namespace multcolumn {

using indextable::NONE;                              // "no side, no row" in the report
constexpr uint64_t HEADER_BYTES = 64;                // the working buffer's first part; the unit's own part lies behind it
constexpr uint32_t MAX_SIDES = 8;
constexpr uint32_t REPORT_WORDS = 4;
// the header's words that every unit has: the smallest failing (side << 32 | row), the matched rows
enum : uint32_t { H_FAIL = 0, H_MATCHED = 1 };
// the kinds of report[0]
enum : uint64_t { CLEAN = 0, F_NOT_IN_T = 1 };

// the column written: column col of the matrix (m, stride)
struct Out { uint64_t *m; uint64_t stride, col; };

inline void clean(uint64_t *report) { if (report) { report[0] = CLEAN; report[1] = report[2] = NONE; report[3] = 0; } }

// the report's four words from the header's two
inline void report_of(const uint64_t *h, uint64_t *report) {
    const bool failed = h[H_FAIL] != NONE;
    report[0] = failed ? F_NOT_IN_T : CLEAN;
    report[1] = failed ? h[H_FAIL] >> 32 : NONE;
    report[2] = failed ? h[H_FAIL] & 0xFFFFFFFFull : NONE;
    report[3] = h[H_MATCHED];
}

// one matrix a call reads: its base, its stride, the columns read of it
struct ReadMatrix { const void *base; uint64_t stride; const uint64_t *cols; uint64_t k; };

// the matrices a call reads, filled by the unit: a table's side if it has one, then each side of f, a side's selector behind it when it has
// one (an absent selector is no matrix and meets nothing); at most 2 + 2 MAX_SIDES
struct Reads {
    ReadMatrix r[2 + 2 * MAX_SIDES];
    uint32_t count = 0;
    void add(const pil2gl_tuple_side &s, uint64_t k) {
        r[count++] = ReadMatrix{ s.base, s.stride, s.hostCols, k };
        if (s.sel) r[count++] = ReadMatrix{ s.sel, s.selStride, &s.selCol, 1 };
    }
};

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

// What both forms of an entry refuse about its buffers, n > 0, after the shapes have passed: 0, or the message for PIL2GL_EINVAL (made in
// `why` where it holds a number).  dev: the pointers are the device's -- aligned, and beside a scratch of at least planBytes that meets
// nothing else.  aligned, overlapped: how the unit's messages name what it reads ("t, every f" and "t, an f" where there is a table side).
inline const char *check_buffers(const Reads &all, const Out &out, uint64_t n, uint32_t elemWords, bool dev, const void *scratch, uint64_t scratchBytes,
                                 uint64_t planBytes, const char *aligned, const char *overlapped, char (&why)[128]) {
    using namespace tupleside;
    uintptr_t bits = (uintptr_t)out.m | (uintptr_t)scratch;
    bool null = !out.m || (dev && !scratch);
    for (uint32_t i = 0; i < all.count; i++) { bits |= (uintptr_t)all.r[i].base; null = null || !all.r[i].base; }
    if (null) return "null buffer";
    if (dev && (bits & 15)) { snprintf(why, sizeof why, "%s, the selectors, m and the scratch must be 16-byte aligned", aligned); return why; }
    if (dev) {
        if (scratchBytes < planBytes) {
            snprintf(why, sizeof why, "the scratch holds %llu bytes, %llu needed", (unsigned long long)scratchBytes, (unsigned long long)planBytes);
            return why;
        }
        bool hit = smapplan::meets(scratch, planBytes, out.m, span_bytes(n, out.stride, out.col, elemWords));
        for (uint32_t i = 0; i < all.count; i++)
            hit = hit || smapplan::meets(scratch, planBytes, all.r[i].base, span_bytes(n, all.r[i].stride, top_column(all.r[i].cols, all.r[i].k), elemWords));
        if (hit) { snprintf(why, sizeof why, "the scratch overlaps %s, a selector or m", overlapped); return why; }
    }
    for (uint32_t i = 0; i < all.count; i++)
        if (!m_allowed(out.m, out.stride, out.col, all.r[i], n, elemWords))
            return "m overlaps a matrix that is read: it may only be a column of that matrix (its base, its stride) that is not read";
    return nullptr;
}

}  // namespace multcolumn
