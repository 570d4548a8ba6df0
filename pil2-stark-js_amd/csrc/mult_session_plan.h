// Host-only half of the multiplicity sessions (mult_session.hip): a table's multiplicity column m counted over MANY calls -- open makes the
// table, add counts f sides of their own row counts, write writes m -- with the counters in the caller's working buffer between the calls.
// Here: what the entries refuse, the launch geometry, where the parts of the working buffer lie, and the checks of a call's buffers with a
// row count PER matrix (mult_column_plan.h's check_buffers has one n for all).  No HIP header: it builds with the plain C++ compiler
// (tests/mult_session_plan_dump.cpp runs it under the sanitizers).  A side's limits, column and span checks are tuple_side_plan.h's, the
// table's capacity index_table_plan.h's, the range's paths, threshold and lo range_mult_plan.h's, the report and the aliasing rule of m
// mult_column_plan.h's.
//
// The working buffer, every part on 16 bytes:
//   HEADER_BYTES             [0] the smallest failing (side << 32 | row) of the LAST add, [1] its matched rows, [3] the matched rows of
//                            every add before it.  An add starts by one lane moving [1] into [3] and clearing [0] and [1]; the session's
//                            total is [3] + [1].
//   lookup: 16 capacity      the slots: the tuple's smallest selected row of t (32 bits), 32 bits unused, the 64-bit counter
//   range:  8 size           the counters, 64 bits each, rounded up to 16 bytes
// Counters are 64 bits: a session has no bound on the rows it counts.  A count launch's grid comes from the rows of ITS side.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include "index_table_plan.h"
#include "tuple_side_plan.h"
#include "mult_column_plan.h"
#include "range_mult_plan.h"

namespace multsessionplan {

using smapplan::THREADS;
using multcolumn::HEADER_BYTES;
using multcolumn::MAX_SIDES;
using multcolumn::Out;
using multcolumn::ReadMatrix;
using rangemultplan::PATH_LDS;
using rangemultplan::PATH_GLOBAL;
using rangemultplan::PATH_AUTO;
using rangemultplan::LDS_THREADS;
using rangemultplan::LDS_BLOCKS;
constexpr uint64_t SLOT_BYTES = 16;                  // a row and a 64-bit counter in one slot: SLOT_WORDS 32-bit words, the counter at COUNTER_WORD
constexpr uint32_t SLOT_WORDS = 4, COUNTER_WORD = 2;
constexpr uint64_t COUNTER_BYTES = 8;
// the header's word behind mult_column_plan.h's two (word 2 is lookup_mult's probe figure; a session keeps none)
enum : uint32_t { H_TOTAL = 3, HEADER_WORDS_USED = 4 };
// launches of open, of an add with one side (every further side with rows is one more) and of write, as outInfo[3] packs them
constexpr uint32_t LOOKUP_LAUNCHES = 2 | 2 << 8 | 1 << 16;      // init, build; begin, count; write
constexpr uint32_t RANGE_LAUNCHES = 1 | 2 << 8 | 1 << 16;       // init; begin, count; write

struct LookupPlan {
    uint64_t capacity;
    uint32_t capBits, blocks;                        // blocks: of the build and of the write, a lane a row of t; a count launch takes count_blocks() of ITS side
    uint64_t offHeader, offSlots, bytes;
};
struct RangePlan {
    uint32_t path, threads, ldsCounters;
    uint64_t offHeader, offCounters, bytes;
};

inline const char *check_field(uint32_t elemWords) { return elemWords != 1 && elemWords != 4 ? "elemWords is 1 (Goldilocks) or 4 (BN254 Fr)" : nullptr; }

// 0, or a message for PIL2GL_EINVAL
inline const char *check_lookup(uint64_t nT, uint64_t k, uint32_t elemWords) {
    if (const char *m = check_field(elemWords)) return m;
    if (k < 1 || k > tupleside::MAX_K) return "k must be 1 .. 16 columns";
    if (nT > tupleside::MAX_N) return "nT must be at most 2^28 rows";
    return nullptr;
}
inline const char *check_range(uint64_t size, uint32_t elemWords, uint32_t force = PATH_AUTO) {
    if (const char *m = check_field(elemWords)) return m;
    if (size < 1 || size > rangemultplan::MAX_SIZE) return "size must be 1 .. 2^28 values";
    if (force > PATH_AUTO) return "the path is 0 (LDS), 1 (global) or 2 (the planner's choice)";
    if (force == PATH_LDS && size > rangemultplan::LDS_MAX) return "the LDS path holds at most 8192 counters";
    return nullptr;
}

inline LookupPlan plan_lookup(uint64_t nT) {
    LookupPlan p{};
    const indextable::Capacity c = indextable::capacity_for(nT);
    p.capacity = c.slots; p.capBits = c.bits;
    p.blocks = smapplan::blocks(nT);
    p.offHeader = 0;
    p.offSlots = HEADER_BYTES;
    p.bytes = nT ? HEADER_BYTES + SLOT_BYTES * p.capacity : 0;
    return p;
}
inline RangePlan plan_range(uint64_t size, uint32_t force = PATH_AUTO) {
    RangePlan p{};
    p.path = force != PATH_AUTO ? force : size <= rangemultplan::LDS_THRESHOLD ? PATH_LDS : PATH_GLOBAL;
    p.threads = p.path == PATH_LDS ? LDS_THREADS : THREADS;
    p.ldsCounters = p.path == PATH_LDS ? (uint32_t)size : 0;
    p.offHeader = 0;
    p.offCounters = HEADER_BYTES;
    p.bytes = (HEADER_BYTES + COUNTER_BYTES * size + 15) & ~15ull;
    return p;
}

// workgroups of a count launch over ONE side of `rows` rows, rows > 0: the side's own rows decide, never the table's
inline uint32_t count_blocks(uint64_t rows, uint32_t path) {
    if (path != PATH_LDS) return smapplan::blocks(rows);
    const uint64_t want = (rows + LDS_THREADS - 1) / LDS_THREADS;
    return (uint32_t)(want < LDS_BLOCKS ? (want ? want : 1) : LDS_BLOCKS);
}

// ---- the buffers of a call: every matrix with the bytes THIS call touches of it ----
struct Spans {
    struct Span { const void *base; uint64_t bytes; } r[2 + 2 * MAX_SIDES];
    uint32_t count = 0;
    // side s over `rows` rows of k columns; it has passed check_side() for those rows.  rows = 0: nothing is touched, nothing is looked at
    void add(const pil2gl_tuple_side &s, uint64_t rows, uint64_t k, uint32_t words) {
        if (!rows) return;
        r[count++] = Span{ s.base, tupleside::matrix_bytes(s, rows, k, words) };
        if (s.sel) r[count++] = Span{ s.sel, tupleside::sel_bytes(s, rows, words) };
    }
};

// 0, or the message for PIL2GL_EINVAL: the matrices and the scratch are there, on 16 bytes, the scratch holds planBytes and meets no matrix
inline const char *check_spans(const Spans &all, const void *scratch, uint64_t scratchBytes, uint64_t planBytes, char (&why)[128]) {
    uintptr_t bits = (uintptr_t)scratch;
    bool null = !scratch;
    for (uint32_t i = 0; i < all.count; i++) { bits |= (uintptr_t)all.r[i].base; null = null || !all.r[i].base; }
    if (null) return "null buffer";
    if (bits & 15) return "the matrices, the selectors, m and the scratch must be 16-byte aligned";
    if (scratchBytes < planBytes) {
        snprintf(why, sizeof why, "the scratch holds %llu bytes, %llu needed", (unsigned long long)scratchBytes, (unsigned long long)planBytes);
        return why;
    }
    for (uint32_t i = 0; i < all.count; i++)
        if (smapplan::meets(scratch, planBytes, all.r[i].base, all.r[i].bytes)) return "the scratch overlaps a matrix of this call";
    return nullptr;
}

// the sides of an add: 0, or the message.  Each side's columns, strides and spans against ITS OWN row count
inline const char *check_add_sides(const pil2gl_tuple_side *f, const uint64_t *rows, uint64_t nF, uint64_t k, char (&why)[80]) {
    if (nF < 1 || nF > MAX_SIDES) return "nF must be 1 .. 8 sides of f";
    if (!f || !rows) return "null sides";
    for (uint64_t i = 0; i < nF; i++) {
        if (rows[i] > tupleside::MAX_N) { snprintf(why, sizeof why, "f %d: a side has at most 2^28 rows", (int)i); return why; }
        const char name[4] = { 'f', ' ', (char)('0' + i), 0 };
        if (rows[i] && tupleside::check_side(name, f[i], rows[i], k, why)) return why;
    }
    return nullptr;
}

// the m of a write, a column of n rows: 0, or the message.  t: the table's side of a lookup session (null: a range session reads no matrix)
inline const char *check_m(const Out &out, uint64_t n, uint32_t words, const pil2gl_tuple_side *t, uint64_t k, const void *scratch, uint64_t planBytes) {
    if (!out.m) return "null buffer";
    if ((uintptr_t)out.m & 15) return "the matrices, the selectors, m and the scratch must be 16-byte aligned";
    if (smapplan::meets(scratch, planBytes, out.m, tupleside::span_bytes(n, out.stride, out.col, words))) return "the scratch overlaps a matrix of this call";
    if (!t) return nullptr;
    const ReadMatrix reads[2] = { { t->base, t->stride, t->hostCols, k }, { t->sel, t->selStride, &t->selCol, 1 } };
    for (int i = 0; i < (t->sel ? 2 : 1); i++)
        if (!multcolumn::m_allowed(out.m, out.stride, out.col, reads[i], n, words))
            return "m overlaps a matrix that is read: it may only be a column of that matrix (its base, its stride) that is not read";
    return nullptr;
}

}  // namespace multsessionplan
