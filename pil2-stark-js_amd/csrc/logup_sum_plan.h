// Host-only half of the lookup grand sum (hints.hip over Goldilocks, bn_scan.hip over BN254 Fr): what the entries refuse, the launch
// geometry, the working bytes and the aliasing rule of the output column.  No HIP header: it builds with the plain C++ compiler
// (tests/logup_sum_plan_dump.cpp runs it under the sanitizers).  A term's side, its limits, column and span checks are
// tuple_side_plan.h's, the aliasing rule mult_column_plan.h's m_allowed over every word column of an output element, the scan's geometry
// hint_plan.h's (Goldilocks) and bn_scan_plan.h's (Fr).
//
// Working memory, neither growing with nTerms or k:
//   Goldilocks   what gsum takes: 3 words a row (the block-local sums) and 3 words a block of SCAN_CHUNK rows (the block totals)
//   Fr           bnscan::plan's bytes, then D and N of every row, 32 bytes each: 64 n
#pragma once
#include <stdint.h>
#include <stdio.h>
#include "hint_plan.h"
#include "bn_scan_plan.h"
#include "mult_column_plan.h"

namespace logupplan {

constexpr uint32_t MAX_TERMS = 9;                    // eight sides of f and t
constexpr uint64_t GL_P = 0xFFFFFFFF00000001ull;

// words of 64 bits an output element spans in its row: Goldilocks writes a cubic-extension element into a row of u64 words (three columns),
// Fr one element
inline uint32_t out_width(uint32_t elemWords) { return elemWords == 1 ? 3 : 1; }

struct Plan {
    uint32_t threads, items, blocks, launches, depth; // items: rows a lane of the first pass takes; depth: totals a lane of pass 2 walks (Goldilocks), levels (Fr)
    uint64_t bytes;
};

// 0, or a message for PIL2GL_EINVAL
inline const char *check(uint64_t n, uint64_t nTerms, uint32_t elemWords) {
    if (elemWords != 1 && elemWords != 4) return "elemWords is 1 (Goldilocks) or 4 (BN254 Fr)";
    if (nTerms < 1 || nTerms > MAX_TERMS) return "nTerms must be 1 .. 9";
    if (n > tupleside::MAX_N) return "n must be at most 2^28 rows";
    return nullptr;
}

// the arguments have passed check()
inline Plan plan(uint64_t n, uint32_t elemWords) {
    Plan p{};
    if (elemWords == 1) {                            // fused first pass, the totals' scan, the fix-up
        const uint64_t nb = hintplan::blocks(n);
        p.threads = hintplan::SCAN_THREADS; p.items = hintplan::SCAN_ITEMS; p.blocks = (uint32_t)nb; p.launches = n ? 3 : 0;
        p.depth = (uint32_t)hintplan::totals_per_lane(nb);
        p.bytes = 24 * n + 24 * nb;
    } else {                                         // compress, then per level a reduce and a store of the inversion and of the scan (the last level: a store each)
        const bnscan::Plan s = bnscan::plan(n, false);
        p.threads = smapplan::THREADS; p.items = 1; p.blocks = n ? smapplan::blocks(n) : 0; p.launches = n ? 1 + 2 * (2 * s.nLevels - 1) : 0;
        p.depth = s.nLevels;
        p.bytes = n ? bnscan::scratch_bytes(s) + 64 * n : 0;
    }
    return p;
}

// The aliasing rule of out, the `width` word columns outCol .. outCol + width - 1 of (base, stride): m_allowed for each of them.  When the
// widest span meets a read matrix the others do (one base, none empty), so this is: out may meet a read matrix only with that matrix's
// base and stride, and with none of its read columns.
inline bool out_allowed(const void *base, uint64_t stride, uint64_t col, uint32_t width, const multcolumn::ReadMatrix &r, uint64_t n, uint32_t elemWords) {
    for (uint32_t w = width; w-- > 0;)
        if (!multcolumn::m_allowed(base, stride, col + w, r, n, elemWords)) return false;
    return true;
}

// What both forms refuse before any device call: 0, or the message for PIL2GL_EINVAL (made in `why` where it names a term).
// dev: the pointers are the device's, 16-byte aligned.
inline const char *check_call(const pil2gl_logup_term *terms, uint64_t nTerms, const uint64_t *alpha, const uint64_t *beta, const uint64_t *out,
                              uint64_t outStride, uint64_t outCol, uint64_t n, uint32_t elemWords, bool dev, char (&why)[96]) {
    using namespace tupleside;
    if (const char *m = check(n, nTerms, elemWords)) return m;
    if (!terms) return "null terms";
    if (!alpha || !beta) return "null alpha or beta";
    const uint32_t width = out_width(elemWords);
    for (uint64_t u = 0; u < nTerms; u++) {
        const pil2gl_logup_term &t = terms[u];
        char name[8], sideWhy[80];
        snprintf(name, sizeof name, "term %u", (unsigned)u);                     // nTerms <= 9: one digit
        if (t.k < 1 || t.k > MAX_K) { snprintf(why, sizeof why, "term %u: k must be 1 .. 16 columns", (unsigned)u); return why; }
        if (check_side(name, t.side, n, t.k, sideWhy)) { snprintf(why, sizeof why, "%s", sideWhy); return why; }
        if (elemWords == 1 && (t.coef[0] >= GL_P || t.busId[0] >= GL_P)) { snprintf(why, sizeof why, "term %u: coef and busId must be canonical", (unsigned)u); return why; }
    }
    uint64_t outCols[3] = { outCol, outCol + 1, outCol + 2 };
    if (outCol >> 32) return "out: a column >= stride";
    if (const char *m = check_columns(n, outStride, outCols, width)) { snprintf(why, sizeof why, "out: %s", m); return why; }
    if (!n) return nullptr;
    uintptr_t bits = (uintptr_t)out;
    bool null = !out;
    for (uint64_t u = 0; u < nTerms; u++) {
        bits |= (uintptr_t)terms[u].side.base | (uintptr_t)terms[u].side.sel;
        null = null || !terms[u].side.base;
    }
    if (null) return "null buffer";
    if (dev && (bits & 15)) return "every matrix, every numerator column and out must be 16-byte aligned";
    for (uint64_t u = 0; u < nTerms; u++) {
        const pil2gl_tuple_side &s = terms[u].side;
        const multcolumn::ReadMatrix reads[2] = { { s.base, s.stride, s.hostCols, terms[u].k }, { s.sel, s.selStride, &s.selCol, 1 } };
        for (int i = 0; i < (s.sel ? 2 : 1); i++)
            if (!out_allowed(out, outStride, outCol, width, reads[i], n, elemWords))
                return "out overlaps a matrix that is read: it may only be columns of that matrix (its base, its stride) that are not read";
    }
    return nullptr;
}

}  // namespace logupplan
