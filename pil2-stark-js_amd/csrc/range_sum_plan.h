// Host-only half of the range-check grand sum (hints.hip over Goldilocks, bn_scan.hip over BN254 Fr): what the entries refuse, the plan,
// the aliasing rule of the output column against the m columns, the bytes of an m matrix that a call touches, and the host-made constants
// of a range.  No HIP header: it builds with the plain C++ compiler (tests/range_sum_plan_dump.cpp runs it under the sanitizers).  The f
// terms, out's own checks and the plan are logup_sum_plan.h's; out against an m column is mult_column_plan.h's m_allowed over every word
// column of an output element (logupplan::out_allowed); the range's first element in either field is range_mult_plan.h's.
//
// Working memory: logup_sum's for the same n, growing with neither nF nor nR.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include "logup_sum_plan.h"
#include "range_mult_plan.h"

namespace rangesumplan {

constexpr uint32_t MAX_F = 8;                        // the f sides of a range check: range_mult's MAX_SIDES
constexpr uint32_t MAX_RANGES = 8;
constexpr uint32_t MAX_TOTAL = logupplan::MAX_TERMS; // f terms and ranges together
using rangemultplan::MAX_SIZE;
using logupplan::GL_P;
using logupplan::Plan;

// 0, or a message for PIL2GL_EINVAL
inline const char *check(uint64_t n, uint64_t nF, uint64_t nR, uint32_t elemWords) {
    if (elemWords != 1 && elemWords != 4) return "elemWords is 1 (Goldilocks) or 4 (BN254 Fr)";
    if (nR < 1 || nR > MAX_RANGES) return "nR must be 1 .. 8 ranges";
    if (nF > MAX_F) return "nF must be at most 8 terms of f";
    if (nF + nR > MAX_TOTAL) return "nF + nR must be at most 9";
    if (n > tupleside::MAX_N) return "n must be at most 2^28 rows";
    return nullptr;
}

// the arguments have passed check(): logup_sum's plan for the same n
inline Plan plan(uint64_t n, uint32_t elemWords) { return logupplan::plan(n, elemWords); }

// the rows of an m matrix that a call touches: up to the window's last
inline uint64_t m_rows(const pil2gl_range_term &r) { return r.row0 + r.size; }
// the 64-bit words of a host m matrix that are staged: from its first element to the window's last element of column mCol
inline uint64_t m_words(const pil2gl_range_term &r, uint32_t elemWords) { return tupleside::span_bytes(m_rows(r), r.mStride, r.mCol, elemWords) / 8; }

// What both forms refuse before any device call: 0, or the message for PIL2GL_EINVAL (made in `why` where it names a term or a range).
// dev: the pointers are the device's, 16-byte aligned.
inline const char *check_call(const pil2gl_logup_term *terms, uint64_t nF, const pil2gl_range_term *ranges, uint64_t nR, const uint64_t *alpha,
                              const uint64_t *beta, const uint64_t *out, uint64_t outStride, uint64_t outCol, uint64_t n, uint32_t elemWords, bool dev,
                              char (&why)[96]) {
    using namespace tupleside;
    if (const char *m = check(n, nF, nR, elemWords)) return m;
    if (!ranges) return "null ranges";
    const uint32_t width = logupplan::out_width(elemWords);
    if (nF) {                                        // the f terms, the challenges and out, also out against the f terms' matrices
        if (const char *m = logupplan::check_call(terms, nF, alpha, beta, out, outStride, outCol, n, elemWords, dev, why)) return m;
    } else {                                         // no f term: what that call says about the challenges and out alone
        if (!alpha || !beta) return "null alpha or beta";
        const uint64_t outCols[3] = { outCol, outCol + 1, outCol + 2 };
        if (outCol >> 32) return "out: a column >= stride";
        if (const char *m = check_columns(n, outStride, outCols, width)) { snprintf(why, sizeof why, "out: %s", m); return why; }
        if (n && !out) return "null buffer";
        if (n && dev && ((uintptr_t)out & 15)) return "every matrix, every numerator column and out must be 16-byte aligned";
    }
    for (uint64_t r = 0; r < nR; r++) {
        const pil2gl_range_term &t = ranges[r];
        if (t.size < 1 || t.size > MAX_SIZE) { snprintf(why, sizeof why, "range %u: size must be 1 .. 2^28 values", (unsigned)r); return why; }
        if (const char *m = check_columns(n, t.mStride, &t.mCol, 1)) { snprintf(why, sizeof why, "range %u: m: %s", (unsigned)r, m); return why; }
        if (elemWords == 1 && (t.coef[0] >= GL_P || t.busId[0] >= GL_P)) { snprintf(why, sizeof why, "range %u: coef and busId must be canonical", (unsigned)r); return why; }
        if (n && rangemultplan::check_rows(n, t.size, t.row0)) { snprintf(why, sizeof why, "range %u: the window ends past row n - 1: row0 + size > n", (unsigned)r); return why; }
    }
    if (!n) return nullptr;
    for (uint64_t r = 0; r < nR; r++) {
        const pil2gl_range_term &t = ranges[r];
        if (!t.m) return "null buffer";
        if (dev && ((uintptr_t)t.m & 15)) return "every m must be 16-byte aligned";
        const multcolumn::ReadMatrix read = { t.m, t.mStride, &t.mCol, 1 };
        if (!logupplan::out_allowed(out, outStride, outCol, width, read, n, elemWords))
            return "out overlaps an m matrix: it may only be columns of that matrix (its base, its stride) other than m";
    }
    return nullptr;
}

// ---- the host-made constants of a range ----
// Goldilocks: E_r[i] = c0 + alpha (i - row0), c0 = alpha field(lo) + busId + beta, an extension element.  mul and add are the caller's base
// field (common.h's h_mul / h_add in the library, Python-checked integers in the dump program); alpha and beta canonical
template <class Mul, class Add>
inline void gl_c0(const pil2gl_range_term &r, const uint64_t alpha[3], const uint64_t beta[3], Mul mul, Add add, uint64_t c0[3]) {
    const uint64_t lo = rangemultplan::lo_mod_p(r.lo);
    for (int c = 0; c < 3; c++) c0[c] = add(mul(alpha[c], lo), beta[c]);
    c0[0] = add(c0[0], r.busId[0]);
}

}  // namespace rangesumplan
