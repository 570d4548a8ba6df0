// Host-only half of the grand product of a permutation or a connection (hints.hip over Goldilocks, bn_scan.hip over BN254 Fr): what the
// entries refuse, the launch geometry, the working bytes and the packed term table that travels as a kernel argument.  No HIP header: it
// builds with the plain C++ compiler (tests/grand_prod_plan_dump.cpp runs it under the sanitizers).  A term's side, its limits, column and
// span checks are tuple_side_plan.h's; the geometry, the working bytes and the aliasing rule of the output column are logup_sum_plan.h's
// (the same first-pass shape, the same scans behind it), the id and selector matrices counting as read matrices.
//
// The table: 40 terms with 64 tuple columns between them must fit the 4 KB of a kernel's arguments, so a term is packed -- strides and
// columns as u32 (check_columns keeps them below 2^32), its tuple's columns as a run `start .. start + k` of ONE list shared by all terms --
// and what the terms share is stored once: the powers of alpha, beta, gamma.  W: u64 words of a challenge (3 Goldilocks, 4 Fr).
//   Goldilocks   72 bytes a term; alpha^1 .. alpha^15 made by the caller, so that a tuple column costs a base-times-extension scaling
//   Fr           80 bytes a term; alpha itself (a Horner step is one Montgomery product either way)
#pragma once
#include <stdint.h>
#include <stdio.h>
#include "logup_sum_plan.h"

namespace grandprodplan {

constexpr uint32_t MAX_TERMS = 40;                   // an 18-column connection takes 36
constexpr uint32_t MAX_SUM_K = 64;
constexpr uint64_t GL_P = logupplan::GL_P;

using logupplan::out_width;
using logupplan::Plan;

// 0, or a message for PIL2GL_EINVAL
inline const char *check(uint64_t n, uint64_t nTerms, uint64_t sumK, uint32_t elemWords) {
    if (elemWords != 1 && elemWords != 4) return "elemWords is 1 (Goldilocks) or 4 (BN254 Fr)";
    if (nTerms < 1 || nTerms > MAX_TERMS) return "nTerms must be 1 .. 40";
    if (sumK < nTerms || sumK > MAX_SUM_K || sumK > tupleside::MAX_K * nTerms) return "the terms' k must add up to nTerms .. 64, each 1 .. 16";
    if (n > tupleside::MAX_N) return "n must be at most 2^28 rows";
    return nullptr;
}

// the arguments have passed check(): the fused first pass (Goldilocks) or the compress (Fr), then the scans of logup_sum's plan with the
// product in place of the sum -- the same launches, the same bytes
inline Plan plan(uint64_t n, uint32_t elemWords) { return logupplan::plan(n, elemWords); }

// a term as the kernels read it
template <uint32_t W> struct Term {
    const void *base, *sel, *id;                     // sel, id: null when the term has none
    uint32_t stride, selStride, idStride, selCol, idCol;
    uint16_t start;                                  // the tuple's columns: cols[start .. start + k)
    uint8_t k, den;
    uint64_t idCoef[W];
};
template <uint32_t W, uint32_t POWERS> struct Job {
    Term<W> t[MAX_TERMS];
    uint32_t cols[MAX_SUM_K];
    uint64_t apow[POWERS][W];                        // apow[e - 1] = alpha^e
    uint64_t beta[W], gamma[W];
    uint32_t nTerms;
    uint64_t n;
};
typedef Job<3, tupleside::MAX_K - 1> GlJob;
typedef Job<4, 1> FrJob;
static_assert(sizeof(Term<3>) == 72 && sizeof(Term<4>) == 80, "a packed term");
// beside the job a kernel takes at most four pointers and the Fr one its Montgomery 1
static_assert(sizeof(GlJob) + 64 <= 4096 && sizeof(FrJob) + 64 <= 4096, "the job must fit a kernel's 4 KB of arguments");

// the table of a call that has passed check_call(); the challenges are copied as they are given (the caller canonicalises)
template <uint32_t W, uint32_t POWERS>
inline void pack(const pil2gl_grand_prod_term *terms, uint32_t nTerms, const uint64_t (*apow)[W], const uint64_t *beta, const uint64_t *gamma, uint64_t n,
                 Job<W, POWERS> &J) {
    uint32_t at = 0;
    for (uint32_t u = 0; u < nTerms; u++) {
        const pil2gl_grand_prod_term &h = terms[u];
        Term<W> &T = J.t[u];
        T.base = h.side.base; T.sel = h.side.sel; T.id = h.id;
        T.stride = (uint32_t)h.side.stride;
        T.selStride = h.side.sel ? (uint32_t)h.side.selStride : 0; T.selCol = h.side.sel ? (uint32_t)h.side.selCol : 0;
        T.idStride = h.id ? (uint32_t)h.idStride : 0; T.idCol = h.id ? (uint32_t)h.idCol : 0;
        T.start = (uint16_t)at; T.k = (uint8_t)h.k; T.den = (uint8_t)h.den;
        for (uint32_t j = 0; j < T.k; j++) J.cols[at++] = (uint32_t)h.side.hostCols[j];
        for (uint32_t w = 0; w < W; w++) T.idCoef[w] = h.idCoef[w];
    }
    for (uint32_t e = 0; e < POWERS; e++) for (uint32_t w = 0; w < W; w++) J.apow[e][w] = apow[e][w];
    for (uint32_t w = 0; w < W; w++) { J.beta[w] = beta[w]; J.gamma[w] = gamma[w]; }
    J.nTerms = nTerms; J.n = n;
}

// What both forms refuse before any device call: 0, or the message for PIL2GL_EINVAL (made in `why` where it names a term).
// dev: the pointers are the device's, 16-byte aligned.
inline const char *check_call(const pil2gl_grand_prod_term *terms, uint64_t nTerms, const uint64_t *alpha, const uint64_t *beta, const uint64_t *gamma,
                              const uint64_t *out, uint64_t outStride, uint64_t outCol, uint64_t n, uint32_t elemWords, bool dev, char (&why)[96]) {
    using namespace tupleside;
    if (const char *m = check(n, nTerms, nTerms, elemWords)) return m;           // the k are summed below
    if (!terms) return "null terms";
    if (!alpha || !beta || !gamma) return "null alpha, beta or gamma";
    const uint32_t width = out_width(elemWords);
    uint64_t sumK = 0;
    for (uint64_t u = 0; u < nTerms; u++) {
        const pil2gl_grand_prod_term &t = terms[u];
        char name[8], sideWhy[80];
        snprintf(name, sizeof name, "term %u", (unsigned)u);                     // nTerms <= 40: two digits
        if (t.k < 1 || t.k > MAX_K) { snprintf(why, sizeof why, "term %u: k must be 1 .. 16 columns", (unsigned)u); return why; }
        if (t.den > 1) { snprintf(why, sizeof why, "term %u: den is 0 (numerator) or 1 (denominator)", (unsigned)u); return why; }
        if (check_side(name, t.side, n, t.k, sideWhy)) { snprintf(why, sizeof why, "%s", sideWhy); return why; }
        if (t.id) if (const char *m = check_columns(n, t.idStride, &t.idCol, 1)) { snprintf(why, sizeof why, "id of term %u: %s", (unsigned)u, m); return why; }
        if (elemWords == 1 && (t.idCoef[0] >= GL_P || t.idCoef[1] >= GL_P || t.idCoef[2] >= GL_P)) {
            snprintf(why, sizeof why, "term %u: idCoef must be canonical", (unsigned)u);
            return why;
        }
        sumK += t.k;
    }
    if (const char *m = check(n, nTerms, sumK, elemWords)) return m;
    uint64_t outCols[3] = { outCol, outCol + 1, outCol + 2 };
    if (outCol >> 32) return "out: a column >= stride";
    if (const char *m = check_columns(n, outStride, outCols, width)) { snprintf(why, sizeof why, "out: %s", m); return why; }
    if (!n) return nullptr;
    uintptr_t bits = (uintptr_t)out;
    bool null = !out;
    for (uint64_t u = 0; u < nTerms; u++) {
        bits |= (uintptr_t)terms[u].side.base | (uintptr_t)terms[u].side.sel | (uintptr_t)terms[u].id;
        null = null || !terms[u].side.base;
    }
    if (null) return "null buffer";
    if (dev && (bits & 15)) return "every matrix, every selector and id column and out must be 16-byte aligned";
    for (uint64_t u = 0; u < nTerms; u++) {
        const pil2gl_grand_prod_term &t = terms[u];
        const pil2gl_tuple_side &s = t.side;
        const multcolumn::ReadMatrix reads[3] = { { s.base, s.stride, s.hostCols, t.k }, { s.sel, s.selStride, &s.selCol, 1 }, { t.id, t.idStride, &t.idCol, 1 } };
        for (int i = 0; i < 3; i++)
            if (reads[i].base && !logupplan::out_allowed(out, outStride, outCol, width, reads[i], n, elemWords))
                return "out overlaps a matrix that is read: it may only be columns of that matrix (its base, its stride) that are not read";
    }
    return nullptr;
}

// the id column of a host term staged as a side's parts are: the 64-bit words it takes, and the staging, after which id is the device's
inline uint64_t id_words(const pil2gl_grand_prod_term &t, uint64_t n, uint32_t words) { return t.id ? tupleside::span_bytes(n, t.idStride, t.idCol, words) / 8 : 0; }
template <class Stage> inline void stage_id(Stage &st, pil2gl_grand_prod_term &t, uint64_t n, uint32_t words) {
    const uint64_t nId = id_words(t, n, words);
    t.id = st.put(t.id, nId); st.take(smapplan::pad16(nId) - nId);
}

}  // namespace grandprodplan
