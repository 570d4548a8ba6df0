// Host-only half of the clustered logUp sum (hints.hip over Goldilocks, bn_scan.hip over BN254 Fr): what the entries refuse, the plan, the
// rules of the cluster array and of the im descriptors, and the aliasing rule of SEVERAL outputs -- s and one im column a cluster.  No HIP
// header: it builds with the plain C++ compiler (tests/logup_cluster_plan_dump.cpp runs it under the sanitizers).  The f terms, the
// challenges and one output's own checks are logup_sum_plan.h's check_call, the ranges range_sum_plan.h's; both are CALLED here, once an
// output, so that every output obeys logupplan::out_allowed against every matrix read (each m_r over all n rows).  What this file adds:
//   the cluster array    one entry a term, f terms first, each 0 .. nIm - 1 or DIRECT; every id 0 .. nIm - 1 used
//   the im descriptors   check_columns over an element's word columns, null and misaligned bases
//   output against output: two outputs may share no word.  Their spans may meet only when they lie in ONE matrix -- the same base, the same
//                        stride -- with disjoint word columns, the normal case (s and its im columns as neighbouring stage-2 columns)
//
// Working memory, growing with neither the terms nor nIm:
//   Goldilocks   logup_sum's: 3 words a row and 3 words a block
//   Fr           bnscan::plan's bytes, then P of every row, 32 bytes: 32 n (logup_sum keeps D and N, 64 n)
#pragma once
#include <stdint.h>
#include <stdio.h>
#include "logup_sum_plan.h"
#include "range_sum_plan.h"

namespace logupclusterplan {

constexpr uint32_t MAX_IM = 9;                       // a cluster holds a term at least, a call nine terms at most
constexpr uint32_t MAX_GROUPS = 9;                   // the clusters and the DIRECT part, each with a term: nine at most
constexpr uint64_t DIRECT = PIL2GL_LOGUP_DIRECT;
constexpr uint32_t GL_ITEMS = hintplan::SCAN_ITEMS;  // rows a lane of cluster_scan1
using logupplan::Plan;

// 0, or a message for PIL2GL_EINVAL
inline const char *check(uint64_t n, uint64_t nF, uint64_t nR, uint64_t nIm, uint32_t elemWords) {
    if (elemWords != 1 && elemWords != 4) return "elemWords is 1 (Goldilocks) or 4 (BN254 Fr)";
    if (nF > rangesumplan::MAX_F) return "nF must be at most 8 terms of f";
    if (nR > rangesumplan::MAX_RANGES) return "nR must be at most 8 ranges";
    if (nF + nR < 1 || nF + nR > rangesumplan::MAX_TOTAL) return "nF + nR must be 1 .. 9";
    if (nIm < 1 || nIm > MAX_IM) return "nIm must be 1 .. 9 clusters";
    if (n > tupleside::MAX_N) return "n must be at most 2^28 rows";
    return nullptr;
}

// the arguments have passed check().  Goldilocks: logup_sum's three launches with cluster_scan1 as the first.  Fr: the product kernel, the
// inversion's launches, the refold, the scan's launches
inline Plan plan(uint64_t n, uint32_t elemWords) {
    Plan p = logupplan::plan(n, elemWords);
    if (elemWords == 1) p.items = GL_ITEMS;
    else if (n) {
        const bnscan::Plan s = bnscan::plan(n, false);
        p.launches = 2 + 2 * (2 * s.nLevels - 1);
        p.bytes = bnscan::scratch_bytes(s) + 32 * n;
    }
    return p;
}

// the cluster array: 0, or the message
inline const char *check_clusters(const uint64_t *cluster, uint64_t nTerms, uint64_t nIm, char (&why)[96]) {
    if (!cluster) return "null cluster array";
    uint32_t used = 0;
    for (uint64_t u = 0; u < nTerms; u++) {
        if (cluster[u] == DIRECT) continue;
        if (cluster[u] >= nIm) { snprintf(why, sizeof why, "term %u: its cluster must be 0 .. nIm - 1 or PIL2GL_LOGUP_DIRECT", (unsigned)u); return why; }
        used |= 1u << cluster[u];
    }
    for (uint64_t c = 0; c < nIm; c++)
        if (!((used >> c) & 1)) { snprintf(why, sizeof why, "cluster %u has no term", (unsigned)c); return why; }
    return nullptr;
}

// two outputs, each `width` word columns from col of (base, stride), checked by check_columns: do they share no word?
inline bool outputs_apart(const void *a, uint64_t aStride, uint64_t aCol, const void *b, uint64_t bStride, uint64_t bCol, uint32_t width, uint64_t n,
                          uint32_t elemWords) {
    using namespace tupleside;
    if (!smapplan::meets(a, span_bytes(n, aStride, aCol + width - 1, elemWords), b, span_bytes(n, bStride, bCol + width - 1, elemWords))) return true;
    if (a != b || aStride != bStride) return false;
    return aCol + width <= bCol || bCol + width <= aCol;
}

// What both forms refuse before any device call: 0, or the message for PIL2GL_EINVAL (made in `why` where it names something).
// dev: the pointers are the device's, 16-byte aligned.
inline const char *check_call(const pil2gl_logup_term *terms, uint64_t nF, const pil2gl_range_term *ranges, uint64_t nR, const uint64_t *cluster,
                              const pil2gl_logup_im_col *im, uint64_t nIm, const uint64_t *alpha, const uint64_t *beta, const uint64_t *out,
                              uint64_t outStride, uint64_t outCol, uint64_t n, uint32_t elemWords, bool dev, char (&why)[96]) {
    using namespace tupleside;
    if (const char *m = check(n, nF, nR, nIm, elemWords)) return m;
    if (const char *m = check_clusters(cluster, nF + nR, nIm, why)) return m;
    if (!im) return "null im descriptors";
    const uint32_t width = logupplan::out_width(elemWords);
    for (uint64_t c = 0; c < nIm; c++) {
        const uint64_t cols[3] = { im[c].col, im[c].col + 1, im[c].col + 2 };
        const char *m = im[c].col >> 32 ? "a column >= stride" : check_columns(n, im[c].stride, cols, width);
        if (m) { snprintf(why, sizeof why, "im %u: %s", (unsigned)c, m); return why; }
        if (n && !im[c].base) return "null buffer";
        if (n && dev && ((uintptr_t)im[c].base & 15)) return "every im column's matrix must be 16-byte aligned";
    }
    // every output against the terms, the ranges and the matrices they read: the checks of logup_sum and range_sum, output by output (the
    // first call is the one that speaks about the terms, the ranges, the challenges and s)
    for (uint64_t o = 0; o <= nIm; o++) {
        const uint64_t *base = o ? im[o - 1].base : out;
        const uint64_t stride = o ? im[o - 1].stride : outStride, col = o ? im[o - 1].col : outCol;
        const char *m = nR ? rangesumplan::check_call(terms, nF, ranges, nR, alpha, beta, base, stride, col, n, elemWords, dev, why)
                           : logupplan::check_call(terms, nF, alpha, beta, base, stride, col, n, elemWords, dev, why);
        if (m && o && m != why) { snprintf(why, sizeof why, "im %u: %s", (unsigned)(o - 1), m); return why; }
        if (m) return m;
    }
    if (!n) return nullptr;
    for (uint64_t a = 0; a <= nIm; a++)
        for (uint64_t b = a + 1; b <= nIm; b++) {
            const bool ok = outputs_apart(a ? (const void *)im[a - 1].base : (const void *)out, a ? im[a - 1].stride : outStride, a ? im[a - 1].col : outCol,
                                          im[b - 1].base, im[b - 1].stride, im[b - 1].col, width, n, elemWords);
            if (!ok) return "two outputs overlap: s and the im columns may only meet as different word columns of one matrix (its base, its stride)";
        }
    return nullptr;
}

// the 64-bit words of a host output matrix that are staged: from its first element to the last word written
inline uint64_t out_words(uint64_t n, uint64_t stride, uint64_t col, uint32_t elemWords) {
    return tupleside::span_bytes(n, stride, col + (elemWords == 1 ? 2 : 0), elemWords) / 8;
}

// ---- staging of the host form: the DISTINCT output matrices ----
// Outputs that share a base and a stride are one matrix, staged once up to the last word any of them writes, so that words between the
// columns go up and come back as they are.  group[o]: the first output (0 = s, c + 1 = im_c) with o's base and stride; words[o]: for such a
// first output, the words of its matrix.  Outputs in different matrices do not meet (check_call)
struct OutGroups { uint32_t group[MAX_IM + 1]; uint64_t words[MAX_IM + 1]; };
inline OutGroups out_groups(const pil2gl_logup_im_col *im, uint64_t nIm, const uint64_t *out, uint64_t outStride, uint64_t outCol, uint64_t n, uint32_t elemWords) {
    OutGroups g{};
    for (uint32_t o = 0; o <= nIm; o++) {
        const void *base = o ? (const void *)im[o - 1].base : (const void *)out;
        const uint64_t stride = o ? im[o - 1].stride : outStride, col = o ? im[o - 1].col : outCol;
        uint32_t first = o;
        for (uint32_t e = 0; e < o; e++)
            if ((e ? (const void *)im[e - 1].base : (const void *)out) == base && (e ? im[e - 1].stride : outStride) == stride) { first = e; break; }
        g.group[o] = first;
        const uint64_t w = out_words(n, stride, col, elemWords);
        if (w > g.words[first]) g.words[first] = w;
    }
    return g;
}

// The host form of either field, after check_call() and n > 0: the read matrices staged as range_sum's, every distinct output matrix up as it
// is, `launch` on the device copies (terms, ranges, im, out -> a PIL2GL code), the output matrices back.  Stage: common.h's, a template
// parameter to keep HIP out
template <class Stage, class Launch>
inline int host_form(const pil2gl_logup_term *hostTerms, uint64_t nF, const pil2gl_range_term *hostRanges, uint64_t nR, const pil2gl_logup_im_col *hostIm, uint64_t nIm,
                     uint64_t *hostOut, uint64_t outStride, uint64_t outCol, uint64_t n, uint32_t elemWords, Launch launch) {
    pil2gl_logup_term terms[rangesumplan::MAX_F];
    pil2gl_range_term ranges[rangesumplan::MAX_RANGES];
    pil2gl_logup_im_col im[MAX_IM];
    const OutGroups og = out_groups(hostIm, nIm, hostOut, outStride, outCol, n, elemWords);
    uint64_t total = 0;
    for (uint64_t o = 0; o <= nIm; o++) total += smapplan::pad16(og.words[o]);
    for (uint64_t u = 0; u < nF; u++) { terms[u] = hostTerms[u]; total += tupleside::staged_words(terms[u].side, n, terms[u].k, elemWords); }
    for (uint64_t r = 0; r < nR; r++) { ranges[r] = hostRanges[r]; total += smapplan::pad16(rangesumplan::m_words(ranges[r], elemWords)); }
    Stage s(total);
    if (int rc = s.rc()) return rc;
    for (uint64_t u = 0; u < nF; u++) tupleside::stage_side(s, terms[u].side, n, terms[u].k, elemWords);
    for (uint64_t r = 0; r < nR; r++) {
        const uint64_t w = rangesumplan::m_words(ranges[r], elemWords);
        ranges[r].m = s.put(ranges[r].m, w); s.take(smapplan::pad16(w) - w);
    }
    uint64_t *dev[MAX_IM + 1] = {};
    for (uint64_t o = 0; o <= nIm; o++) {
        if (og.group[o] != o) continue;
        const uint64_t w = og.words[o];
        dev[o] = (uint64_t *)s.put(o ? hostIm[o - 1].base : hostOut, w); s.take(smapplan::pad16(w) - w);
    }
    if (int rc = s.rc()) return rc;
    for (uint64_t c = 0; c < nIm; c++) im[c] = pil2gl_logup_im_col{ dev[og.group[c + 1]], hostIm[c].stride, hostIm[c].col };
    if (int rc = launch(terms, ranges, im, dev[og.group[0]])) return rc;
    for (uint64_t o = 0; o <= nIm; o++)
        if (og.group[o] == o)
            if (int rc = s.get(o ? hostIm[o - 1].base : hostOut, dev[o], og.words[o])) return rc;
    return 0;
}

}  // namespace logupclusterplan
