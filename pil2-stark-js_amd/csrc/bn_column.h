// The column contract of the BN254 Fr blocks (bn_poly, bn_scan, bn_h1h2, bn_polymul), host-only: what the entries refuse about a column,
// how two columns may lie to each other, how the host-pointer entries stage them.  No HIP header: it builds with the plain C++ compiler
// (tests/bn_column_dump.cpp walks it under the sanitizers).  A column is (ptr, stride, n): element i is the 32 bytes at ptr + 32 i stride.
#pragma once
#include <stdint.h>

namespace bncol {

constexpr uint64_t MAX_N = 1ull << 28;
// the refusals, before any device call: 0, or a message for PIL2GL_EINVAL
inline const char *check_size(uint64_t n) { return n > MAX_N ? "at most 2^28 rows" : nullptr; }
inline const char *check_stride(uint64_t stride) { return stride == 0 || stride >> 32 ? "1 <= stride < 2^32" : nullptr; }

// 64-bit words from a column's first to the end of its last element.  The one place that computes a span: (n - 1) * stride overflows 64
// bits for n near 2^28 with stride near 2^32; no such column fits in memory, and the entries never refused one, so it is left as it is.
inline uint64_t span_words(uint64_t n, uint64_t stride) { return n ? 4 * ((n - 1) * stride + 1) : 0; }

// Two columns, each with its own count:
//   either is empty, or byte ranges [ptr, ptr + 8 span_words) apart              -> APART
//   the same column (same ptr, same stride)                                     -> SAME   (allowed only where the operator says so)
//   equal strides, ptrs a multiple of 32 bytes apart but not of 32 stride bytes  -> APART  (two columns of one section: ranges meet, no element does)
//   anything else                                                               -> OVERLAP (refused without looking for a common element)
enum Relation { APART = 0, SAME = 1, OVERLAP = 2 };
inline Relation relation(uintptr_t a, uint64_t aStride, uint64_t aN, uintptr_t b, uint64_t bStride, uint64_t bN) {
    if (aN == 0 || bN == 0) return APART;
    if (a == b && aStride == bStride) return SAME;
    if (a + 8 * span_words(aN, aStride) <= b || b + 8 * span_words(bN, bStride) <= a) return APART;
    if (aStride == bStride) {
        const uint64_t d = a > b ? a - b : b - a;
        if (d % 32 == 0 && d % (32 * aStride) != 0) return APART;
    }
    return OVERLAP;
}
inline Relation relation(uintptr_t a, uint64_t aStride, uintptr_t b, uint64_t bStride, uint64_t n) { return relation(a, aStride, n, b, bStride, n); }

// ---- staging a call's columns (the host-pointer entries) ----
// Every non-empty column lies in one staged range, consecutive words of the staging buffer that mirror host words [lo, lo + words):
//   alone, only read                       uploaded up to its last element
//   alone, written, not read, stride 1     taken: not uploaded, only copied back
//   alone, written, strided or also read   uploaded (the words between a strided column's elements travel, to come back unchanged)
//   ranges meet, one of the two written,   ONE range from the lowest start to the highest end, uploaded once and copied back once, so that
//   and the two are SAME or APART          neither copy back undoes the other; and so on through every column that range then meets
// A range is copied back, whole, when it holds a written column.  Two columns that are both only read stay two copies even where they
// meet, and so does an OVERLAP pair that an entry lets through (poly_div): nothing says their distance is a multiple of 16 bytes.
struct Col { uintptr_t ptr; uint64_t n, stride; bool read, written; };
constexpr uint32_t MAX_COLS = 4, NO_RANGE = ~0u;
struct Range { uintptr_t lo; uint64_t words; bool upload, download; };                // the ranges follow each other in the staging buffer
struct StagePlan {
    uint32_t nRanges;
    Range range[MAX_COLS];
    uint32_t of[MAX_COLS];                           // column -> its range, NO_RANGE for an empty column
    uint64_t off[MAX_COLS];                          // column -> its first word within its range
    uint64_t words;                                  // the staging buffer
};

inline StagePlan stage_plan(const Col *c, uint32_t nCols) {
    StagePlan p{};
    uint32_t group[MAX_COLS];                        // columns of one range carry one number
    auto end = [&](uint32_t i) { return c[i].ptr + 8 * span_words(c[i].n, c[i].stride); };
    for (uint32_t j = 0; j < nCols; j++) {
        group[j] = j;
        p.of[j] = NO_RANGE;
        for (uint32_t i = 0; i < j; i++) {
            const bool meet = c[i].n && c[j].n && end(i) > c[j].ptr && end(j) > c[i].ptr;
            if (!meet || !(c[i].written || c[j].written) || relation(c[i].ptr, c[i].stride, c[i].n, c[j].ptr, c[j].stride, c[j].n) == OVERLAP) continue;
            for (uint32_t k = 0, from = group[i]; k < j; k++) if (group[k] == from) group[k] = group[j];
        }
    }
    for (uint32_t g = 0; g < nCols; g++) {
        if (p.of[g] != NO_RANGE || !c[g].n) continue;
        Range &r = p.range[p.nRanges];
        uintptr_t hi = 0;
        uint32_t members = 0;
        bool read = false;
        r.lo = c[g].ptr;
        for (uint32_t k = g; k < nCols; k++) {
            if (group[k] != group[g] || !c[k].n) continue;
            if (c[k].ptr < r.lo) r.lo = c[k].ptr;
            if (end(k) > hi) hi = end(k);
            read |= c[k].read; r.download |= c[k].written;
            members++;
            p.of[k] = p.nRanges;
        }
        r.words = (hi - r.lo) / 8;
        r.upload = !(members == 1 && !read && c[g].stride == 1);
        p.words += r.words;
        p.nRanges++;
    }
    for (uint32_t k = 0; k < nCols; k++) if (p.of[k] != NO_RANGE) p.off[k] = (c[k].ptr - p.range[p.of[k]].lo) / 8;
    return p;
}

}  // namespace bncol
