// Host-only half of the plookup argument of pil1 (hints.hip over Goldilocks, bn_scan.hip over BN254 Fr): what the fold and the product
// entries refuse, the launch geometry, the working bytes and the packed job that travels as a kernel argument.  No HIP header: it builds
// with the plain C++ compiler (tests/plookup_plan_dump.cpp runs it under the sanitizers).  A side's limits, column and span checks are
// tuple_side_plan.h's; the geometry, the working bytes and the aliasing rule of a written column are logup_sum_plan.h's (the same
// first-pass shape, the same scans behind it), the selector and the h matrices counting as read matrices.
//
// The job: two packed sides (strides and columns as u32, check_columns keeps them below 2^32), the two h columns, and what the rows
// share -- the powers of alpha, beta, gamma, delta and, over Goldilocks, g = gamma (1 + delta), 1 + delta and hDim.  W: u64 words of a challenge (3 Goldilocks, 4 Fr).
//   Goldilocks   alpha^1 .. alpha^15, g and 1 + delta made by the caller, so that a tuple column costs a base-times-extension scaling
//   Fr           alpha itself (a Horner step is one Montgomery product either way); g and 1 + delta are made by the kernel, once a lane
#pragma once
#include <stdint.h>
#include <stdio.h>
#include "logup_sum_plan.h"

namespace plookupplan {

using logupplan::out_width;
using logupplan::Plan;

// a column of `width` words an element: element i at word i stride + col of base (over Fr: element i stride + col)
struct Column { const uint64_t *base; uint64_t stride, col; };

// words an h element takes in its row: hDim over Goldilocks (1 or 3), one element over Fr
inline bool hdim_ok(uint32_t hDim, uint32_t elemWords) { return elemWords == 1 ? (hDim == 1 || hDim == 3) : hDim == 1; }

// 0, or a message for PIL2GL_EINVAL
inline const char *check(uint64_t n, uint64_t kF, uint64_t kT, uint32_t elemWords) {
    if (elemWords != 1 && elemWords != 4) return "elemWords is 1 (Goldilocks) or 4 (BN254 Fr)";
    if (kF < 1 || kF > tupleside::MAX_K) return "kF must be 1 .. 16 columns";
    if (kT < 1 || kT > tupleside::MAX_K) return "kT must be 1 .. 16 columns";
    if (n > tupleside::MAX_N) return "n must be at most 2^28 rows";
    return nullptr;
}

// the arguments have passed check(): the fused first pass (Goldilocks) or the compress (Fr), then the scans of logup_sum's plan with the
// product in place of the sum -- the same launches, the same bytes
inline Plan plan(uint64_t n, uint32_t elemWords) { return logupplan::plan(n, elemWords); }

// a side and an h column as the kernels read them
struct Side {
    const void *base, *sel;                          // sel: null when the side has none
    uint32_t stride, selStride, selCol, k;
    uint32_t cols[tupleside::MAX_K];
};
struct HCol { const void *base; uint32_t stride, col; };
// what the host makes for the Goldilocks kernels alone: g, 1 + delta and the words of an h element (the Fr kernels make the first two
// themselves and know one element)
template <uint32_t W, bool HOST> struct Derived { uint64_t g[W], onePlusDelta[W]; uint32_t hDim; };
template <uint32_t W> struct Derived<W, false> {};
template <uint32_t W, uint32_t POWERS, bool HOST> struct Job : Derived<W, HOST> {
    Side f, t;
    HCol h1, h2;
    uint64_t apow[POWERS][W];                        // apow[e - 1] = alpha^e
    uint64_t beta[W], gamma[W], delta[W];
    uint64_t n;
};
typedef Job<3, tupleside::MAX_K - 1, true> GlJob;
typedef Job<4, 1, false> FrJob;
static_assert(sizeof(Side) == 96 && sizeof(HCol) == 16, "a packed side, a packed h column");
// beside the job a kernel takes at most four pointers and the Fr one its Montgomery 1
static_assert(sizeof(GlJob) + 64 <= 4096 && sizeof(FrJob) + 64 <= 4096, "the job must fit a kernel's 4 KB of arguments");

inline Side pack_side(const pil2gl_tuple_side &h, uint64_t k) {
    Side s{};
    s.base = h.base; s.sel = h.sel; s.stride = (uint32_t)h.stride; s.k = (uint32_t)k;
    s.selStride = h.sel ? (uint32_t)h.selStride : 0; s.selCol = h.sel ? (uint32_t)h.selCol : 0;
    for (uint32_t j = 0; j < k; j++) s.cols[j] = (uint32_t)h.hostCols[j];
    return s;
}
inline HCol pack_column(const Column &c) { return HCol{ c.base, (uint32_t)c.stride, (uint32_t)c.col }; }

// the job of a call that has passed check_call(); the challenges are copied as they are given (the caller canonicalises).  h1, h2: the
// product's columns; the fold leaves them null and passes its outputs beside the job.  gamma .. onePlusDelta: null for the fold; g,
// onePlusDelta and hDim go into a job that has them
template <uint32_t W, uint32_t POWERS, bool HOST>
inline void pack(const pil2gl_tuple_side &f, uint64_t kF, const pil2gl_tuple_side &t, uint64_t kT, const Column *h1, const Column *h2, uint32_t hDim,
                 const uint64_t (*apow)[W], const uint64_t *beta, const uint64_t *gamma, const uint64_t *delta, const uint64_t *g, const uint64_t *onePlusDelta,
                 uint64_t n, Job<W, POWERS, HOST> &J) {
    J.f = pack_side(f, kF); J.t = pack_side(t, kT);
    if (h1) J.h1 = pack_column(*h1);
    if (h2) J.h2 = pack_column(*h2);
    for (uint32_t e = 0; e < POWERS; e++) for (uint32_t w = 0; w < W; w++) J.apow[e][w] = apow[e][w];
    for (uint32_t w = 0; w < W; w++) {
        J.beta[w] = beta[w];
        J.gamma[w] = gamma ? gamma[w] : 0; J.delta[w] = delta ? delta[w] : 0;
        if constexpr (HOST) { J.g[w] = g ? g[w] : 0; J.onePlusDelta[w] = onePlusDelta ? onePlusDelta[w] : 0; }
    }
    if constexpr (HOST) J.hDim = hDim;
    J.n = n;
}

// the matrices a call reads: f, t, their selectors, then the h columns (the product) -- at most six
struct Reads {
    multcolumn::ReadMatrix r[6];
    uint64_t hCols[2][3];
    uint32_t count = 0;
    void side(const pil2gl_tuple_side &s, uint64_t k) {
        r[count++] = multcolumn::ReadMatrix{ s.base, s.stride, s.hostCols, k };
        if (s.sel) r[count++] = multcolumn::ReadMatrix{ s.sel, s.selStride, &s.selCol, 1 };
    }
    void column(const Column &c, uint32_t width, int which) {
        for (uint32_t w = 0; w < 3; w++) hCols[which][w] = c.col + w;
        r[count++] = multcolumn::ReadMatrix{ c.base, c.stride, hCols[which], width };
    }
};

// a column that is read or written, `width` words wide: 0, or the message made in `why`
inline const char *check_column(const char *name, const Column &c, uint32_t width, uint64_t n, char (&why)[96]) {
    const uint64_t cols[3] = { c.col, c.col + 1, c.col + 2 };
    const char *m = (c.col >> 32) ? "a column >= stride" : tupleside::check_columns(n, c.stride, cols, width);
    if (m) { snprintf(why, sizeof why, "%s: %s", name, m); return why; }
    return nullptr;
}

// What both forms of both entries refuse before any device call: 0, or the message for PIL2GL_EINVAL (made in `why` where it names a part).
// The product: reads h1 and h2 (nRead = 2) and writes out[0] = z, three words over Goldilocks.  The fold: reads no column (nRead = 0) and
// writes out[0] = F and out[1] = T, hDim words each.  ch: the nCh challenges.  dev: the pointers are the device's, 16-byte aligned.
inline const char *check_call(const pil2gl_tuple_side *f, uint64_t kF, const pil2gl_tuple_side *t, uint64_t kT, const Column *read, uint32_t nRead, uint32_t hDim,
                              const uint64_t *const *ch, uint32_t nCh, const Column *out, uint32_t nOut, uint64_t n, uint32_t elemWords, bool dev, char (&why)[96]) {
    using namespace tupleside;
    if (const char *m = check(n, kF, kT, elemWords)) return m;
    if (!hdim_ok(hDim, elemWords)) return "hDim is 1 or 3 over Goldilocks and 1 over BN254 Fr";
    if (!f || !t) return "null side";
    for (uint32_t c = 0; c < nCh; c++) if (!ch[c]) return "null challenge";
    const bool fold = nRead == 0;
    if (fold && elemWords == 1 && hDim == 1 && (kF != 1 || kT != 1 || t->sel)) return "hDim = 1 takes kF = kT = 1 and no selT: anything else is an extension element";
    const uint32_t hWidth = elemWords == 1 ? hDim : 1, outWidth = fold ? hWidth : out_width(elemWords);
    char sideWhy[80];
    if (check_side("f", *f, n, kF, sideWhy)) { snprintf(why, sizeof why, "%s", sideWhy); return why; }
    if (check_side("t", *t, n, kT, sideWhy)) { snprintf(why, sizeof why, "%s", sideWhy); return why; }
    static const char *const readNames[2] = { "h1", "h2" }, *const foldNames[2] = { "outF", "outT" };
    for (uint32_t i = 0; i < nRead; i++) if (const char *m = check_column(readNames[i], read[i], hWidth, n, why)) return m;
    for (uint32_t i = 0; i < nOut; i++) if (const char *m = check_column(fold ? foldNames[i] : "out", out[i], outWidth, n, why)) return m;
    if (!n) return nullptr;
    uintptr_t bits = (uintptr_t)f->base | (uintptr_t)f->sel | (uintptr_t)t->base | (uintptr_t)t->sel;
    bool null = !f->base || !t->base;
    for (uint32_t i = 0; i < nRead; i++) { bits |= (uintptr_t)read[i].base; null = null || !read[i].base; }
    for (uint32_t i = 0; i < nOut; i++) { bits |= (uintptr_t)out[i].base; null = null || !out[i].base; }
    if (null) return "null buffer";
    if (dev && (bits & 15)) return "every matrix, every selector, h1, h2 and every output must be 16-byte aligned";
    Reads all;
    all.side(*f, kF); all.side(*t, kT);
    for (uint32_t i = 0; i < nRead; i++) all.column(read[i], hWidth, (int)i);
    for (uint32_t i = 0; i < nOut; i++)
        for (uint32_t r = 0; r < all.count; r++)
            if (!logupplan::out_allowed(out[i].base, out[i].stride, out[i].col, outWidth, all.r[r], n, elemWords))
                return "an output overlaps a matrix that is read: it may only be columns of that matrix (its base, its stride) that are not read";
    if (nOut == 2) {                                 // the fold's two outputs against each other: one matrix's distinct columns, or apart
        Reads other;
        other.column(out[1], outWidth, 0);
        if (!logupplan::out_allowed(out[0].base, out[0].stride, out[0].col, outWidth, other.r[0], n, elemWords))
            return "outF overlaps outT: they may only be distinct columns of one matrix (one base, one stride)";
    }
    return nullptr;
}

// a read column of a host call staged as a side's parts are: the 64-bit words it takes, and the staging, after which base is the device's
inline uint64_t column_words(const Column &c, uint32_t width, uint64_t n, uint32_t words) { return tupleside::span_bytes(n, c.stride, c.col + width - 1, words) / 8; }
template <class Stage> inline void stage_column(Stage &st, Column &c, uint32_t width, uint64_t n, uint32_t words) {
    const uint64_t nw = column_words(c, width, n, words);
    c.base = st.put(c.base, nw); st.take(smapplan::pad16(nw) - nw);
}

}  // namespace plookupplan
