// Grand product, grand sum and batch inverse over the BN254 scalar field Fr, gfx950: what resolves the gprod / gsum hints of a fflonk
// stage with a permutation, connection or lookup argument (src/prover/hints_helpers.js:92-113; calculateZ / calculateS of
// src/helpers/polutils.js:132-164 with F = curve.Fr, one F.batchInverse and a serial walk of N products each).
//
//     batch_inverse   dst[i] = src[i]^-1
//     gprod           z[0] = 1,  z[i] = z[i - 1] num[i - 1] / den[i - 1]
//     gsum            s[i] = s[i - 1] + num / den[i],  s[0] = num / den[0]          (num: ONE element, on the host)
//     gsum_col        s[i] = s[i - 1] + num[i] / den[i]                              (num: a column, as gprod's)
//     logup_sum       the lookup grand sum of include/pil2gl.h: gsum_col over a row's terms folded into one fraction (near the end of this file)
//     range_sum       that sum with the table side of a range check given as numbers, no t column (behind it)
//     logup_cluster   those sums with the terms gathered into clusters: s and one im column a cluster (behind them)
//     grand_prod      the grand product of a permutation or a connection: gprod over a row's terms multiplied into N and D (near the end)
//     plookup         pil1's plookup argument: the fold of F and T, and gprod over a row's num and den made from f, t, h1, h2 (at the end)
//
// Elements are 32 bytes of Montgomery words, canonical in and out, moved as two 16-byte halves; element i of a column lies at word
// 4 i stride, so a column of a row-major section is worked on where it is (as poly_div and g1_msm take theirs).
//
// ZERO DENOMINATORS -- a stated choice.  The reference's Fr is ffjavascript's wasm field, which the reference tree does not vendor, so
// what its batchInverse makes of a zero cannot be pinned from here.  This library's own convention is used (include/pil2gl.h on the
// Goldilocks hints, fq_inv of bn_fq.cuh: 0 -> 0): a zero inverts to zero and is kept out of every running product, so it spoils no other
// row's inverse.  In gprod the ratio of that row is then 0 and every later row is 0; in gsum the row adds 0.  A zero NUMERATOR is plain
// arithmetic.
//
// Arithmetic.  One Fermat inversion is about 380 products of 328 vector instructions each (DESIGN.md section 14's count), so there is one
// per call, on one lane, and everything else is Montgomery's trick spread over lanes.  bnscan::plan (bn_scan_plan.h) cuts the n items
// into S segments of L, a lane per segment [s L, min((s + 1) L, n)):
//   inversion   reduce: a lane leaves the product of its segment (zeros left out).  Those S products are the same problem one level up,
//               inverted in place; the last level is one lane, which inverts its total with the ladder.  store: a lane walks its segment
//               upwards writing the prefix products q[i], takes r = 1 / (its segment's product) from the level above, and walks back down:
//               y[i] = r q[i - 1] (times the numerator for the two hints), r = r x[i].  1 + 3 products per row, + 1 with a numerator.
//               The prefixes are kept in the destination itself (read back before each element is overwritten); an inversion in place has
//               no such room and keeps them in the working buffer (n elements more).
//   scan        the hints then run a prefix scan over the ratios, in place in the destination: reduce, the totals scanned one level up
//               (inclusive), store seeded with the total before the segment.  gprod: an exclusive running product, 2 products per row;
//               gsum: an inclusive running sum, additions only.
// Products per row, the levels above the first adding 1/15 at most: batch_inverse 4, gsum 5, gprod 7.  A level boundary is a kernel
// boundary; no workgroup waits for another.  The alternative of DESIGN.md section 15 (prefix and suffix products, 5 per row for gprod)
// was not taken: it needs a second strided temporary where this needs none.
//
// Memory safety does not rest on n being a multiple of anything: a lane with s >= S returns, a lane walks only [s L, min((s + 1) L, n)),
// and an empty segment leaves the identity.
#include "bn_column_stage.h"
#include "bn_elem.cuh"
#include "bn_params.h"
#include "bn_scan_plan.h"
#include "logup_sum_plan.h"
#include "range_sum_plan.h"
#include "logup_cluster_plan.h"
#include "grand_prod_plan.h"
#include "plookup_plan.h"
#include "tuple_side.cuh"

using namespace pil2gl;
using bn::u32;
using bn::ld_elem;
using bn::st_elem;
using bn::is_zero;

namespace {

struct Elem { u32 w[8]; };

enum Mode : u32 { MODE_NONE = 0, MODE_COLUMN = 1, MODE_CONST = 2 };      // what the inverses are multiplied by

struct InvArgs {
    const uint4 *x; u64 xs;                          // element i of the level at x + 2 i xs (16-byte halves)
    uint4 *y; u64 ys;                                // its inverse (may be x)
    uint4 *q; u64 qs;                                // the prefix products (may be y, never x)
    const uint4 *num; u64 ns;                        // MODE_COLUMN: the numerators
    const uint4 *vinv;                               // store: the inverses of the segment products (dense), unless this is the last level
    uint4 *v;                                        // reduce: the segment products (dense)
    u64 n, S; u32 L, mode;
    Elem one, mul;                                   // 1 in Montgomery form; MODE_CONST: the numerator
};
struct ScanArgs {
    uint4 *y; u64 ys;                                // scanned in place
    const uint4 *carry;                              // store: the inclusive scan of the segment totals (dense), or null when S = 1
    uint4 *v;                                        // reduce: the segment totals (dense)
    u64 n, S; u32 L, exclusive;
    Elem ident;                                      // 0, or 1 in Montgomery form
};

__device__ __forceinline__ void set(u32 x[8], const Elem &e) {
#pragma unroll
    for (int i = 0; i < 8; i++) x[i] = e.w[i];
}

// a^-1 = a^(r - 2), Montgomery in and out, a != 0: 252 squarings and a product per set bit below the top one (bit 253), the exponent's
// bits taken from r's constant limbs (r ends in ...f0000001: subtracting 2 borrows from no other limb).  One lane, once per call.
__device__ __noinline__ void fr_inv(u32 out[8], const u32 a[8]) {
    u32 acc[8];
#pragma unroll
    for (int i = 0; i < 8; i++) acc[i] = a[i];
    for (int bit = 252; bit >= 0; bit--) {
        bn::fr_mul(acc, acc, acc);
        u32 w = 0;
#pragma unroll
        for (int l = 0; l < 8; l++) if ((bit >> 5) == l) w = bn::r_limb(l) - (l == 0 ? 2u : 0u);
        if ((w >> (bit & 31)) & 1) bn::fr_mul(acc, acc, a);
    }
#pragma unroll
    for (int i = 0; i < 8; i++) out[i] = acc[i];
}

// the segment [b, e) of lane t; false for a lane without one
__device__ __forceinline__ bool segment(u64 n, u64 S, u32 L, u64 &t, u64 &b, u64 &e) {
    t = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= S) return false;
    b = t * L;
    e = b + L < n ? b + L : n;
    return true;
}

__global__ void __launch_bounds__(bnscan::THREADS) bn_inv_reduce_kernel(InvArgs a) {
    u64 t, b, e;
    if (!segment(a.n, a.S, a.L, t, b, e)) return;
    u32 acc[8], x[8];
    set(acc, a.one);
    const size_t step = 2 * (size_t)a.xs;
    const uint4 *px = a.x + b * step;
    for (u64 i = b; i < e; i++, px += step) {
        ld_elem(px, x);
        if (!is_zero(x)) bn::fr_mul(acc, acc, x);
    }
    st_elem(a.v + 2 * t, acc);
}

template <bool TOP>
__global__ void __launch_bounds__(bnscan::THREADS) bn_inv_store_kernel(InvArgs a) {
    u64 t, b, e;
    if (!segment(a.n, a.S, a.L, t, b, e) || b >= e) return;
    u32 r[8], x[8], p[8];
    set(r, a.one);
    const size_t xstep = 2 * (size_t)a.xs, qstep = 2 * (size_t)a.qs, ystep = 2 * (size_t)a.ys, nstep = 2 * (size_t)a.ns;
    const uint4 *px = a.x + b * xstep;
    uint4 *pq = a.q + b * qstep;
    for (u64 i = b; i < e; i++, px += xstep, pq += qstep) {       // up: q[i] = the product of the segment's non-zero elements up to i
        ld_elem(px, x);
        if (!is_zero(x)) bn::fr_mul(r, r, x);
        st_elem(pq, r);
    }
    if (TOP) fr_inv(r, r);                                        // a product of non-zero elements: never zero
    else ld_elem(a.vinv + 2 * t, r);
    uint4 *py = a.y + e * ystep;
    const uint4 *pn = a.num + e * nstep;
    for (u64 i = e; i-- > b;) {                                   // down: r = 1 / q[i]
        px -= xstep; pq -= qstep; py -= ystep; pn -= nstep;
        ld_elem(px, x);                                           // before y[i] is stored: y may be x
        if (i > b) ld_elem(pq - qstep, p); else set(p, a.one);    // q[i - 1] is below everything stored so far: q may be y
        if (is_zero(x)) {
#pragma unroll
            for (int l = 0; l < 8; l++) p[l] = 0;
        } else {
            bn::fr_mul(p, p, r);
            bn::fr_mul(r, r, x);
            if (a.mode == MODE_COLUMN) { ld_elem(pn, x); bn::fr_mul(p, p, x); }
            else if (a.mode == MODE_CONST) { set(x, a.mul); bn::fr_mul(p, p, x); }
        }
        st_elem(py, p);
    }
}

template <bool ADD>
__device__ __forceinline__ void combine(u32 acc[8], const u32 x[8]) {
    if (ADD) bn::fr_add(acc, x); else bn::fr_mul(acc, acc, x);
}

template <bool ADD>
__global__ void __launch_bounds__(bnscan::THREADS) bn_scan_reduce_kernel(ScanArgs a) {
    u64 t, b, e;
    if (!segment(a.n, a.S, a.L, t, b, e)) return;
    u32 acc[8], x[8];
    set(acc, a.ident);
    const size_t step = 2 * (size_t)a.ys;
    const uint4 *py = a.y + b * step;
    for (u64 i = b; i < e; i++, py += step) {
        ld_elem(py, x);
        combine<ADD>(acc, x);
    }
    st_elem(a.v + 2 * t, acc);
}

template <bool ADD>
__global__ void __launch_bounds__(bnscan::THREADS) bn_scan_store_kernel(ScanArgs a) {
    u64 t, b, e;
    if (!segment(a.n, a.S, a.L, t, b, e)) return;
    u32 acc[8], x[8];
    if (a.carry && t > 0) ld_elem(a.carry + 2 * (t - 1), acc); else set(acc, a.ident);
    const size_t step = 2 * (size_t)a.ys;
    uint4 *py = a.y + b * step;
    for (u64 i = b; i < e; i++, py += step) {
        ld_elem(py, x);
        if (a.exclusive) { st_elem(py, acc); combine<ADD>(acc, x); }
        else { combine<ADD>(acc, x); st_elem(py, acc); }
    }
}

unsigned blocks(u64 lanes) { return (unsigned)((lanes + bnscan::THREADS - 1) / bnscan::THREADS); }

// y[i] = mode(x[i]^-1) over the plan's levels; q: where level 0 keeps its prefixes (y, or the working buffer when y is x)
int inverse_launch(const bnscan::Plan &p, uint4 *base, const uint4 *x, u64 xs, uint4 *y, u64 ys, uint4 *q, u64 qs,
                   u32 mode, const uint4 *num, u64 ns, const Elem &mul, hipStream_t st) {
    auto values = [&](u32 i) { return base + 2 * p.lv[i].off; };
    auto args = [&](u32 i) {
        const bnscan::Level &l = p.lv[i];
        InvArgs a{};
        if (i == 0) { a.x = x; a.xs = xs; a.y = y; a.ys = ys; a.q = q; a.qs = qs; a.mode = mode; a.num = num; a.ns = ns; a.mul = mul; }
        else { a.x = values(i); a.y = values(i); a.q = values(i) + 2 * l.n; a.xs = a.ys = a.qs = 1; a.mode = MODE_NONE; }
        a.n = l.n; a.S = l.S; a.L = l.L; bnp::bn_limbs(bnp::bn_mont_one().w, a.one.w);
        return a;
    };
    const u32 last = p.nLevels - 1;
    for (u32 i = 0; i < last; i++) {
        InvArgs a = args(i);
        a.v = values(i + 1);
        bn_inv_reduce_kernel<<<blocks(a.S), bnscan::THREADS, 0, st>>>(a);
        KERNEL_CHECK();
    }
    for (u32 i = p.nLevels; i-- > 0;) {
        InvArgs a = args(i);
        if (i == last) bn_inv_store_kernel<true><<<1, 64, 0, st>>>(a);
        else { a.vinv = values(i + 1); bn_inv_store_kernel<false><<<blocks(a.S), bnscan::THREADS, 0, st>>>(a); }
        KERNEL_CHECK();
    }
    return PIL2GL_OK;
}

// the running sum (inclusive) or product (exclusive, from 1) of y, in place
template <bool ADD>
int scan_launch(const bnscan::Plan &p, uint4 *base, uint4 *y, u64 ys, hipStream_t st) {
    auto values = [&](u32 i) { return base + 2 * p.lv[i].off; };
    auto args = [&](u32 i) {
        const bnscan::Level &l = p.lv[i];
        ScanArgs a{};
        a.y = i ? values(i) : y; a.ys = i ? 1 : ys;
        a.n = l.n; a.S = l.S; a.L = l.L; a.exclusive = !ADD && i == 0;
        if (!ADD) bnp::bn_limbs(bnp::bn_mont_one().w, a.ident.w);
        return a;
    };
    const u32 last = p.nLevels - 1;
    for (u32 i = 0; i < last; i++) {
        ScanArgs a = args(i);
        a.v = values(i + 1);
        bn_scan_reduce_kernel<ADD><<<blocks(a.S), bnscan::THREADS, 0, st>>>(a);
        KERNEL_CHECK();
    }
    for (u32 i = p.nLevels; i-- > 0;) {
        ScanArgs a = args(i);
        a.carry = i < last ? values(i + 1) : nullptr;
        bn_scan_store_kernel<ADD><<<blocks(a.S), bnscan::THREADS, 0, st>>>(a);
        KERNEL_CHECK();
    }
    return PIL2GL_OK;
}

int run(u32 op, const u64 *num, u64 numStride, const u64 *hostNum, const u64 *den, u64 denStride, u64 n, u64 *out, u64 outStride, hipStream_t st) {
    if (n == 0) return PIL2GL_OK;
    const bool inPlace = op == bnscan::OP_BATCH_INVERSE && den == out;
    const bnscan::Plan p = bnscan::plan(n, inPlace);
    u64 *d = nullptr;
    if (p.elems) P2_TRY(scratch(SCR_BN_SCAN, 4 * p.elems, &d));
    uint4 *base = (uint4 *)d, *y = (uint4 *)out;
    uint4 *q = inPlace ? base + 2 * p.q0Off : y;
    const u32 mode = op == bnscan::OP_GPROD || (op == bnscan::OP_GSUM && num) ? MODE_COLUMN : op == bnscan::OP_GSUM ? MODE_CONST : MODE_NONE;   // gsum with num: gsum_col
    Elem mul{};
    if (hostNum) bnp::bn_limbs(hostNum, mul.w);
    P2_TRY(inverse_launch(p, base, (const uint4 *)den, denStride, y, outStride, q, inPlace ? 1 : outStride, mode, (const uint4 *)num, numStride, mul, st));
    if (op == bnscan::OP_GPROD) return scan_launch<false>(p, base, y, outStride, st);
    if (op == bnscan::OP_GSUM) return scan_launch<true>(p, base, y, outStride, st);
    return PIL2GL_OK;
}

int check_apart(const void *in, u64 inStride, const void *out, u64 outStride, u64 n, bool sameAllowed) {
    const bncol::Relation r = bncol::relation((uintptr_t)in, inStride, (uintptr_t)out, outStride, n);
    if (r == bncol::OVERLAP || (r == bncol::SAME && !sameAllowed))
        return fail(PIL2GL_EINVAL, "the output overlaps an input (only batch_inverse may run in place, on the same pointer and stride)");
    return PIL2GL_OK;
}
int check_inverse(const u64 *src, u64 srcStride, u64 n, const u64 *dst, u64 dstStride) {
    P2_TRY(check_column(src, n, srcStride, "src"));
    P2_TRY(check_column(dst, n, dstStride, "dst"));
    return check_apart(src, srcStride, dst, dstStride, n, true);
}
int check_gprod(const u64 *num, u64 numStride, const u64 *den, u64 denStride, u64 n, const u64 *out, u64 outStride) {
    P2_TRY(check_column(num, n, numStride, "num"));
    P2_TRY(check_column(den, n, denStride, "den"));
    P2_TRY(check_column(out, n, outStride, "out"));
    P2_TRY(check_apart(num, numStride, out, outStride, n, false));
    return check_apart(den, denStride, out, outStride, n, false);
}
int check_gsum(const u64 *hostNum, const u64 *den, u64 denStride, u64 n, const u64 *out, u64 outStride) {
    if (!hostNum) return fail(PIL2GL_EINVAL, "null buffer");
    P2_TRY(check_column(den, n, denStride, "den"));
    P2_TRY(check_column(out, n, outStride, "out"));
    return check_apart(den, denStride, out, outStride, n, false);
}
// the host-pointer forms: the columns staged by the one rule (bn_column.h), the operator, the written column copied back
int run_host(u32 op, const u64 *num, u64 numStride, const u64 *hostNum, const u64 *den, u64 denStride, u64 n, u64 *out, u64 outStride) {
    const bncol::Col cols[3] = { { (uintptr_t)den, n, denStride, true, false }, { (uintptr_t)out, n, outStride, false, true },
                                 { (uintptr_t)num, num ? n : 0, numStride, true, false } };
    ColumnStage s(cols, 3);
    P2_TRY(s.rc());
    P2_TRY(run(op, s.dev(2), numStride, hostNum, s.dev(0), denStride, n, s.dev(1), outStride, 0));
    return s.copy_back();
}

}  // namespace

extern "C" {

int pil2gl_debug_bn128_scan_plan(uint64_t n, uint32_t op, uint32_t *outInfo, uint64_t *scratchBytes) {
    if (!outInfo || !scratchBytes) return fail(PIL2GL_EINVAL, "null argument");
    if (const char *m = bncol::check_size(n)) return fail(PIL2GL_EINVAL, "n = %llu: %s", (unsigned long long)n, m);
    if (op >= bnscan::N_OPS) return fail(PIL2GL_EINVAL, "op = %u: 0 batch_inverse, 1 gprod, 2 gsum, 3 batch_inverse in place", op);
    const bnscan::Plan p = bnscan::plan(n, op == bnscan::OP_BATCH_INVERSE_IN_PLACE);
    outInfo[0] = p.lv[0].L; outInfo[1] = (uint32_t)p.lv[0].S; outInfo[2] = p.nLevels; outInfo[3] = bnscan::THREADS;
    outInfo[4] = bnscan::THREADS;                    // segments per workgroup: a lane each
    *scratchBytes = n ? bnscan::scratch_bytes(p) : 0;
    return PIL2GL_OK;
}

int pil2gl_bn128_batch_inverse_dev(const uint64_t *src, uint64_t srcStride, uint64_t n, uint64_t *dst, uint64_t dstStride, void *stream) {
    P2_TRY(check_inverse(src, srcStride, n, dst, dstStride));
    if (n == 0) return PIL2GL_OK;
    P2_TRY(ensure_init());
    P2_TRY(check_aligned16({ src, dst }));
    return run(bnscan::OP_BATCH_INVERSE, nullptr, 0, nullptr, src, srcStride, n, dst, dstStride, as_stream(stream));
}

int pil2gl_bn128_gprod_dev(const uint64_t *num, uint64_t numStride, const uint64_t *den, uint64_t denStride, uint64_t n,
                           uint64_t *out, uint64_t outStride, void *stream) {
    P2_TRY(check_gprod(num, numStride, den, denStride, n, out, outStride));
    if (n == 0) return PIL2GL_OK;
    P2_TRY(ensure_init());
    P2_TRY(check_aligned16({ num, den, out }));
    return run(bnscan::OP_GPROD, num, numStride, nullptr, den, denStride, n, out, outStride, as_stream(stream));
}

int pil2gl_bn128_gsum_dev(const uint64_t hostNum[4], const uint64_t *den, uint64_t denStride, uint64_t n,
                          uint64_t *out, uint64_t outStride, void *stream) {
    P2_TRY(check_gsum(hostNum, den, denStride, n, out, outStride));
    if (n == 0) return PIL2GL_OK;
    P2_TRY(ensure_init());
    P2_TRY(check_aligned16({ den, out }));
    return run(bnscan::OP_GSUM, nullptr, 0, hostNum, den, denStride, n, out, outStride, as_stream(stream));
}

int pil2gl_bn128_gsum_col_dev(const uint64_t *num, uint64_t numStride, const uint64_t *den, uint64_t denStride, uint64_t n,
                              uint64_t *out, uint64_t outStride, void *stream) {
    P2_TRY(check_gprod(num, numStride, den, denStride, n, out, outStride));
    if (n == 0) return PIL2GL_OK;
    P2_TRY(ensure_init());
    P2_TRY(check_aligned16({ num, den, out }));
    return run(bnscan::OP_GSUM, num, numStride, nullptr, den, denStride, n, out, outStride, as_stream(stream));
}

int pil2gl_bn128_batch_inverse(const uint64_t *src, uint64_t srcStride, uint64_t n, uint64_t *dst, uint64_t dstStride) {
    P2_TRY(check_inverse(src, srcStride, n, dst, dstStride));
    if (n == 0) return PIL2GL_OK;
    return run_host(bnscan::OP_BATCH_INVERSE, nullptr, 0, nullptr, src, srcStride, n, dst, dstStride);
}

int pil2gl_bn128_gprod(const uint64_t *num, uint64_t numStride, const uint64_t *den, uint64_t denStride, uint64_t n,
                       uint64_t *out, uint64_t outStride) {
    P2_TRY(check_gprod(num, numStride, den, denStride, n, out, outStride));
    if (n == 0) return PIL2GL_OK;
    return run_host(bnscan::OP_GPROD, num, numStride, nullptr, den, denStride, n, out, outStride);
}

int pil2gl_bn128_gsum(const uint64_t hostNum[4], const uint64_t *den, uint64_t denStride, uint64_t n, uint64_t *out, uint64_t outStride) {
    P2_TRY(check_gsum(hostNum, den, denStride, n, out, outStride));
    if (n == 0) return PIL2GL_OK;
    return run_host(bnscan::OP_GSUM, nullptr, 0, hostNum, den, denStride, n, out, outStride);
}

int pil2gl_bn128_gsum_col(const uint64_t *num, uint64_t numStride, const uint64_t *den, uint64_t denStride, uint64_t n,
                          uint64_t *out, uint64_t outStride) {
    P2_TRY(check_gprod(num, numStride, den, denStride, n, out, outStride));
    if (n == 0) return PIL2GL_OK;
    return run_host(bnscan::OP_GSUM, num, numStride, nullptr, den, denStride, n, out, outStride);
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------------------------------
// The lookup grand sum over Fr (include/pil2gl.h states it):  s[i] = s[i-1] + sum_u coef_u w_u[i] / D_u[i],
//   D_u[i] = ((..(v_0 alpha + v_1) alpha .. + v_{k-1}) alpha + busId_u) + beta.
// One compress kernel, a lane a row, folds the row's terms into ONE fraction N / D (N <- N D_u + coef_u w_u D, D <- D D_u; a zero D_u is
// left out of both, so D is never zero) and writes D and N into the working buffer; then the operators above as they are:
// inverse_launch(MODE_COLUMN) leaves N / D in the output column -- its prefixes live there meanwhile, which is why N cannot -- and
// scan_launch<true> sums in place.  One Fermat ladder a call.  Products a row: nTerms (k + 4) in the compress (k Horner steps, coef w, three
// for the fold; a NULL numerator column saves one), then gsum_col's 5.
// The term table is a kernel argument read with wave-uniform indices: no copy to the device, nothing in a private segment.
namespace {

using tupleside::FrField;
typedef FrField::Elem FrE;

struct FrLogupTerm { tupleside::Side<FrField> s; u32 k; FrE coef, bus; };
struct FrLogupJob {
    FrLogupTerm t[logupplan::MAX_TERMS];
    FrE alpha, beta, one;                            // one: 1 in Montgomery form
    u32 nTerms;
    u64 n;
    FrField::Mem *D, *N;                             // dense, n elements each
};

// one f term of row i folded into the row's fraction N / D
__device__ __forceinline__ void fr_logup_fold(const FrLogupTerm &T, u64 i, const FrE &alpha, const FrE &beta, FrE &N, FrE &D) {
    FrE d = tupleside::elem_of(T.s, i, 0);
    for (u32 j = 1; j < T.k; j++) d = FrField::add(FrField::mul(d, alpha), tupleside::elem_of(T.s, i, j));
    d = FrField::add(FrField::add(FrField::mul(d, alpha), FrField::reduce(T.bus)), beta);
    if (bn::is_zero(d.v)) return;                     // a zero D_u: the term adds 0 and is left out of the product
    FrE c = FrField::reduce(T.coef);
    if (T.s.sel) c = FrField::mul(FrField::load(T.s.sel, i * T.s.selStride + T.s.selCol), c);
    N = FrField::add(FrField::mul(N, d), FrField::mul(D, c));
    D = FrField::mul(D, d);
}

__global__ void __launch_bounds__(smapplan::THREADS) bn_logup_compress_kernel(const FrLogupJob J) {
    const FrE alpha = FrField::reduce(J.alpha), beta = FrField::reduce(J.beta);
    for (u64 i = (u64)blockIdx.x * smapplan::THREADS + threadIdx.x; i < J.n; i += (u64)gridDim.x * smapplan::THREADS) {
        FrE N{}, D = J.one;
        for (u32 u = 0; u < J.nTerms; u++) fr_logup_fold(J.t[u], i, alpha, beta, N, D);
        FrField::store(J.D, i, D);
        FrField::store(J.N, i, N);
    }
}

// a term's table entry from the entry's term, its pointers the device's
void fill_term(FrLogupTerm &T, const pil2gl_logup_term &t) {
    T.s = tupleside::device_side<FrField>(t.side, (u32)t.k);
    T.k = (u32)t.k;
    bnp::bn_limbs(t.coef, T.coef.v);
    bnp::bn_limbs(t.busId, T.bus.v);
}

// every launch of a call, on st; the arguments have passed logupplan::check_call() and n > 0, the pointers are the device's
int bn_logup_launch(const pil2gl_logup_term *terms, u32 nTerms, const u64 *alpha, const u64 *beta, u64 *out, u64 outStride, u64 outCol, u64 n, hipStream_t st) {
    const bnscan::Plan p = bnscan::plan(n, false);
    u64 *d;
    P2_TRY(scratch(SCR_BN_SCAN, 4 * p.elems + 8 * n, &d));        // the plan's levels, then D and N
    FrLogupJob J{};
    for (u32 u = 0; u < nTerms; u++) fill_term(J.t[u], terms[u]);
    bnp::bn_limbs(alpha, J.alpha.v); bnp::bn_limbs(beta, J.beta.v); bnp::bn_limbs(bnp::bn_mont_one().w, J.one.v);
    J.nTerms = nTerms; J.n = n;
    J.D = (FrField::Mem *)(d + 4 * p.elems); J.N = J.D + n;
    bn_logup_compress_kernel<<<smapplan::blocks(n), smapplan::THREADS, 0, st>>>(J);
    KERNEL_CHECK();
    uint4 *base = (uint4 *)d, *y = (uint4 *)(out + 4 * outCol);
    P2_TRY(inverse_launch(p, base, (const uint4 *)J.D, 1, y, outStride, y, outStride, MODE_COLUMN, (const uint4 *)J.N, 1, Elem{}, st));
    return scan_launch<true>(p, base, y, outStride, st);
}

int bn_logup_check(const pil2gl_logup_term *terms, u64 nTerms, const u64 *alpha, const u64 *beta, const u64 *out, u64 outStride, u64 outCol, u64 n, bool dev) {
    char why[96];
    if (const char *msg = logupplan::check_call(terms, nTerms, alpha, beta, out, outStride, outCol, n, 4, dev, why)) return fail(PIL2GL_EINVAL, "%s", msg);
    return PIL2GL_OK;
}

}  // namespace

extern "C" {

int pil2gl_bn128_logup_sum_dev(const pil2gl_logup_term *hostTerms, uint64_t nTerms, const uint64_t *hostAlpha, const uint64_t *hostBeta,
                               uint64_t *out, uint64_t outStride, uint64_t outCol, uint64_t n, void *stream) {
    P2_TRY(bn_logup_check(hostTerms, nTerms, hostAlpha, hostBeta, out, outStride, outCol, n, true));
    if (!n) return PIL2GL_OK;
    P2_TRY(ensure_init());
    return bn_logup_launch(hostTerms, (u32)nTerms, hostAlpha, hostBeta, out, outStride, outCol, n, as_stream(stream));
}

// host matrices, each staged up to the last element touched; out's matrix goes up as it is and comes back with the column written
int pil2gl_bn128_logup_sum(const pil2gl_logup_term *hostTerms, uint64_t nTerms, const uint64_t *hostAlpha, const uint64_t *hostBeta,
                           uint64_t *hostOut, uint64_t outStride, uint64_t outCol, uint64_t n) {
    P2_TRY(bn_logup_check(hostTerms, nTerms, hostAlpha, hostBeta, hostOut, outStride, outCol, n, false));
    if (!n) return PIL2GL_OK;
    pil2gl_logup_term terms[logupplan::MAX_TERMS];
    const u64 outWords = tupleside::span_bytes(n, outStride, outCol, 4) / 8;
    u64 total = smapplan::pad16(outWords);
    for (u64 u = 0; u < nTerms; u++) { terms[u] = hostTerms[u]; total += tupleside::staged_words(terms[u].side, n, terms[u].k, 4); }
    Stage s(total);
    P2_TRY(s.rc());
    for (u64 u = 0; u < nTerms; u++) tupleside::stage_side(s, terms[u].side, n, terms[u].k, 4);
    u64 *dOut = (u64 *)s.put(hostOut, outWords);
    P2_TRY(s.rc());
    P2_TRY(bn_logup_launch(terms, (u32)nTerms, hostAlpha, hostBeta, dOut, outStride, outCol, n, 0));
    return s.get(hostOut, dOut, outWords);
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------------------------------
// The range-check grand sum over Fr (include/pil2gl.h states it): the lookup grand sum above with the table side of a range as numbers,
//   E_r[i] = field(lo_r + (i - row0_r)) alpha + busId_r + beta   inside the window row0_r <= i < row0_r + size_r, the range adding 0 outside.
// One compress kernel, a lane a row, writing D and N as bn_logup_compress_kernel does (its f terms through the same fr_logup_fold), then
// inverse_launch(MODE_COLUMN) and scan_launch<true> as they are.  field(lo + j) is a PLAIN integer mod r: lo mod r from the host (normal
// form, range_mult_plan.h) plus j, one modular addition.  The host also makes alpha R^2 (h_to_mont of alpha's Montgomery words, canonical
// for any pattern), so that ONE Montgomery product of it with the plain integer is alpha field(lo + j) in Montgomery form.  Products a
// range-row inside the window: that one, coef m, three for the fold -- 5, what the block above's k = 1 term takes; what is saved is t's
// 32-byte load and its reduction.  Outside the window a range costs no product and no load.
namespace {

struct FrRangeTerm { const FrField::Mem *m; u64 stride, col, row0, end; FrE lo, coef, bus; };      // lo: lo mod r, normal form
struct FrRangeJob {
    FrLogupTerm t[rangesumplan::MAX_F];
    FrRangeTerm r[rangesumplan::MAX_RANGES];
    FrE alpha, alphaR2, beta, one;                   // alphaR2: alpha 2^512 mod r; one: 1 in Montgomery form
    u32 nTerms, nRanges;
    u64 n;
    FrField::Mem *D, *N;                             // dense, n elements each
};

// one range of row i folded into the row's fraction N / D: the loop body of bn_range_compress_kernel below as a function, for the clustered
// sum's kernels (that kernel keeps its own copy: calling this one there moved its register count; a fix here belongs there too)
__device__ __forceinline__ void fr_range_fold(const FrRangeTerm &T, u64 i, const FrE &alphaR2, const FrE &beta, FrE &N, FrE &D) {
    if (i < T.row0 || i >= T.end) return;             // outside the window: adds 0, m is not read.  end <= n
    FrE v = { { (u32)(i - T.row0), 0, 0, 0, 0, 0, 0, 0 } };                        // j < 2^28
    v = FrField::add(v, T.lo);                        // field(lo + j), both below r
    FrE d = FrField::add(FrField::add(FrField::mul(alphaR2, v), FrField::reduce(T.bus)), beta);
    if (bn::is_zero(d.v)) return;                     // a zero E_r: the range adds 0 and is left out of the product
    const FrE c = FrField::mul(FrField::load(T.m, i * T.stride + T.col), FrField::reduce(T.coef));
    N = FrField::add(FrField::mul(N, d), FrField::mul(D, c));
    D = FrField::mul(D, d);
}

__global__ void __launch_bounds__(smapplan::THREADS) bn_range_compress_kernel(const FrRangeJob J) {
    const FrE alpha = FrField::reduce(J.alpha), beta = FrField::reduce(J.beta);
    for (u64 i = (u64)blockIdx.x * smapplan::THREADS + threadIdx.x; i < J.n; i += (u64)gridDim.x * smapplan::THREADS) {
        FrE N{}, D = J.one;
        for (u32 u = 0; u < J.nTerms; u++) fr_logup_fold(J.t[u], i, alpha, beta, N, D);
        for (u32 r = 0; r < J.nRanges; r++) {           // fr_range_fold above is this body as a function: a fix here belongs there too
            const FrRangeTerm &T = J.r[r];
            if (i < T.row0 || i >= T.end) continue;   // outside the window: adds 0, m is not read.  end <= n
            FrE v = { { (u32)(i - T.row0), 0, 0, 0, 0, 0, 0, 0 } };                // j < 2^28
            v = FrField::add(v, T.lo);                // field(lo + j), both below r
            FrE d = FrField::add(FrField::add(FrField::mul(J.alphaR2, v), FrField::reduce(T.bus)), beta);
            if (bn::is_zero(d.v)) continue;           // a zero E_r: the range adds 0 and is left out of the product
            const FrE c = FrField::mul(FrField::load(T.m, i * T.stride + T.col), FrField::reduce(T.coef));
            N = FrField::add(FrField::mul(N, d), FrField::mul(D, c));
            D = FrField::mul(D, d);
        }
        FrField::store(J.D, i, D);
        FrField::store(J.N, i, N);
    }
}

// a job's tables and constants from the entry's terms and ranges, their pointers the device's
void fill_range_job(FrRangeJob &J, const pil2gl_logup_term *terms, u32 nF, const pil2gl_range_term *ranges, u32 nR, const u64 *alpha, const u64 *beta, u64 n) {
    for (u32 u = 0; u < nF; u++) fill_term(J.t[u], terms[u]);
    for (u32 r = 0; r < nR; r++) {
        const pil2gl_range_term &R = ranges[r];
        FrRangeTerm &T = J.r[r];
        T.m = (const FrField::Mem *)R.m; T.stride = R.mStride; T.col = R.mCol; T.row0 = R.row0; T.end = R.row0 + R.size;
        u64 lo[4];
        rangemultplan::lo_mod_r(R.lo, lo);
        bnp::bn_limbs(lo, T.lo.v); bnp::bn_limbs(R.coef, T.coef.v); bnp::bn_limbs(R.busId, T.bus.v);
    }
    const bnp::U256 a = { { alpha[0], alpha[1], alpha[2], alpha[3] } };
    bnp::bn_limbs(alpha, J.alpha.v); bnp::bn_limbs(bnp::h_to_mont(a).w, J.alphaR2.v); bnp::bn_limbs(beta, J.beta.v); bnp::bn_limbs(bnp::bn_mont_one().w, J.one.v);
    J.nTerms = nF; J.nRanges = nR; J.n = n;
}

// every launch of a call, on st; the arguments have passed rangesumplan::check_call() and n > 0, the pointers are the device's
int bn_range_sum_launch(const pil2gl_logup_term *terms, u32 nF, const pil2gl_range_term *ranges, u32 nR, const u64 *alpha, const u64 *beta, u64 *out,
                        u64 outStride, u64 outCol, u64 n, hipStream_t st) {
    const bnscan::Plan p = bnscan::plan(n, false);
    u64 *d;
    P2_TRY(scratch(SCR_BN_SCAN, 4 * p.elems + 8 * n, &d));        // the plan's levels, then D and N
    FrRangeJob J{};
    fill_range_job(J, terms, nF, ranges, nR, alpha, beta, n);
    J.D = (FrField::Mem *)(d + 4 * p.elems); J.N = J.D + n;
    bn_range_compress_kernel<<<smapplan::blocks(n), smapplan::THREADS, 0, st>>>(J);
    KERNEL_CHECK();
    uint4 *base = (uint4 *)d, *y = (uint4 *)(out + 4 * outCol);
    P2_TRY(inverse_launch(p, base, (const uint4 *)J.D, 1, y, outStride, y, outStride, MODE_COLUMN, (const uint4 *)J.N, 1, Elem{}, st));
    return scan_launch<true>(p, base, y, outStride, st);
}

int bn_range_sum_check(const pil2gl_logup_term *terms, u64 nF, const pil2gl_range_term *ranges, u64 nR, const u64 *alpha, const u64 *beta, const u64 *out,
                       u64 outStride, u64 outCol, u64 n, bool dev) {
    char why[96];
    if (const char *msg = rangesumplan::check_call(terms, nF, ranges, nR, alpha, beta, out, outStride, outCol, n, 4, dev, why)) return fail(PIL2GL_EINVAL, "%s", msg);
    return PIL2GL_OK;
}

}  // namespace

extern "C" {

int pil2gl_bn128_range_sum_dev(const pil2gl_logup_term *hostTerms, uint64_t nF, const pil2gl_range_term *hostRanges, uint64_t nR, const uint64_t *hostAlpha,
                               const uint64_t *hostBeta, uint64_t *out, uint64_t outStride, uint64_t outCol, uint64_t n, void *stream) {
    P2_TRY(bn_range_sum_check(hostTerms, nF, hostRanges, nR, hostAlpha, hostBeta, out, outStride, outCol, n, true));
    if (!n) return PIL2GL_OK;
    P2_TRY(ensure_init());
    return bn_range_sum_launch(hostTerms, (u32)nF, hostRanges, (u32)nR, hostAlpha, hostBeta, out, outStride, outCol, n, as_stream(stream));
}

// host matrices, each staged up to the last element touched (an m up to its window's last row); out's matrix goes up as it is and comes back
// with the column written
int pil2gl_bn128_range_sum(const pil2gl_logup_term *hostTerms, uint64_t nF, const pil2gl_range_term *hostRanges, uint64_t nR, const uint64_t *hostAlpha,
                           const uint64_t *hostBeta, uint64_t *hostOut, uint64_t outStride, uint64_t outCol, uint64_t n) {
    P2_TRY(bn_range_sum_check(hostTerms, nF, hostRanges, nR, hostAlpha, hostBeta, hostOut, outStride, outCol, n, false));
    if (!n) return PIL2GL_OK;
    pil2gl_logup_term terms[rangesumplan::MAX_F];
    pil2gl_range_term ranges[rangesumplan::MAX_RANGES];
    const u64 outWords = tupleside::span_bytes(n, outStride, outCol, 4) / 8;
    u64 total = smapplan::pad16(outWords);
    for (u64 u = 0; u < nF; u++) { terms[u] = hostTerms[u]; total += tupleside::staged_words(terms[u].side, n, terms[u].k, 4); }
    for (u64 r = 0; r < nR; r++) { ranges[r] = hostRanges[r]; total += smapplan::pad16(rangesumplan::m_words(ranges[r], 4)); }
    Stage s(total);
    P2_TRY(s.rc());
    for (u64 u = 0; u < nF; u++) tupleside::stage_side(s, terms[u].side, n, terms[u].k, 4);
    for (u64 r = 0; r < nR; r++) {
        const u64 w = rangesumplan::m_words(ranges[r], 4);
        ranges[r].m = s.put(ranges[r].m, w); s.take(smapplan::pad16(w) - w);
    }
    u64 *dOut = (u64 *)s.put(hostOut, outWords);
    P2_TRY(s.rc());
    P2_TRY(bn_range_sum_launch(terms, (u32)nF, ranges, (u32)nR, hostAlpha, hostBeta, dOut, outStride, outCol, n, 0));
    return s.get(hostOut, dOut, outWords);
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------------------------------
// The clustered logUp sum over Fr (include/pil2gl.h states it): the two sums above with the terms gathered into clusters, im_c[i] the part
// of cluster c in row i's increment, written as a column of its own beside s.  Working memory must not grow with nIm, so no D_c column is
// written: ONE product column P and one inversion a call,
//   bn_cluster_prod_kernel     a lane a row: P[i] = the product of the row's non-zero denominators over every cluster and the DIRECT part
//                              (the folds above with the numerator unused), 32 bytes a row into the working buffer
//   inverse_launch(MODE_NONE)  1 / P into the output column, its prefixes there meanwhile; one Fermat ladder a call
//   bn_cluster_refold_kernel   a lane a row REFOLDS the row, group by group (the clusters, then the DIRECT part if there is one): group g
//                              gives N_g / D_g; going up it keeps X_g = N_g prod_{h < g} D_h and D_g in registers, going down r = (1 / P)
//                              prod_{h > g} D_h = 1 / prod_{h <= g} D_h, so that X_g r = N_g / D_g: 1 / D_g peeled off 1 / P with the
//                              prefix and the suffix products, 4 products a group.  Writes every im_c and the row's increment into out
//   scan_launch<true>          sums out in place
// The refold costs k + 4 products a term again, cheaper than the 64 bytes a cluster-row that D_c and N_c columns would be written and read
// with.  The per-group registers are indexed by compile-time constants (each_group) and stay out of the private segment.
// Safety: nothing read from a matrix is used as an address; a lane's row is below n; the group of a term is a wave-uniform kernel-argument read.
namespace {

using logupclusterplan::MAX_GROUPS;

struct FrImCol { FrField::Mem *base; u64 stride, col; };
struct FrClusterJob : FrRangeJob {                   // D: the product column P; N unused
    FrImCol im[logupclusterplan::MAX_IM];
    u32 group[logupplan::MAX_TERMS];                 // the group of term u (f terms, then ranges): its cluster, or nIm for a DIRECT term
    u32 nIm, nGroups;                                // nGroups: nIm, + 1 with a DIRECT term.  Every group has a term
    FrField::Mem *out; u64 outStride, outCol;
};

template <class Fn, int... G> __device__ __forceinline__ void each_group(Fn f, std::integer_sequence<int, G...>) { (f(std::integral_constant<int, G>{}), ...); }
template <class Fn> __device__ __forceinline__ void each_group(Fn f) { each_group(f, std::make_integer_sequence<int, (int)MAX_GROUPS>{}); }

__global__ void __launch_bounds__(smapplan::THREADS) bn_cluster_prod_kernel(const FrClusterJob J) {
    const FrE alpha = FrField::reduce(J.alpha), beta = FrField::reduce(J.beta);
    for (u64 i = (u64)blockIdx.x * smapplan::THREADS + threadIdx.x; i < J.n; i += (u64)gridDim.x * smapplan::THREADS) {
        FrE N{}, D = J.one;
        for (u32 u = 0; u < J.nTerms; u++) fr_logup_fold(J.t[u], i, alpha, beta, N, D);
        for (u32 r = 0; r < J.nRanges; r++) fr_range_fold(J.r[r], i, J.alphaR2, beta, N, D);
        FrField::store(J.D, i, D);
    }
}

__global__ void __launch_bounds__(smapplan::THREADS) bn_cluster_refold_kernel(const FrClusterJob J) {
    const FrE alpha = FrField::reduce(J.alpha), beta = FrField::reduce(J.beta);
    for (u64 i = (u64)blockIdx.x * smapplan::THREADS + threadIdx.x; i < J.n; i += (u64)gridDim.x * smapplan::THREADS) {
        u32 X[MAX_GROUPS][8] = {}, Dg[MAX_GROUPS][8] = {};      // written and read with selects on the wave-uniform g, never with an index
        FrE pre = J.one;                              // the product of the groups' D below g
        for (u32 g = 0; g < J.nGroups; g++) {
            FrE N{}, D = J.one;                       // every group anew
            for (u32 u = 0; u < J.nTerms; u++) if (J.group[u] == g) fr_logup_fold(J.t[u], i, alpha, beta, N, D);
            for (u32 r = 0; r < J.nRanges; r++) if (J.group[J.nTerms + r] == g) fr_range_fold(J.r[r], i, J.alphaR2, beta, N, D);
            const FrE x = FrField::mul(N, pre);
            each_group([&](auto G) {
#pragma unroll
                for (int l = 0; l < 8; l++) { X[G][l] = G == g ? x.v[l] : X[G][l]; Dg[G][l] = G == g ? D.v[l] : Dg[G][l]; }
            });
            pre = FrField::mul(pre, D);
        }
        FrE r = FrField::load(J.out, i * J.outStride + J.outCol);                // 1 / P[i]
        FrE inc{};
        for (u32 g = J.nGroups; g-- > 0;) {
            FrE x{}, d{};
            each_group([&](auto G) {
#pragma unroll
                for (int l = 0; l < 8; l++) { x.v[l] = G == g ? X[G][l] : x.v[l]; d.v[l] = G == g ? Dg[G][l] : d.v[l]; }
            });
            const FrE v = FrField::mul(x, r);         // N_g / D_g: r = 1 / (the product of the groups' D up to g)
            r = FrField::mul(r, d);
            if (g < J.nIm) FrField::store(J.im[g].base, i * J.im[g].stride + J.im[g].col, v);
            inc = FrField::add(inc, v);
        }
        FrField::store(J.out, i * J.outStride + J.outCol, inc);
    }
}

// every launch of a call, on st; the arguments have passed logupclusterplan::check_call() and n > 0, the pointers are the device's
int bn_cluster_launch(const pil2gl_logup_term *terms, u32 nF, const pil2gl_range_term *ranges, u32 nR, const u64 *cluster, const pil2gl_logup_im_col *im,
                      u32 nIm, const u64 *alpha, const u64 *beta, u64 *out, u64 outStride, u64 outCol, u64 n, hipStream_t st) {
    const bnscan::Plan p = bnscan::plan(n, false);
    u64 *d;
    P2_TRY(scratch(SCR_BN_SCAN, 4 * p.elems + 4 * n, &d));        // the plan's levels, then P
    FrClusterJob J{};
    fill_range_job(J, terms, nF, ranges, nR, alpha, beta, n);
    J.D = (FrField::Mem *)(d + 4 * p.elems);
    J.nIm = J.nGroups = nIm;
    for (u32 u = 0; u < nF + nR; u++) {
        J.group[u] = cluster[u] == logupclusterplan::DIRECT ? nIm : (u32)cluster[u];
        if (J.group[u] == nIm) J.nGroups = nIm + 1;
    }
    for (u32 c = 0; c < nIm; c++) J.im[c] = FrImCol{ (FrField::Mem *)im[c].base, im[c].stride, im[c].col };
    J.out = (FrField::Mem *)out; J.outStride = outStride; J.outCol = outCol;
    bn_cluster_prod_kernel<<<smapplan::blocks(n), smapplan::THREADS, 0, st>>>(J);
    KERNEL_CHECK();
    uint4 *base = (uint4 *)d, *y = (uint4 *)(out + 4 * outCol);
    P2_TRY(inverse_launch(p, base, (const uint4 *)J.D, 1, y, outStride, y, outStride, MODE_NONE, nullptr, 0, Elem{}, st));
    bn_cluster_refold_kernel<<<smapplan::blocks(n), smapplan::THREADS, 0, st>>>(J);
    KERNEL_CHECK();
    return scan_launch<true>(p, base, y, outStride, st);
}

int bn_cluster_check(const pil2gl_logup_term *terms, u64 nF, const pil2gl_range_term *ranges, u64 nR, const u64 *cluster, const pil2gl_logup_im_col *im, u64 nIm,
                     const u64 *alpha, const u64 *beta, const u64 *out, u64 outStride, u64 outCol, u64 n, bool dev) {
    char why[96];
    if (const char *msg = logupclusterplan::check_call(terms, nF, ranges, nR, cluster, im, nIm, alpha, beta, out, outStride, outCol, n, 4, dev, why))
        return fail(PIL2GL_EINVAL, "%s", msg);
    return PIL2GL_OK;
}

}  // namespace

extern "C" {

int pil2gl_bn128_logup_cluster_dev(const pil2gl_logup_term *hostTerms, uint64_t nF, const pil2gl_range_term *hostRanges, uint64_t nR, const uint64_t *hostCluster,
                                   const pil2gl_logup_im_col *hostIm, uint64_t nIm, const uint64_t *hostAlpha, const uint64_t *hostBeta, uint64_t *out,
                                   uint64_t outStride, uint64_t outCol, uint64_t n, void *stream) {
    P2_TRY(bn_cluster_check(hostTerms, nF, hostRanges, nR, hostCluster, hostIm, nIm, hostAlpha, hostBeta, out, outStride, outCol, n, true));
    if (!n) return PIL2GL_OK;
    P2_TRY(ensure_init());
    return bn_cluster_launch(hostTerms, (u32)nF, hostRanges, (u32)nR, hostCluster, hostIm, (u32)nIm, hostAlpha, hostBeta, out, outStride, outCol, n, as_stream(stream));
}

// host matrices: logupclusterplan::host_form stages them, the read ones as range_sum's, every distinct output matrix as it is
int pil2gl_bn128_logup_cluster(const pil2gl_logup_term *hostTerms, uint64_t nF, const pil2gl_range_term *hostRanges, uint64_t nR, const uint64_t *hostCluster,
                               const pil2gl_logup_im_col *hostIm, uint64_t nIm, const uint64_t *hostAlpha, const uint64_t *hostBeta, uint64_t *hostOut,
                               uint64_t outStride, uint64_t outCol, uint64_t n) {
    P2_TRY(bn_cluster_check(hostTerms, nF, hostRanges, nR, hostCluster, hostIm, nIm, hostAlpha, hostBeta, hostOut, outStride, outCol, n, false));
    if (!n) return PIL2GL_OK;
    return logupclusterplan::host_form<Stage>(hostTerms, nF, hostRanges, nR, hostIm, nIm, hostOut, outStride, outCol, n, 4,
        [&](const pil2gl_logup_term *t, const pil2gl_range_term *r, const pil2gl_logup_im_col *im, u64 *dOut) {
            return bn_cluster_launch(t, (u32)nF, r, (u32)nR, hostCluster, im, (u32)nIm, hostAlpha, hostBeta, dOut, outStride, outCol, n, 0);
        });
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------------------------------
// The grand product of a permutation or a connection over Fr (include/pil2gl.h states it):  z[0] = 1, z[i] = z[i-1] R[i-1],
//   R = prod_{num terms} D_u / prod_{den terms} D_u,  D_u = B_u + idCoef_u id_u + gamma,  B_u = H_u or (H_u - beta) sel_u + beta,
//   H_u = (..(v_0 alpha + v_1) alpha ..) alpha + v_{k-1}.
// One compress kernel, a lane a row, multiplies the row's terms into N and D and writes both into the working buffer; then gprod's own
// operators as they are: inverse_launch(MODE_COLUMN) leaves N / D in the output column, a zero D giving 0, and scan_launch<false> is the
// exclusive running product in place.  One Fermat ladder a call.  Products a row: a term's k (k - 1 Horner steps and the one into N or
// D), one more for a selector and for an id column each; then gprod's 7.
// The packed term table (grand_prod_plan.h) is a kernel argument read with wave-uniform indices.
namespace {

typedef grandprodplan::Term<4> FrGprodTerm;
typedef grandprodplan::FrJob FrGprodJob;

__device__ __forceinline__ FrE fr_of(const uint64_t w[4]) {
    FrE x;
#pragma unroll
    for (int i = 0; i < 4; i++) { x.v[2 * i] = (u32)w[i]; x.v[2 * i + 1] = (u32)(w[i] >> 32); }
    return FrField::reduce(x);
}
__device__ __forceinline__ FrE fr_at(const void *m, u64 at) { return FrField::reduce(FrField::load((const FrField::Mem *)m, at)); }

__global__ void __launch_bounds__(smapplan::THREADS) bn_gprod_compress_kernel(const FrGprodJob J, const FrE one, FrField::Mem *__restrict__ D, FrField::Mem *__restrict__ N) {
    const FrE alpha = fr_of(J.apow[0]), beta = fr_of(J.beta), gamma = fr_of(J.gamma);
    for (u64 i = (u64)blockIdx.x * smapplan::THREADS + threadIdx.x; i < J.n; i += (u64)gridDim.x * smapplan::THREADS) {
        FrE num = one, den = one;
        for (u32 u = 0; u < J.nTerms; u++) {
            const FrGprodTerm &T = J.t[u];
            const u64 row = i * T.stride;
            FrE d = fr_at(T.base, row + J.cols[T.start]);
            for (u32 j = 1; j < T.k; j++) d = FrField::add(FrField::mul(d, alpha), fr_at(T.base, row + J.cols[T.start + j]));
            if (T.sel) {
                bn::fr_sub(d.v, beta.v);
                d = FrField::add(FrField::mul(d, fr_at(T.sel, i * T.selStride + T.selCol)), beta);
            }
            if (T.id) d = FrField::add(d, FrField::mul(fr_of(T.idCoef), fr_at(T.id, i * T.idStride + T.idCol)));
            d = FrField::add(d, gamma);
            if (T.den) den = FrField::mul(den, d);
            else num = FrField::mul(num, d);
        }
        FrField::store(D, i, den);
        FrField::store(N, i, num);
    }
}

// every launch of a call, on st; the arguments have passed grandprodplan::check_call() and n > 0, the pointers are the device's
int bn_gprod_fold_launch(const pil2gl_grand_prod_term *terms, u32 nTerms, const u64 *alpha, const u64 *beta, const u64 *gamma, u64 *out, u64 outStride,
                         u64 outCol, u64 n, hipStream_t st) {
    const bnscan::Plan p = bnscan::plan(n, false);
    u64 *d;
    P2_TRY(scratch(SCR_BN_SCAN, 4 * p.elems + 8 * n, &d));        // the plan's levels, then D and N
    FrGprodJob J{};
    const u64 (*a)[4] = (const u64 (*)[4])alpha;
    grandprodplan::pack(terms, nTerms, a, beta, gamma, n, J);
    FrE one;
    bnp::bn_limbs(bnp::bn_mont_one().w, one.v);
    FrField::Mem *D = (FrField::Mem *)(d + 4 * p.elems), *N = D + n;
    bn_gprod_compress_kernel<<<smapplan::blocks(n), smapplan::THREADS, 0, st>>>(J, one, D, N);
    KERNEL_CHECK();
    uint4 *base = (uint4 *)d, *y = (uint4 *)(out + 4 * outCol);
    P2_TRY(inverse_launch(p, base, (const uint4 *)D, 1, y, outStride, y, outStride, MODE_COLUMN, (const uint4 *)N, 1, Elem{}, st));
    return scan_launch<false>(p, base, y, outStride, st);
}

int bn_gprod_fold_check(const pil2gl_grand_prod_term *terms, u64 nTerms, const u64 *alpha, const u64 *beta, const u64 *gamma, const u64 *out, u64 outStride,
                        u64 outCol, u64 n, bool dev) {
    char why[96];
    if (const char *msg = grandprodplan::check_call(terms, nTerms, alpha, beta, gamma, out, outStride, outCol, n, 4, dev, why)) return fail(PIL2GL_EINVAL, "%s", msg);
    return PIL2GL_OK;
}

}  // namespace

extern "C" {

int pil2gl_bn128_grand_prod_dev(const pil2gl_grand_prod_term *hostTerms, uint64_t nTerms, const uint64_t *hostAlpha, const uint64_t *hostBeta,
                                const uint64_t *hostGamma, uint64_t *out, uint64_t outStride, uint64_t outCol, uint64_t n, void *stream) {
    P2_TRY(bn_gprod_fold_check(hostTerms, nTerms, hostAlpha, hostBeta, hostGamma, out, outStride, outCol, n, true));
    if (!n) return PIL2GL_OK;
    P2_TRY(ensure_init());
    return bn_gprod_fold_launch(hostTerms, (u32)nTerms, hostAlpha, hostBeta, hostGamma, out, outStride, outCol, n, as_stream(stream));
}

// host matrices, each staged up to the last element touched; out's matrix goes up as it is and comes back with the column written
int pil2gl_bn128_grand_prod(const pil2gl_grand_prod_term *hostTerms, uint64_t nTerms, const uint64_t *hostAlpha, const uint64_t *hostBeta,
                            const uint64_t *hostGamma, uint64_t *hostOut, uint64_t outStride, uint64_t outCol, uint64_t n) {
    P2_TRY(bn_gprod_fold_check(hostTerms, nTerms, hostAlpha, hostBeta, hostGamma, hostOut, outStride, outCol, n, false));
    if (!n) return PIL2GL_OK;
    pil2gl_grand_prod_term terms[grandprodplan::MAX_TERMS];
    const u64 outWords = tupleside::span_bytes(n, outStride, outCol, 4) / 8;
    u64 total = smapplan::pad16(outWords);
    for (u64 u = 0; u < nTerms; u++) {
        terms[u] = hostTerms[u];
        total += tupleside::staged_words(terms[u].side, n, terms[u].k, 4) + smapplan::pad16(grandprodplan::id_words(terms[u], n, 4));
    }
    Stage s(total);
    P2_TRY(s.rc());
    for (u64 u = 0; u < nTerms; u++) { tupleside::stage_side(s, terms[u].side, n, terms[u].k, 4); grandprodplan::stage_id(s, terms[u], n, 4); }
    u64 *dOut = (u64 *)s.put(hostOut, outWords);
    P2_TRY(s.rc());
    P2_TRY(bn_gprod_fold_launch(terms, (u32)nTerms, hostAlpha, hostBeta, hostGamma, dOut, outStride, outCol, n, 0));
    return s.get(hostOut, dOut, outWords);
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------------------------------
// The plookup argument of pil1 over Fr (include/pil2gl.h states it):
//   T = H_t or (H_t - beta) selT + beta,   F = H_f or (H_f - T) selF + T,   g = gamma (1 + delta),
//   num[i] = (F[i] + gamma) (T[i] + delta T[i+1] + g) (1 + delta),   den[i] = (h1[i] + delta h2[i] + g) (h2[i] + delta h1[i+1] + g),
//   z[0] = 1, z[i] = z[i-1] num[i-1] / den[i-1],   row n - 1's neighbour is row 0.
// The fold is one kernel, a lane a row, writing F and T as strided columns for bn128_h1h2.  The product is one compress kernel, a lane a
// row -- it makes T of its row and of the next from the trace, so t's tuple is read twice -- that writes num and den into the working
// buffer; then gprod's own operators as grand_prod above runs them.  g and 1 + delta are made by the kernel, once a lane.  Products a row:
// kF - 1 + 2 (kT - 1) Horner steps, one a selector (selT two), 2 + 3 + 3 for num and den; then gprod's 7.
namespace {

typedef plookupplan::FrJob FrPlJob;
typedef plookupplan::Side FrPlSide;
typedef plookupplan::Column FrPlColumn;

// H of the side's row i, blended towards `to` by the selector's value where there is one
__device__ __forceinline__ FrE fr_pl_side(const FrPlSide &S, u64 i, const FrE &alpha, const FrE &to) {
    const u64 row = i * S.stride;
    FrE d = fr_at(S.base, row + S.cols[0]);
    for (u32 j = 1; j < S.k; j++) d = FrField::add(FrField::mul(d, alpha), fr_at(S.base, row + S.cols[j]));
    if (S.sel) {
        bn::fr_sub(d.v, to.v);
        d = FrField::add(FrField::mul(d, fr_at(S.sel, i * S.selStride + S.selCol)), to);
    }
    return d;
}

__global__ void __launch_bounds__(smapplan::THREADS) bn_plookup_compress_kernel(const FrPlJob J, const FrE one, FrField::Mem *__restrict__ D, FrField::Mem *__restrict__ N) {
    const FrE alpha = fr_of(J.apow[0]), beta = fr_of(J.beta), gamma = fr_of(J.gamma), delta = fr_of(J.delta);
    const FrE opd = FrField::add(one, delta), g = FrField::mul(gamma, opd);
    for (u64 i = (u64)blockIdx.x * smapplan::THREADS + threadIdx.x; i < J.n; i += (u64)gridDim.x * smapplan::THREADS) {
        const u64 nx = i + 1 < J.n ? i + 1 : 0;                                // row n - 1's neighbour is row 0
        const FrE T = fr_pl_side(J.t, i, alpha, beta), Tn = fr_pl_side(J.t, nx, alpha, beta), F = fr_pl_side(J.f, i, alpha, T);
        FrE num = FrField::mul(FrField::add(F, gamma), FrField::add(FrField::add(T, FrField::mul(delta, Tn)), g));
        num = FrField::mul(num, opd);
        const FrE a = fr_at(J.h1.base, i * J.h1.stride + J.h1.col), b = fr_at(J.h2.base, i * J.h2.stride + J.h2.col);
        const FrE an = fr_at(J.h1.base, nx * J.h1.stride + J.h1.col);
        const FrE den = FrField::mul(FrField::add(FrField::add(a, FrField::mul(delta, b)), g), FrField::add(FrField::add(b, FrField::mul(delta, an)), g));
        FrField::store(D, i, den);
        FrField::store(N, i, num);
    }
}

__global__ void __launch_bounds__(smapplan::THREADS) bn_plookup_fold_kernel(const FrPlJob J, FrField::Mem *__restrict__ outF, u64 strideF, u64 colF,
                                                                           FrField::Mem *__restrict__ outT, u64 strideT, u64 colT) {
    const FrE alpha = fr_of(J.apow[0]), beta = fr_of(J.beta);
    for (u64 i = (u64)blockIdx.x * smapplan::THREADS + threadIdx.x; i < J.n; i += (u64)gridDim.x * smapplan::THREADS) {
        const FrE T = fr_pl_side(J.t, i, alpha, beta), F = fr_pl_side(J.f, i, alpha, T);
        FrField::store(outF, i * strideF + colF, F);
        FrField::store(outT, i * strideT + colT, T);
    }
}

// every launch of a product call, on st; the arguments have passed plookupplan::check_call() and n > 0, the pointers are the device's
int bn_plookup_prod_launch(const pil2gl_tuple_side &f, u64 kF, const pil2gl_tuple_side &t, u64 kT, const FrPlColumn &h1, const FrPlColumn &h2, const u64 *const *ch,
                           const FrPlColumn &out, u64 n, hipStream_t st) {
    const bnscan::Plan p = bnscan::plan(n, false);
    u64 *d;
    P2_TRY(scratch(SCR_BN_SCAN, 4 * p.elems + 8 * n, &d));        // the plan's levels, then D and N
    FrPlJob J{};
    plookupplan::pack(f, kF, t, kT, &h1, &h2, 1, (const u64 (*)[4])ch[0], ch[1], ch[2], ch[3], (const u64 *)nullptr, (const u64 *)nullptr, n, J);
    FrE one;
    bnp::bn_limbs(bnp::bn_mont_one().w, one.v);
    FrField::Mem *D = (FrField::Mem *)(d + 4 * p.elems), *N = D + n;
    bn_plookup_compress_kernel<<<smapplan::blocks(n), smapplan::THREADS, 0, st>>>(J, one, D, N);
    KERNEL_CHECK();
    uint4 *base = (uint4 *)d, *y = (uint4 *)((u64 *)out.base + 4 * out.col);
    P2_TRY(inverse_launch(p, base, (const uint4 *)D, 1, y, out.stride, y, out.stride, MODE_COLUMN, (const uint4 *)N, 1, Elem{}, st));
    return scan_launch<false>(p, base, y, out.stride, st);
}

int bn_plookup_fold_launch(const pil2gl_tuple_side &f, u64 kF, const pil2gl_tuple_side &t, u64 kT, const u64 *const *ch, const FrPlColumn *out, u64 n, hipStream_t st) {
    FrPlJob J{};
    plookupplan::pack(f, kF, t, kT, (const FrPlColumn *)nullptr, (const FrPlColumn *)nullptr, 1, (const u64 (*)[4])ch[0], ch[1], (const u64 *)nullptr,
                      (const u64 *)nullptr, (const u64 *)nullptr, (const u64 *)nullptr, n, J);
    bn_plookup_fold_kernel<<<smapplan::blocks(n), smapplan::THREADS, 0, st>>>(J, (FrField::Mem *)out[0].base, out[0].stride, out[0].col, (FrField::Mem *)out[1].base,
                                                                            out[1].stride, out[1].col);
    KERNEL_CHECK();
    return PIL2GL_OK;
}

int bn_plookup_check(const pil2gl_tuple_side *f, u64 kF, const pil2gl_tuple_side *t, u64 kT, const FrPlColumn *read, u32 nRead, u32 hDim, const u64 *const *ch, u32 nCh,
                     const FrPlColumn *out, u32 nOut, u64 n, bool dev) {
    char why[96];
    if (const char *msg = plookupplan::check_call(f, kF, t, kT, read, nRead, hDim, ch, nCh, out, nOut, n, 4, dev, why)) return fail(PIL2GL_EINVAL, "%s", msg);
    return PIL2GL_OK;
}

}  // namespace

extern "C" {

int pil2gl_bn128_plookup_fold_dev(const pil2gl_tuple_side *hostF, uint64_t kF, const pil2gl_tuple_side *hostT, uint64_t kT, const uint64_t *hostAlpha,
                                  const uint64_t *hostBeta, uint32_t hDim, uint64_t *outF, uint64_t strideF, uint64_t colF, uint64_t *outT, uint64_t strideT,
                                  uint64_t colT, uint64_t n, void *stream) {
    const u64 *const ch[2] = { hostAlpha, hostBeta };
    const FrPlColumn out[2] = { { outF, strideF, colF }, { outT, strideT, colT } };
    P2_TRY(bn_plookup_check(hostF, kF, hostT, kT, nullptr, 0, hDim, ch, 2, out, 2, n, true));
    if (!n) return PIL2GL_OK;
    P2_TRY(ensure_init());
    return bn_plookup_fold_launch(*hostF, kF, *hostT, kT, ch, out, n, as_stream(stream));
}

// host matrices, each staged up to the last element touched; an output's matrix goes up as it is and comes back with the column written
// (outF and outT of one matrix: that matrix once)
int pil2gl_bn128_plookup_fold(const pil2gl_tuple_side *hostF, uint64_t kF, const pil2gl_tuple_side *hostT, uint64_t kT, const uint64_t *hostAlpha,
                              const uint64_t *hostBeta, uint32_t hDim, uint64_t *hostOutF, uint64_t strideF, uint64_t colF, uint64_t *hostOutT, uint64_t strideT,
                              uint64_t colT, uint64_t n) {
    const u64 *const ch[2] = { hostAlpha, hostBeta };
    FrPlColumn out[2] = { { hostOutF, strideF, colF }, { hostOutT, strideT, colT } };
    P2_TRY(bn_plookup_check(hostF, kF, hostT, kT, nullptr, 0, hDim, ch, 2, out, 2, n, false));
    if (!n) return PIL2GL_OK;
    pil2gl_tuple_side f = *hostF, t = *hostT;
    const bool same = hostOutF == hostOutT;
    u64 wF = plookupplan::column_words(out[0], 1, n, 4), wT = plookupplan::column_words(out[1], 1, n, 4);
    if (same) wF = wT = wF > wT ? wF : wT;
    Stage s(tupleside::staged_words(f, n, kF, 4) + tupleside::staged_words(t, n, kT, 4) + smapplan::pad16(wF) + (same ? 0 : smapplan::pad16(wT)));
    P2_TRY(s.rc());
    tupleside::stage_side(s, f, n, kF, 4);
    tupleside::stage_side(s, t, n, kT, 4);
    out[0].base = s.put(hostOutF, wF); s.take(smapplan::pad16(wF) - wF);
    out[1].base = same ? out[0].base : s.put(hostOutT, wT);
    P2_TRY(s.rc());
    P2_TRY(bn_plookup_fold_launch(f, kF, t, kT, ch, out, n, 0));
    P2_TRY(s.get(hostOutF, out[0].base, wF));
    return same ? PIL2GL_OK : s.get(hostOutT, out[1].base, wT);
}

int pil2gl_bn128_plookup_prod_dev(const pil2gl_tuple_side *hostF, uint64_t kF, const pil2gl_tuple_side *hostT, uint64_t kT, const uint64_t *h1, uint64_t h1Stride,
                                  uint64_t h1Col, const uint64_t *h2, uint64_t h2Stride, uint64_t h2Col, uint32_t hDim, const uint64_t *hostAlpha,
                                  const uint64_t *hostBeta, const uint64_t *hostGamma, const uint64_t *hostDelta, uint64_t *out, uint64_t outStride,
                                  uint64_t outCol, uint64_t n, void *stream) {
    const u64 *const ch[4] = { hostAlpha, hostBeta, hostGamma, hostDelta };
    const FrPlColumn h[2] = { { h1, h1Stride, h1Col }, { h2, h2Stride, h2Col } }, o = { out, outStride, outCol };
    P2_TRY(bn_plookup_check(hostF, kF, hostT, kT, h, 2, hDim, ch, 4, &o, 1, n, true));
    if (!n) return PIL2GL_OK;
    P2_TRY(ensure_init());
    return bn_plookup_prod_launch(*hostF, kF, *hostT, kT, h[0], h[1], ch, o, n, as_stream(stream));
}

int pil2gl_bn128_plookup_prod(const pil2gl_tuple_side *hostF, uint64_t kF, const pil2gl_tuple_side *hostT, uint64_t kT, const uint64_t *hostH1, uint64_t h1Stride,
                              uint64_t h1Col, const uint64_t *hostH2, uint64_t h2Stride, uint64_t h2Col, uint32_t hDim, const uint64_t *hostAlpha,
                              const uint64_t *hostBeta, const uint64_t *hostGamma, const uint64_t *hostDelta, uint64_t *hostOut, uint64_t outStride,
                              uint64_t outCol, uint64_t n) {
    const u64 *const ch[4] = { hostAlpha, hostBeta, hostGamma, hostDelta };
    FrPlColumn h[2] = { { hostH1, h1Stride, h1Col }, { hostH2, h2Stride, h2Col } }, o = { hostOut, outStride, outCol };
    P2_TRY(bn_plookup_check(hostF, kF, hostT, kT, h, 2, hDim, ch, 4, &o, 1, n, false));
    if (!n) return PIL2GL_OK;
    pil2gl_tuple_side f = *hostF, t = *hostT;
    const u64 outWords = plookupplan::column_words(o, 1, n, 4);
    Stage s(tupleside::staged_words(f, n, kF, 4) + tupleside::staged_words(t, n, kT, 4) + smapplan::pad16(plookupplan::column_words(h[0], 1, n, 4)) +
            smapplan::pad16(plookupplan::column_words(h[1], 1, n, 4)) + smapplan::pad16(outWords));
    P2_TRY(s.rc());
    tupleside::stage_side(s, f, n, kF, 4);
    tupleside::stage_side(s, t, n, kT, 4);
    plookupplan::stage_column(s, h[0], 1, n, 4);
    plookupplan::stage_column(s, h[1], 1, n, 4);
    o.base = s.put(hostOut, outWords);
    P2_TRY(s.rc());
    P2_TRY(bn_plookup_prod_launch(f, kF, t, kT, h[0], h[1], ch, o, n, 0));
    return s.get(hostOut, o.base, outWords);
}

}  // extern "C"
