// Products with a sparse polynomial, scaled sums and the degree of polynomials over the BN254 scalar field Fr, gfx950: what shplonkjs
// open (computeOpeningsFflonk, fflonk_prover_helpers.js:212) does between its evaluations and its divisions -- the Polynomial class's
// add, sub, mulScalar, byXSubValue, byXNSubValue and degree on vectors of up to 2^28 coefficients.  One form covers the first five:
//
//     acc[i] <- s acc[i] + sum_{j < t} m[j] src[i - e[j]]        0 <= i < nAcc,   src[x] = 0 for x < 0 or x >= nSrc
//
// the product of src with M(x) = sum_j m[j] x^e[j] added to the scaled accumulator.  s = NULL means "no accumulator": acc is written and
// never read.  A zerofier prod_j (x^k_j - beta_j), multiplied out on the host, is ONE sweep; W += alpha^i Z f_i is one call.
//
//   fma      a lane per output element i, a loop over the t terms (their count and exponents are the same for every lane: the loop is
//            uniform, a term's range test is not).  A term whose source index i - e[j] lies outside [0, nSrc) is skipped BEFORE its load.
//            The compacted term list (the host drops zero coefficients) travels as kernel arguments: at most 64 x 40 bytes, read through
//            the scalar cache, no copy, no working buffer.  A coefficient equal to 1 or r - 1 (Montgomery form) is an fr_add / fr_sub
//            without the product, and s = 1 leaves the accumulator as loaded: add / sub of the reference are pure additions.
//   degree   a lane per element, from the top of the column down, all eight 32-bit words deciding; a ballot and one atomic maximum of
//            (index + 1) per wave that saw a non-zero element, into a cell cleared to 0: the host reads cell - 1, which is UINT64_MAX for
//            the zero polynomial.  A wave whose elements all lie below what the cell already holds leaves without loading them.
//
// Elements are 32 bytes of Montgomery words, canonical in and out, moved as two 16-byte halves as in bn_poly.hip; add, sub and mul are
// bn_field.cuh's.  Fr arithmetic is exact: every order of the sum gives the same bytes.  All index arithmetic is 64-bit.
//
// Aliasing: a lane writes acc[i] only and reads acc[i] and src[i - e[j]].  With t = 1, e[0] = 0 those are the same index, so acc may be
// the same column as src; in every other case a lane would read what another lane writes, and the entries refuse any shared element.
// Memory safety rests on the range tests alone: i < nAcc, 0 <= i - e[j] < nSrc.
#include "bn_column_stage.h"
#include "bn_elem.cuh"
#include "bn_params.h"

using namespace pil2gl;
using bn::u32;
using bn::unpack;

namespace {

constexpr u32 THREADS = 256;
constexpr u32 MAX_TERMS = 64;

enum Scale : u32 { SCALE_NONE = 0, SCALE_ONE = 1, SCALE_MUL = 2 };      // acc never read / kept as loaded / multiplied by s

struct Term { u32 m[8]; u64 e; };
struct FmaArgs {
    uint4 *acc; const uint4 *src;                    // element i at 2 * i * stride (in 16-byte halves)
    u64 nAcc, nSrc, accStride, srcStride;
    u64 oneMask, negMask;                            // bit j: m[j] is 1 / r - 1, the term is an addition / a subtraction
    u32 s[8];
    u32 scale, t;
    Term term[MAX_TERMS];
};
static_assert(sizeof(FmaArgs) <= 4096, "the term list travels as kernel arguments");

__global__ void __launch_bounds__(THREADS) bn_poly_fma_kernel(FmaArgs a) {
    const u64 i = (u64)blockIdx.x * THREADS + threadIdx.x;
    if (i >= a.nAcc) return;
    uint4 *pa = a.acc + 2 * i * a.accStride;
    u32 x[8], y[8], c[8];
    if (a.scale == SCALE_NONE) {
#pragma unroll
        for (int l = 0; l < 8; l++) x[l] = 0;
    } else {
        unpack(pa[0], pa[1], x);
        if (a.scale == SCALE_MUL) {
#pragma unroll
            for (int l = 0; l < 8; l++) c[l] = a.s[l];
            bn::fr_mul(x, x, c);
        }
    }
    for (u32 j = 0; j < a.t; j++) {
        const u64 e = a.term[j].e;
        if (i < e || i - e >= a.nSrc) continue;      // outside the source: contributes nothing and is not loaded
        const uint4 *ps = a.src + 2 * (i - e) * a.srcStride;
        unpack(ps[0], ps[1], y);
        if ((a.oneMask >> j) & 1) bn::fr_add(x, y);
        else if ((a.negMask >> j) & 1) bn::fr_sub(x, y);
        else {
#pragma unroll
            for (int l = 0; l < 8; l++) c[l] = a.term[j].m[l];
            bn::fr_mul(y, y, c);
            bn::fr_add(x, y);
        }
    }
    bn::st_elem(pa, x);
}

// *best = max over the non-zero elements of (index + 1); the caller clears it to 0.  Lanes run over the column FROM THE TOP (lane g of
// the grid looks at element n - 1 - g), so the workgroups dispatched first hold the highest indices: a wave first reads the cell and
// leaves, without loading its elements, when the cell already holds more than anything it could find.  The cell only grows and the
// result is a maximum, so a stale reading costs a wave its shortcut and nothing else.  (A lane per element in ascending order, an atomic
// per wave, measured 1.56 ms on 2^24 elements: the 2^17 atomics on the one cell, 23 times the traffic floor.)
__global__ void __launch_bounds__(THREADS) bn_poly_degree_kernel(const uint4 *__restrict__ col, u64 n, u64 stride, unsigned long long *best) {
    const u64 g = (u64)blockIdx.x * THREADS + threadIdx.x, g0 = g & ~63ull;  // g0: the wave's first lane, its highest element n - 1 - g0
    if (g0 >= n) return;
    if (__hip_atomic_load(best, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= n - g0) return;
    bool nz = false;
    if (g < n) {
        const u64 i = n - 1 - g;
        const uint4 a = col[2 * i * stride], b = col[2 * i * stride + 1];
        nz = !bn::is_zero(a, b);
    }
    const u64 mask = __ballot(nz);
    if (mask && g == g0) atomicMax(best, (unsigned long long)(n - g0 - __builtin_ctzll(mask)));      // the lowest lane set is the highest element
}

struct Call {
    u64 *acc; u64 nAcc, accStride; const u64 *scale;
    const u64 *src; u64 nSrc, srcStride;
    const u64 *coefs, *exps; u32 t;
};

bool words_eq(const u64 *a, const bnp::U256 &b) { return a[0] == b.w[0] && a[1] == b.w[1] && a[2] == b.w[2] && a[3] == b.w[3]; }
bool words_zero(const u64 *a) { return (a[0] | a[1] | a[2] | a[3]) == 0; }

int check(const Call &c) {
    P2_TRY(check_column(c.acc, c.nAcc, c.accStride, "acc"));
    P2_TRY(check_column(c.src, c.nSrc, c.srcStride, "src"));
    if (c.t == 0 || c.t > MAX_TERMS) return fail(PIL2GL_EINVAL, "t = %u: 1 <= t <= %u terms", c.t, MAX_TERMS);
    if (!c.coefs || !c.exps) return fail(PIL2GL_EINVAL, "null buffer (hostCoefs / hostExps)");
    for (u32 j = 1; j < c.t; j++)
        if (c.exps[j] <= c.exps[j - 1]) return fail(PIL2GL_EINVAL, "exponents must be strictly increasing (e[%u] = %llu after %llu)", j, (unsigned long long)c.exps[j], (unsigned long long)c.exps[j - 1]);
    const u64 eMax = c.exps[c.t - 1];
    if (eMax > bncol::MAX_N) return fail(PIL2GL_EINVAL, "exponent %llu: at most 2^28", (unsigned long long)eMax);
    if (c.nSrc && c.nSrc + eMax > c.nAcc)
        return fail(PIL2GL_EINVAL, "the product has %llu + %llu coefficients, acc holds %llu: nothing is truncated", (unsigned long long)c.nSrc, (unsigned long long)eMax, (unsigned long long)c.nAcc);
    const bncol::Relation rel = bncol::relation((uintptr_t)c.acc, c.accStride, c.nAcc, (uintptr_t)c.src, c.srcStride, c.nSrc);
    if (rel == bncol::OVERLAP || (rel == bncol::SAME && !(c.t == 1 && c.exps[0] == 0)))
        return fail(PIL2GL_EINVAL, "acc overlaps src (only columns of one section may interleave; the same column only with t = 1, e = 0)");
    return PIL2GL_OK;
}

int fma_launch(const Call &c, hipStream_t st) {
    if (c.nAcc == 0) return PIL2GL_OK;
    FmaArgs a{};
    a.acc = (uint4 *)c.acc; a.src = (const uint4 *)c.src;
    a.nAcc = c.nAcc; a.nSrc = c.nSrc; a.accStride = c.accStride; a.srcStride = c.srcStride;
    if (c.scale) {
        a.scale = words_eq(c.scale, bnp::bn_mont_one()) ? SCALE_ONE : SCALE_MUL;
        bnp::bn_limbs(c.scale, a.s);
    }
    if (c.nSrc)
        for (u32 j = 0; j < c.t; j++) {              // zero coefficients are dropped here
            const u64 *m = c.coefs + 4 * j;
            if (words_zero(m)) continue;
            if (words_eq(m, bnp::bn_mont_one())) a.oneMask |= 1ull << a.t;
            else if (words_eq(m, bnp::bn_mont_neg_one())) a.negMask |= 1ull << a.t;
            bnp::bn_limbs(m, a.term[a.t].m);
            a.term[a.t].e = c.exps[j];
            a.t++;
        }
    bn_poly_fma_kernel<<<(unsigned)((c.nAcc + THREADS - 1) / THREADS), THREADS, 0, st>>>(a);
    KERNEL_CHECK();
    return PIL2GL_OK;
}

int check_degree(const u64 *src, u64 n, u64 stride, const u64 *degree) {
    if (!degree) return fail(PIL2GL_EINVAL, "null buffer (degree)");
    return check_column(src, n, stride, "src");
}

// blocks for the 8-byte readback
int degree_run(const u64 *src, u64 n, u64 stride, u64 *degree, hipStream_t st) {
    u64 *cell;
    P2_TRY(scratch(SCR_BN_POLYMUL, 2, &cell));
    HIP_TRY(hipMemsetAsync(cell, 0, 8, st));
    bn_poly_degree_kernel<<<(unsigned)((n + THREADS - 1) / THREADS), THREADS, 0, st>>>((const uint4 *)src, n, stride, (unsigned long long *)cell);
    KERNEL_CHECK();
    u64 top = 0;
    HIP_TRY(hipMemcpyAsync(&top, cell, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    *degree = top - 1;                               // 0: no non-zero element, UINT64_MAX
    return PIL2GL_OK;
}

}  // namespace

extern "C" {

int pil2gl_bn128_poly_fma_dev(uint64_t *acc, uint64_t nAcc, uint64_t accStride, const uint64_t *hostScale,
                              const uint64_t *src, uint64_t nSrc, uint64_t srcStride,
                              const uint64_t *hostCoefs, const uint64_t *hostExps, uint32_t t, void *stream) {
    const Call c{ acc, nAcc, accStride, hostScale, src, nSrc, srcStride, hostCoefs, hostExps, t };
    P2_TRY(check(c));
    if (nAcc == 0) return PIL2GL_OK;
    P2_TRY(check_aligned16({ acc, src }));
    P2_TRY(ensure_init());
    return fma_launch(c, as_stream(stream));
}

int pil2gl_bn128_poly_fma(uint64_t *acc, uint64_t nAcc, uint64_t accStride, const uint64_t *hostScale,
                          const uint64_t *src, uint64_t nSrc, uint64_t srcStride,
                          const uint64_t *hostCoefs, const uint64_t *hostExps, uint32_t t) {
    Call c{ acc, nAcc, accStride, hostScale, src, nSrc, srcStride, hostCoefs, hostExps, t };
    P2_TRY(check(c));
    if (nAcc == 0) return PIL2GL_OK;
    // without a scale acc is written and never read; acc and src of one section, or the same column, are one staged range (bn_column.h)
    const bncol::Col cols[2] = { { (uintptr_t)acc, nAcc, accStride, hostScale != nullptr, true }, { (uintptr_t)src, nSrc, srcStride, true, false } };
    ColumnStage s(cols, 2);
    P2_TRY(s.rc());
    c.acc = s.dev(0); c.src = s.dev(1);
    P2_TRY(fma_launch(c, 0));
    return s.copy_back();
}

int pil2gl_bn128_poly_degree_dev(const uint64_t *src, uint64_t n, uint64_t stride, uint64_t *degree, void *stream) {
    P2_TRY(check_degree(src, n, stride, degree));
    *degree = ~0ull;
    if (n == 0) return PIL2GL_OK;
    P2_TRY(check_aligned16({ src }));
    P2_TRY(ensure_init());
    return degree_run(src, n, stride, degree, as_stream(stream));
}

int pil2gl_bn128_poly_degree(const uint64_t *src, uint64_t n, uint64_t stride, uint64_t *degree) {
    P2_TRY(check_degree(src, n, stride, degree));
    *degree = ~0ull;
    if (n == 0) return PIL2GL_OK;
    const bncol::Col col{ (uintptr_t)src, n, stride, true, false };
    ColumnStage s(&col, 1);
    P2_TRY(s.rc());
    return degree_run(s.dev(0), n, stride, degree, 0);
}

}  // extern "C"
