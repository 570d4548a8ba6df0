// Stage-2 witness hints on the device: the grand product / grand sum columns
//   calculateZ(F,num,den)  src/helpers/polutils.js:128-143   z[0] = 1, z[i] = z[i-1] * num[i-1] / den[i-1]
//   calculateS(F,num,den)  src/helpers/polutils.js:145-164   s[i] = s[i-1] + num / den[i]        (num: one element)
// called from resolveHint (src/prover/hints_helpers.js:91-114).  The reference walks the column serially with BigInt
// arithmetic after one batch inversion; here a thread inverts its eight denominators together (one field inversion per
// eight rows) and the running product / sum is a three-kernel scan: per-block inclusive scan + block totals, scan of the
// totals, then the fix-up (for the product: shifted by one row, z[0] = 1).  Operands may be base (dim 1) or cubic
// extension (dim 3) columns, row-major; the result is dim 3 if either operand is, else dim 1.  gsum_col is the sum with a column
// numerator; the lookup grand sum further down folds a lookup's sides into the sum's first pass, and the grand product behind it a
// permutation's or a connection's terms into the product's.
#include "common.h"
#include "gl_field.cuh"
#include "hint_plan.h"
#include "logup_sum_plan.h"
#include "grand_prod_plan.h"
#include <utility>

using namespace gl;
using namespace pil2gl;
using hintplan::SCAN_THREADS;
using hintplan::SCAN_ITEMS;
using hintplan::SCAN_CHUNK;

namespace {

__device__ __forceinline__ E3 ld_dim(const u64 *p, u64 i, u32 dim) { return dim == 3 ? E3{ { p[3 * i], p[3 * i + 1], p[3 * i + 2] } } : E3{ { p[i], 0, 0 } }; }
__device__ __forceinline__ void st3(u64 *p, u64 i, const E3 &v) { p[3 * i] = v.v[0]; p[3 * i + 1] = v.v[1]; p[3 * i + 2] = v.v[2]; }
template <bool PROD> __device__ __forceinline__ E3 comb(const E3 &a, const E3 &b) { return PROD ? e3_mul(a, b) : e3_add(a, b); }
template <bool PROD> __device__ __forceinline__ E3 ident() { return PROD ? E3{ { 1, 0, 0 } } : E3{ { 0, 0, 0 } }; }

// inclusive scan of the 256 per-thread totals in LDS (Hillis-Steele); returns this thread's exclusive prefix
template <bool PROD>
__device__ E3 block_exclusive(E3 total, E3 *sh, E3 *blockTotal) {
    const u32 t = threadIdx.x;
    sh[t] = total;
    __syncthreads();
    for (u32 d = 1; d < SCAN_THREADS; d <<= 1) {
        E3 v = sh[t];
        if (t >= d) v = comb<PROD>(sh[t - d], v);
        __syncthreads();
        sh[t] = v;
        __syncthreads();
    }
    const E3 ex = t ? sh[t - 1] : ident<PROD>();
    *blockTotal = sh[SCAN_THREADS - 1];
    __syncthreads();
    return ex;
}

// pass 1: ratios, block-local inclusive scan into tmp (n x 3), block totals.  COLNUM: the numerator is a column of n rows (always for the
// product; for the sum it is ONE element unless asked for)
template <bool PROD, bool COLNUM = PROD>
__global__ void __launch_bounds__(SCAN_THREADS) hint_scan1(const u64 *__restrict__ num, u32 dimNum, const u64 *__restrict__ den, u32 dimDen, u64 n,
                                                          u64 *__restrict__ tmp, u64 *__restrict__ totals) {
    __shared__ E3 sh[SCAN_THREADS];
    const u64 base = (u64)blockIdx.x * SCAN_CHUNK + (u64)threadIdx.x * SCAN_ITEMS;
    E3 loc[SCAN_ITEMS];
    E3 run = ident<PROD>();
    const E3 numS = COLNUM ? ident<true>() : ld_dim(num, 0, dimNum);
    // the thread's SCAN_ITEMS denominators are inverted together (Montgomery's trick, what the reference's F.batchInverse does for the whole
    // column, polutils.js:134): ONE field inversion -- an exponentiation, ~130 products -- and three extension products per row instead
    // of an inversion per row.  A zero denominator inverts to zero, as it does alone (0^(p-2)): it is kept out of the running product.
    const E3 one = ident<true>();
    u32 zero = 0;
    E3 acc = one;
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; k++) {
        const u64 i = base + k;
        E3 d = i < n ? ld_dim(den, i, dimDen) : one;
        if (!(d.v[0] | d.v[1] | d.v[2])) { zero |= 1u << k; d = one; }
        loc[k] = acc;                                   // the product of the denominators before this one
        acc = e3_mul(acc, d);
    }
    E3 ai = (acc.v[1] | acc.v[2]) ? e3_inv(acc) : E3{ { inv(acc.v[0]), 0, 0 } };
#pragma unroll
    for (int k = SCAN_ITEMS - 1; k >= 0; k--) {
        const u64 i = base + k;
        E3 d = i < n ? ld_dim(den, i, dimDen) : one;
        if ((zero >> k) & 1) d = one;
        const E3 di = e3_mul(ai, loc[k]);               // 1 / d_k
        ai = e3_mul(ai, d);
        loc[k] = ((zero >> k) & 1) ? E3{ { 0, 0, 0 } } : di;
    }
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; k++) {
        const u64 i = base + k;
        if (i < n) {
            const E3 r = e3_mul(COLNUM ? ld_dim(num, i, dimNum) : numS, loc[k]);
            run = comb<PROD>(run, r);
        }
        loc[k] = run;
    }
    E3 bt;
    const E3 ex = block_exclusive<PROD>(run, sh, &bt);
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; k++) { const u64 i = base + k; if (i < n) st3(tmp, i, comb<PROD>(ex, loc[k])); }
    if (threadIdx.x == 0) st3(totals, blockIdx.x, bt);
}
// pass 2: exclusive scan of the block totals, one block (each thread walks a contiguous run)
template <bool PROD>
__global__ void __launch_bounds__(SCAN_THREADS) hint_scan2(u64 *__restrict__ totals, u64 nb) {
    __shared__ E3 sh[SCAN_THREADS];
    const u64 per = hintplan::totals_per_lane(nb), b0 = (u64)threadIdx.x * per;
    E3 run = ident<PROD>();
    for (u64 k = 0; k < per; k++) { const u64 i = b0 + k; if (i < nb) run = comb<PROD>(run, ld_dim(totals, i, 3)); }
    E3 bt;
    E3 ex = block_exclusive<PROD>(run, sh, &bt);
    for (u64 k = 0; k < per; k++) {
        const u64 i = b0 + k;
        if (i < nb) { const E3 v = ld_dim(totals, i, 3); st3(totals, i, ex); ex = comb<PROD>(ex, v); }
    }
}
// pass 3: add the block prefix; the product column is the EXCLUSIVE scan (z[0] = 1), the sum column the inclusive one
// out: element i at word i outStride + outCol (a dense column: outStride = dimOut, outCol = 0)
template <bool PROD>
__global__ void hint_scan3(const u64 *__restrict__ tmp, const u64 *__restrict__ totals, u64 n, u32 dimOut, u64 *__restrict__ out, u64 outStride, u64 outCol) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    E3 v;
    if (PROD) {
        if (i == 0) v = ident<true>();
        else { const u64 j = i - 1; v = comb<true>(ld_dim(totals, j / SCAN_CHUNK, 3), ld_dim(tmp, j, 3)); }
    } else v = comb<false>(ld_dim(totals, i / SCAN_CHUNK, 3), ld_dim(tmp, i, 3));
    u64 *o = out + i * outStride + outCol;
    o[0] = v.v[0];
    if (dimOut == 3) { o[1] = v.v[1]; o[2] = v.v[2]; }
}

template <bool PROD, bool COLNUM = PROD>
int run_hint(const u64 *num, u32 dimNum, const u64 *den, u32 dimDen, u64 n, u64 *out, hipStream_t st) {
    if (n == 0) return PIL2GL_OK;
    if (!num || !den || !out) return fail(PIL2GL_EINVAL, "null buffer");
    if ((dimNum != 1 && dimNum != 3) || (dimDen != 1 && dimDen != 3)) return fail(PIL2GL_EINVAL, "dimensions must be 1 or 3");
    const u64 nb = hintplan::blocks(n);
    if (nb > 0x7fffffffull) return fail(PIL2GL_EINVAL, "grid too large");
    u64 *tmp, *totals;
    P2_TRY(scratch(SCR_HINT_TMP, n * 3, &tmp));
    P2_TRY(scratch(SCR_HINT_TOTALS, nb * 3, &totals));
    hint_scan1<PROD, COLNUM><<<(unsigned)nb, SCAN_THREADS, 0, st>>>(num, dimNum, den, dimDen, n, tmp, totals);
    KERNEL_CHECK();
    hint_scan2<PROD><<<1, SCAN_THREADS, 0, st>>>(totals, nb);
    KERNEL_CHECK();
    const u32 dimOut = (dimNum == 3 || dimDen == 3) ? 3u : 1u;
    hint_scan3<PROD><<<(unsigned)((n + 255) / 256), 256, 0, st>>>(tmp, totals, n, dimOut, out, dimOut, 0);
    KERNEL_CHECK();
    return PIL2GL_OK;
}

}  // namespace

extern "C" {

int pil2gl_gprod_dev(const uint64_t *num, uint32_t dimNum, const uint64_t *den, uint32_t dimDen, uint64_t n, uint64_t *out, void *stream) {
    P2_TRY(ensure_init());
    return run_hint<true>(num, dimNum, den, dimDen, n, out, as_stream(stream));
}
int pil2gl_gsum_dev(const uint64_t *num, uint32_t dimNum, const uint64_t *den, uint32_t dimDen, uint64_t n, uint64_t *out, void *stream) {
    P2_TRY(ensure_init());
    return run_hint<false>(num, dimNum, den, dimDen, n, out, as_stream(stream));
}
int pil2gl_gsum_col_dev(const uint64_t *num, uint32_t dimNum, const uint64_t *den, uint32_t dimDen, uint64_t n, uint64_t *out, void *stream) {
    P2_TRY(ensure_init());
    return run_hint<false, true>(num, dimNum, den, dimDen, n, out, as_stream(stream));
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------------------------------
// The lookup grand sum (include/pil2gl.h states it; tests/logup_sum_ref.py restates it over integers):
//   s[i] = s[i-1] + sum_u coef_u w_u[i] / D_u[i],   D_u[i] = sum_j v_j[i] alpha^(k_u - j) + busId_u + beta
// One fused first pass beside hint_scan1, then hint_scan2<false> and hint_scan3<false> as they are.  A lane takes its SCAN_ITEMS rows;
// for each row it folds the terms into ONE fraction N / D in registers,
//   N <- N D_u + (coef_u w_u) D,   D <- D D_u        (a zero D_u is left out of both: the term adds 0 and spoils nothing)
// so that a row costs one inverse whatever nTerms is, and the lane inverts its rows' D together: one e3_inv a lane, as hint_scan1.
// No denominator column is ever written.  The powers of alpha and busId + beta are made on the host, so a tuple column costs three
// base products (a base value scaling an extension power), not an extension product.  Base products a row, nTerms terms of k columns:
// nTerms (3 k + 16) for the fold (two extension products of 6, a scaling of 3, coef w), 6 + 6 + 6 for the shared inversion and the
// ratio, and 1/8 of the lane's e3_inv.
// The term table travels as a kernel argument and is read with wave-uniform indices (scalar loads from the kernel-argument segment):
// nothing is copied to the device and nothing lies in a private segment.
// Safety: nothing read from a matrix is used as an address; a row index is checked against n before any load.
namespace {

using logupplan::MAX_TERMS;

struct LogupTerm {
    const u64 *base, *sel;                           // sel null: w = 1
    u64 stride, selStride, selCol;
    u32 cols[tupleside::MAX_K];
    u32 k;
    u64 coef;
    E3 cst;                                          // busId + beta
};
struct LogupJob {
    LogupTerm t[MAX_TERMS];
    E3 apow[tupleside::MAX_K + 1];                   // apow[e] = alpha^e, e = 1 .. 16
    u32 nTerms;
    u64 n;
};

// f(k) for k = 0 .. SCAN_ITEMS - 1 with k a compile-time constant: the lane's per-row arrays are indexed by constants from the start
// and live in registers (a #pragma unroll around loops with run-time trip counts left them in the private segment)
template <class Fn, int... K> __device__ __forceinline__ void each_item(Fn f, std::integer_sequence<int, K...>) { (f(std::integral_constant<int, K>{}), ...); }
template <class Fn> __device__ __forceinline__ void each_item(Fn f) { each_item(f, std::make_integer_sequence<int, SCAN_ITEMS>{}); }
template <class Fn, int... K> __device__ __forceinline__ void each_item_down(Fn f, std::integer_sequence<int, K...>) { (f(std::integral_constant<int, SCAN_ITEMS - 1 - K>{}), ...); }
template <class Fn> __device__ __forceinline__ void each_item_down(Fn f) { each_item_down(f, std::make_integer_sequence<int, SCAN_ITEMS>{}); }

__global__ void __launch_bounds__(SCAN_THREADS) logup_scan1(const LogupJob J, u64 *__restrict__ tmp, u64 *__restrict__ totals) {
    __shared__ E3 sh[SCAN_THREADS];
    const u64 base = (u64)blockIdx.x * SCAN_CHUNK + (u64)threadIdx.x * SCAN_ITEMS;
    // the lane's rows as fractions num / den, den never zero; rows at or past n stay 0 / 1.  The terms are the outer loop, so that a term's
    // table entries are read once for the lane's rows and the rows' loads of one column are in flight together
    E3 num[SCAN_ITEMS], den[SCAN_ITEMS], loc[SCAN_ITEMS];
    each_item([&](auto k) { num[k] = ident<false>(); den[k] = ident<true>(); });
    for (u32 u = 0; u < J.nTerms; u++) {
        const LogupTerm &T = J.t[u];
        const E3 cst = T.cst;
        each_item([&](auto k) { loc[k] = cst; });
        for (u32 j = 0; j < T.k; j++) {
            const E3 ap = J.apow[T.k - j];
            const u64 *p = T.base + base * T.stride + T.cols[j];
            each_item([&](auto k) { if (base + k < J.n) loc[k] = e3_add(loc[k], e3_scale(ap, p[k * T.stride])); });
        }
        each_item([&](auto k) {
            const u64 i = base + k;
            const E3 d = loc[k];
            if (i >= J.n || !(d.v[0] | d.v[1] | d.v[2])) return;             // a zero D_u: the term adds 0 and is left out of the product
            const u64 c = T.sel ? mul(T.sel[i * T.selStride + T.selCol], T.coef) : T.coef;
            num[k] = e3_add(e3_mul(num[k], d), e3_scale(den[k], c));
            den[k] = e3_mul(den[k], d);
        });
    }
    E3 acc = ident<true>();
    each_item([&](auto k) {
        loc[k] = acc;                                   // the product of the rows' den before this one
        acc = e3_mul(acc, den[k]);
    });
    E3 ai = (acc.v[1] | acc.v[2]) ? e3_inv(acc) : E3{ { inv(acc.v[0]), 0, 0 } };
    each_item_down([&](auto k) {
        const E3 di = e3_mul(ai, loc[k]);               // 1 / den_k
        ai = e3_mul(ai, den[k]);
        loc[k] = e3_mul(num[k], di);
    });
    E3 run = ident<false>();
    each_item([&](auto k) { run = e3_add(run, loc[k]); loc[k] = run; });      // rows at or past n hold num = 0
    E3 bt;
    const E3 ex = block_exclusive<false>(run, sh, &bt);
    each_item([&](auto k) { const u64 i = base + k; if (i < J.n) st3(tmp, i, e3_add(ex, loc[k])); });
    if (threadIdx.x == 0) st3(totals, blockIdx.x, bt);
}

u64 h_canon(u64 a) { return a >= P ? a - P : a; }

// every launch of a call, on st; the arguments have passed logupplan::check_call() and n > 0, the pointers are the device's
int logup_launch(const pil2gl_logup_term *terms, u32 nTerms, const u64 *alpha, const u64 *beta, u64 *out, u64 outStride, u64 outCol, u64 n, hipStream_t st) {
    LogupJob J{};
    const u64 a[3] = { h_canon(alpha[0]), h_canon(alpha[1]), h_canon(alpha[2]) };
    u64 pw[3] = { 1, 0, 0 };
    for (u32 e = 1; e <= tupleside::MAX_K; e++) {
        u64 r[3];
        h_e3_mul(pw, a, r);
        for (int c = 0; c < 3; c++) J.apow[e].v[c] = pw[c] = r[c];
    }
    for (u32 u = 0; u < nTerms; u++) {
        const pil2gl_tuple_side &s = terms[u].side;
        LogupTerm &T = J.t[u];
        T.base = s.base; T.sel = s.sel; T.stride = s.stride; T.selStride = s.selStride; T.selCol = s.selCol;
        T.k = (u32)terms[u].k;
        for (u32 j = 0; j < T.k; j++) T.cols[j] = (u32)s.hostCols[j];
        T.coef = terms[u].coef[0];
        T.cst = E3{ { h_add(h_canon(beta[0]), terms[u].busId[0]), h_canon(beta[1]), h_canon(beta[2]) } };
    }
    J.nTerms = nTerms; J.n = n;
    const u64 nb = hintplan::blocks(n);
    u64 *tmp, *totals;
    P2_TRY(scratch(SCR_HINT_TMP, n * 3, &tmp));
    P2_TRY(scratch(SCR_HINT_TOTALS, nb * 3, &totals));
    logup_scan1<<<(unsigned)nb, SCAN_THREADS, 0, st>>>(J, tmp, totals);
    KERNEL_CHECK();
    hint_scan2<false><<<1, SCAN_THREADS, 0, st>>>(totals, nb);
    KERNEL_CHECK();
    hint_scan3<false><<<(unsigned)((n + 255) / 256), 256, 0, st>>>(tmp, totals, n, 3, out, outStride, outCol);
    KERNEL_CHECK();
    return PIL2GL_OK;
}

int logup_check(const pil2gl_logup_term *terms, u64 nTerms, const u64 *alpha, const u64 *beta, const u64 *out, u64 outStride, u64 outCol, u64 n, bool dev) {
    char why[96];
    if (const char *msg = logupplan::check_call(terms, nTerms, alpha, beta, out, outStride, outCol, n, 1, dev, why)) return fail(PIL2GL_EINVAL, "%s", msg);
    return PIL2GL_OK;
}

}  // namespace

extern "C" {

int pil2gl_logup_sum_plan(uint64_t n, uint64_t nTerms, uint32_t elemWords, uint32_t *outInfo, uint64_t *workBytes) {
    if (workBytes) *workBytes = 0;
    if (const char *msg = logupplan::check(n, nTerms, elemWords)) return fail(PIL2GL_EINVAL, "%s", msg);
    const logupplan::Plan p = logupplan::plan(n, elemWords);
    if (outInfo) {
        outInfo[0] = p.threads; outInfo[1] = p.items; outInfo[2] = p.blocks; outInfo[3] = p.launches; outInfo[4] = p.depth;
        outInfo[5] = logupplan::out_width(elemWords);
    }
    if (workBytes) *workBytes = p.bytes;
    return PIL2GL_OK;
}

int pil2gl_logup_sum_dev(const pil2gl_logup_term *hostTerms, uint64_t nTerms, const uint64_t *hostAlpha, const uint64_t *hostBeta,
                         uint64_t *out, uint64_t outStride, uint64_t outCol, uint64_t n, void *stream) {
    P2_TRY(logup_check(hostTerms, nTerms, hostAlpha, hostBeta, out, outStride, outCol, n, true));
    if (!n) return PIL2GL_OK;
    P2_TRY(ensure_init());
    return logup_launch(hostTerms, (u32)nTerms, hostAlpha, hostBeta, out, outStride, outCol, n, as_stream(stream));
}

// host matrices, each staged up to the last element touched; out's matrix goes up as it is and comes back with the column written
int pil2gl_logup_sum(const pil2gl_logup_term *hostTerms, uint64_t nTerms, const uint64_t *hostAlpha, const uint64_t *hostBeta,
                     uint64_t *hostOut, uint64_t outStride, uint64_t outCol, uint64_t n) {
    P2_TRY(logup_check(hostTerms, nTerms, hostAlpha, hostBeta, hostOut, outStride, outCol, n, false));
    if (!n) return PIL2GL_OK;
    pil2gl_logup_term terms[MAX_TERMS];
    const u64 outWords = tupleside::span_bytes(n, outStride, outCol + 2, 1) / 8;
    u64 total = smapplan::pad16(outWords);
    for (u64 u = 0; u < nTerms; u++) { terms[u] = hostTerms[u]; total += tupleside::staged_words(terms[u].side, n, terms[u].k, 1); }
    Stage s(total);
    P2_TRY(s.rc());
    for (u64 u = 0; u < nTerms; u++) tupleside::stage_side(s, terms[u].side, n, terms[u].k, 1);
    u64 *dOut = (u64 *)s.put(hostOut, outWords);
    P2_TRY(s.rc());
    P2_TRY(logup_launch(terms, (u32)nTerms, hostAlpha, hostBeta, dOut, outStride, outCol, n, 0));
    return s.get(hostOut, dOut, outWords);
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------------------------------
// The grand product of a permutation or a connection (include/pil2gl.h states it; tests/grand_prod_ref.py restates it over integers):
//   z[0] = 1, z[i] = z[i-1] R[i-1],   R = prod_{num terms} D_u / prod_{den terms} D_u,   D_u = B_u + idCoef_u id_u + gamma,
//   B_u = H_u or (H_u - beta) sel_u + beta,   H_u = sum_j v_j alpha^(k_u - 1 - j)
// One fused first pass beside hint_scan1 and logup_scan1, then hint_scan2<true> and hint_scan3<true> as they are (the shift by one row
// that makes the product exclusive is hint_scan3's).  A lane takes its SCAN_ITEMS rows and keeps each row's N and D as extension elements
// in registers, N <- N D_u or D <- D D_u; it inverts its rows' D together, one e3_inv a lane, a zero D inverting to zero as in hint_scan1,
// so that a zero den factor gives R = 0; then the block-local product scan into tmp.  Neither num nor den is ever a column.
// The powers of alpha come from the host: a tuple column costs three base products, the last column none.  Base products a row, a term
// of k columns: 3 (k - 1) for H, 3 for a selector, 3 for an id, 6 for the product into N or D; then 18 for the shared inversion and the
// ratio, 6 for the lane's running product, 6 for the block prefix and 1/8 of the lane's e3_inv.
// The packed term table (grand_prod_plan.h) travels as a kernel argument and is read with wave-uniform indices.
// Safety: nothing read from a matrix is used as an address; a row index is checked against n before any load.
namespace {

typedef grandprodplan::Term<3> GprodTerm;
typedef grandprodplan::GlJob GprodJob;

__device__ __forceinline__ E3 e3_of(const u64 w[3]) { return E3{ { w[0], w[1], w[2] } }; }

__global__ void __launch_bounds__(SCAN_THREADS) gprod_fold_scan1(const GprodJob J, u64 *__restrict__ tmp, u64 *__restrict__ totals) {
    __shared__ E3 sh[SCAN_THREADS];
    const u64 base = (u64)blockIdx.x * SCAN_CHUNK + (u64)threadIdx.x * SCAN_ITEMS;
    const E3 beta = e3_of(J.beta), gamma = e3_of(J.gamma);
    // the lane's rows as N and D; rows at or past n stay 1 / 1.  The terms are the outer loop, so that a term's table entries are read once
    // for the lane's rows and the rows' loads of one column are in flight together
    E3 num[SCAN_ITEMS], den[SCAN_ITEMS], loc[SCAN_ITEMS];
    each_item([&](auto k) { num[k] = ident<true>(); den[k] = ident<true>(); });
    for (u32 u = 0; u < J.nTerms; u++) {
        const GprodTerm &T = J.t[u];
        const u64 stride = T.stride;
        const u64 *rows = (const u64 *)T.base + base * stride;
        each_item([&](auto k) { loc[k] = ident<false>(); });
        for (u32 j = 0; j + 1 < T.k; j++) {
            const E3 ap = e3_of(J.apow[T.k - 2 - j]);                            // alpha^(k - 1 - j)
            const u64 *p = rows + J.cols[T.start + j];
            each_item([&](auto k) { if (base + k < J.n) loc[k] = e3_add(loc[k], e3_scale(ap, p[k * stride])); });
        }
        {
            const u64 *p = rows + J.cols[T.start + T.k - 1];
            each_item([&](auto k) { if (base + k < J.n) loc[k].v[0] = add(loc[k].v[0], canon(p[k * stride])); });
        }
        if (T.sel) {
            const u64 ss = T.selStride;
            const u64 *p = (const u64 *)T.sel + base * ss + T.selCol;
            each_item([&](auto k) { if (base + k < J.n) loc[k] = e3_add(e3_scale(e3_sub(loc[k], beta), p[k * ss]), beta); });
        }
        if (T.id) {
            const E3 c = e3_of(T.idCoef);
            const u64 is = T.idStride;
            const u64 *p = (const u64 *)T.id + base * is + T.idCol;
            each_item([&](auto k) { if (base + k < J.n) loc[k] = e3_add(loc[k], e3_scale(c, p[k * is])); });
        }
        if (T.den) each_item([&](auto k) { if (base + k < J.n) den[k] = e3_mul(den[k], e3_add(loc[k], gamma)); });
        else each_item([&](auto k) { if (base + k < J.n) num[k] = e3_mul(num[k], e3_add(loc[k], gamma)); });
    }
    // hint_scan1's inversion: a zero D is kept out of the running product and its row's ratio is 0
    u32 zero = 0;
    E3 acc = ident<true>();
    each_item([&](auto k) {
        if (!(den[k].v[0] | den[k].v[1] | den[k].v[2])) { zero |= 1u << k; den[k] = ident<true>(); }
        loc[k] = acc;                                   // the product of the rows' D before this one
        acc = e3_mul(acc, den[k]);
    });
    E3 ai = (acc.v[1] | acc.v[2]) ? e3_inv(acc) : E3{ { inv(acc.v[0]), 0, 0 } };
    each_item_down([&](auto k) {
        const E3 di = e3_mul(ai, loc[k]);               // 1 / D_k
        ai = e3_mul(ai, den[k]);
        loc[k] = ((zero >> k) & 1) ? ident<false>() : e3_mul(num[k], di);
    });
    E3 run = ident<true>();
    each_item([&](auto k) { run = e3_mul(run, loc[k]); loc[k] = run; });        // rows at or past n hold 1 / 1
    E3 bt;
    const E3 ex = block_exclusive<true>(run, sh, &bt);
    each_item([&](auto k) { const u64 i = base + k; if (i < J.n) st3(tmp, i, e3_mul(ex, loc[k])); });
    if (threadIdx.x == 0) st3(totals, blockIdx.x, bt);
}

// every launch of a call, on st; the arguments have passed grandprodplan::check_call() and n > 0, the pointers are the device's
int gprod_fold_launch(const pil2gl_grand_prod_term *terms, u32 nTerms, const u64 *alpha, const u64 *beta, const u64 *gamma, u64 *out, u64 outStride,
                      u64 outCol, u64 n, hipStream_t st) {
    GprodJob J{};
    const u64 a[3] = { h_canon(alpha[0]), h_canon(alpha[1]), h_canon(alpha[2]) };
    const u64 b[3] = { h_canon(beta[0]), h_canon(beta[1]), h_canon(beta[2]) }, g[3] = { h_canon(gamma[0]), h_canon(gamma[1]), h_canon(gamma[2]) };
    u64 pw[tupleside::MAX_K - 1][3], cur[3] = { 1, 0, 0 };
    for (u32 e = 0; e < tupleside::MAX_K - 1; e++) {
        h_e3_mul(cur, a, pw[e]);
        for (int c = 0; c < 3; c++) cur[c] = pw[e][c];
    }
    grandprodplan::pack(terms, nTerms, pw, b, g, n, J);
    const u64 nb = hintplan::blocks(n);
    u64 *tmp, *totals;
    P2_TRY(scratch(SCR_HINT_TMP, n * 3, &tmp));
    P2_TRY(scratch(SCR_HINT_TOTALS, nb * 3, &totals));
    gprod_fold_scan1<<<(unsigned)nb, SCAN_THREADS, 0, st>>>(J, tmp, totals);
    KERNEL_CHECK();
    hint_scan2<true><<<1, SCAN_THREADS, 0, st>>>(totals, nb);
    KERNEL_CHECK();
    hint_scan3<true><<<(unsigned)((n + 255) / 256), 256, 0, st>>>(tmp, totals, n, 3, out, outStride, outCol);
    KERNEL_CHECK();
    return PIL2GL_OK;
}

int gprod_fold_check(const pil2gl_grand_prod_term *terms, u64 nTerms, const u64 *alpha, const u64 *beta, const u64 *gamma, const u64 *out, u64 outStride,
                     u64 outCol, u64 n, bool dev) {
    char why[96];
    if (const char *msg = grandprodplan::check_call(terms, nTerms, alpha, beta, gamma, out, outStride, outCol, n, 1, dev, why)) return fail(PIL2GL_EINVAL, "%s", msg);
    return PIL2GL_OK;
}

}  // namespace

extern "C" {

int pil2gl_grand_prod_plan(uint64_t n, uint64_t nTerms, uint64_t sumK, uint32_t elemWords, uint32_t *outInfo, uint64_t *workBytes) {
    if (workBytes) *workBytes = 0;
    if (const char *msg = grandprodplan::check(n, nTerms, sumK, elemWords)) return fail(PIL2GL_EINVAL, "%s", msg);
    const grandprodplan::Plan p = grandprodplan::plan(n, elemWords);
    if (outInfo) {
        outInfo[0] = p.threads; outInfo[1] = p.items; outInfo[2] = p.blocks; outInfo[3] = p.launches; outInfo[4] = p.depth;
        outInfo[5] = grandprodplan::out_width(elemWords);
    }
    if (workBytes) *workBytes = p.bytes;
    return PIL2GL_OK;
}

int pil2gl_grand_prod_dev(const pil2gl_grand_prod_term *hostTerms, uint64_t nTerms, const uint64_t *hostAlpha, const uint64_t *hostBeta,
                          const uint64_t *hostGamma, uint64_t *out, uint64_t outStride, uint64_t outCol, uint64_t n, void *stream) {
    P2_TRY(gprod_fold_check(hostTerms, nTerms, hostAlpha, hostBeta, hostGamma, out, outStride, outCol, n, true));
    if (!n) return PIL2GL_OK;
    P2_TRY(ensure_init());
    return gprod_fold_launch(hostTerms, (u32)nTerms, hostAlpha, hostBeta, hostGamma, out, outStride, outCol, n, as_stream(stream));
}

// host matrices, each staged up to the last element touched; out's matrix goes up as it is and comes back with the column written
int pil2gl_grand_prod(const pil2gl_grand_prod_term *hostTerms, uint64_t nTerms, const uint64_t *hostAlpha, const uint64_t *hostBeta,
                      const uint64_t *hostGamma, uint64_t *hostOut, uint64_t outStride, uint64_t outCol, uint64_t n) {
    P2_TRY(gprod_fold_check(hostTerms, nTerms, hostAlpha, hostBeta, hostGamma, hostOut, outStride, outCol, n, false));
    if (!n) return PIL2GL_OK;
    pil2gl_grand_prod_term terms[grandprodplan::MAX_TERMS];
    const u64 outWords = tupleside::span_bytes(n, outStride, outCol + 2, 1) / 8;
    u64 total = smapplan::pad16(outWords);
    for (u64 u = 0; u < nTerms; u++) {
        terms[u] = hostTerms[u];
        total += tupleside::staged_words(terms[u].side, n, terms[u].k, 1) + smapplan::pad16(grandprodplan::id_words(terms[u], n, 1));
    }
    Stage s(total);
    P2_TRY(s.rc());
    for (u64 u = 0; u < nTerms; u++) { tupleside::stage_side(s, terms[u].side, n, terms[u].k, 1); grandprodplan::stage_id(s, terms[u], n, 1); }
    u64 *dOut = (u64 *)s.put(hostOut, outWords);
    P2_TRY(s.rc());
    P2_TRY(gprod_fold_launch(terms, (u32)nTerms, hostAlpha, hostBeta, hostGamma, dOut, outStride, outCol, n, 0));
    return s.get(hostOut, dOut, outWords);
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------------------------------
// calculateH1H2(F, f, t)  src/helpers/polutils.js:105-126 (hint "h1h2", hints_helpers.js:115-121).
// The reference builds s = [(t[i], i)] ++ [(f[j], idx_t[f[j]])] with idx_t[v] = LAST i with t[i] = v, sorts it stably by
// the index and reads h1[i] = s[2i], h2[i] = s[2i+1].  All entries with the same index carry the same VALUE, so the
// sorted sequence is "t[i] repeated 1 + cnt[i] times, for i = 0..n-1", with cnt[i] = #{j : f[j] = t[i]} when i is the last
// occurrence of its value and 0 otherwise.  No sort is needed: a hash table value -> last index, the counts, an
// exclusive scan of (1 + cnt) for the group starts, and one binary search per output position.
namespace {

constexpr u64 H_EMPTY = ~0ull;

__device__ __forceinline__ u64 key_hash(const u64 *p, u64 i, u32 dim) { return hintplan::key_hash(p + i * dim, dim); }
__device__ __forceinline__ bool key_eq(const u64 *a, u64 i, const u64 *b, u64 j, u32 dim) {
    for (u32 k = 0; k < dim; k++) if (a[i * dim + k] != b[j * dim + k]) return false;
    return true;
}
__global__ void h1h2_insert(const u64 *__restrict__ t, u64 n, u32 dim, unsigned long long *__restrict__ table, u64 mask) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    u64 s = key_hash(t, i, dim) & mask;
    for (;;) {
        unsigned long long cur = table[s];
        if (cur == H_EMPTY) {
            cur = atomicCAS(&table[s], (unsigned long long)H_EMPTY, (unsigned long long)i);
            if (cur == H_EMPTY) return;                          // claimed the slot
        }
        if (key_eq(t, i, t, cur, dim)) { atomicMax(&table[s], (unsigned long long)i); return; }   // same value: keep the last index
        s = (s + 1) & mask;
    }
}
__global__ void h1h2_count(const u64 *__restrict__ f, const u64 *__restrict__ t, u64 n, u32 dim, const unsigned long long *__restrict__ table, u64 mask,
                           unsigned long long *__restrict__ cnt, unsigned long long *__restrict__ missing) {
    const u64 j = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    u64 s = key_hash(f, j, dim) & mask;
    for (;;) {
        const unsigned long long cur = table[s];
        if (cur == H_EMPTY) { atomicMin(missing, (unsigned long long)j); return; }      // "Number not included" (polutils.js:115)
        if (key_eq(f, j, t, cur, dim)) { atomicAdd(&cnt[cur], 1ull); return; }
        s = (s + 1) & mask;
    }
}
// in: cnt[i];  out: start[i] = sum_{k<i} (1 + cnt[k])  -- block-local exclusive scan + block totals (u64 adds)
__global__ void __launch_bounds__(SCAN_THREADS) h1h2_scan1(const unsigned long long *__restrict__ cnt, u64 n, u64 *__restrict__ start, u64 *__restrict__ totals) {
    __shared__ u64 sh[SCAN_THREADS];
    const u64 base = (u64)blockIdx.x * SCAN_CHUNK + (u64)threadIdx.x * SCAN_ITEMS;
    u64 loc[SCAN_ITEMS], run = 0;
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; k++) { const u64 i = base + k; loc[k] = run; if (i < n) run += 1 + cnt[i]; }
    sh[threadIdx.x] = run;
    __syncthreads();
    for (u32 d = 1; d < SCAN_THREADS; d <<= 1) {
        u64 v = sh[threadIdx.x];
        if (threadIdx.x >= d) v += sh[threadIdx.x - d];
        __syncthreads();
        sh[threadIdx.x] = v;
        __syncthreads();
    }
    const u64 ex = threadIdx.x ? sh[threadIdx.x - 1] : 0;
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; k++) { const u64 i = base + k; if (i < n) start[i] = ex + loc[k]; }
    if (threadIdx.x == SCAN_THREADS - 1) totals[blockIdx.x] = sh[SCAN_THREADS - 1];
}
__global__ void h1h2_scan2(u64 *__restrict__ totals, u64 nb) {           // tiny: one thread
    if (blockIdx.x || threadIdx.x) return;
    u64 run = 0;
    for (u64 b = 0; b < nb; b++) { const u64 v = totals[b]; totals[b] = run; run += v; }
}
__global__ void h1h2_scan3(u64 *__restrict__ start, const u64 *__restrict__ totals, u64 n) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) start[i] += totals[i / SCAN_CHUNK];
}
// output position p in [0, 2n): its group is the last i with start[i] <= p
__global__ void h1h2_expand(const u64 *__restrict__ t, const u64 *__restrict__ start, u64 n, u32 dim, u64 *__restrict__ h1, u64 *__restrict__ h2) {
    const u64 p = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= 2 * n) return;
    u64 lo = 0, hi = n - 1;
    while (lo < hi) { const u64 mid = (lo + hi + 1) >> 1; if (start[mid] <= p) lo = mid; else hi = mid - 1; }
    u64 *o = (p & 1) ? h2 : h1;
    for (u32 k = 0; k < dim; k++) o[(p >> 1) * dim + k] = t[lo * dim + k];
}

}  // namespace

extern "C" int pil2gl_h1h2_dev(const uint64_t *f, const uint64_t *t, uint64_t n, uint32_t dim, uint64_t *h1, uint64_t *h2, void *stream) {
    P2_TRY(ensure_init());
    if (n == 0) return PIL2GL_OK;
    if (!f || !t || !h1 || !h2) return fail(PIL2GL_EINVAL, "null buffer");
    if (dim != 1 && dim != 3) return fail(PIL2GL_EINVAL, "dimension must be 1 or 3");
    if (n > hintplan::H1H2_MAX_N) return fail(PIL2GL_EINVAL, "column too long");
    hipStream_t st = as_stream(stream);
    const hintplan::H1H2Work w = hintplan::h1h2_work(n);  // table[cap] | cnt[n] | start[n] | totals[nb] | missing[1]
    const u64 cap = w.capacity, nb = hintplan::blocks(n);
    u64 *ws;
    P2_TRY(scratch(SCR_HINT_WORK, w.words, &ws));
    unsigned long long *table = (unsigned long long *)(ws + w.offTable), *cnt = (unsigned long long *)(ws + w.offCnt);
    u64 *start = ws + w.offStart, *totals = ws + w.offTotals;
    unsigned long long *missing = (unsigned long long *)(ws + w.offMissing);
    HIP_TRY(hipMemsetAsync(table, 0xFF, cap * 8, st));
    HIP_TRY(hipMemsetAsync(cnt, 0, n * 8, st));
    HIP_TRY(hipMemsetAsync(missing, 0xFF, 8, st));
    const unsigned g = (unsigned)((n + 255) / 256);
    h1h2_insert<<<g, 256, 0, st>>>(t, n, dim, table, cap - 1);
    KERNEL_CHECK();
    h1h2_count<<<g, 256, 0, st>>>(f, t, n, dim, table, cap - 1, cnt, missing);
    KERNEL_CHECK();
    h1h2_scan1<<<(unsigned)nb, SCAN_THREADS, 0, st>>>(cnt, n, start, totals);
    KERNEL_CHECK();
    h1h2_scan2<<<1, 1, 0, st>>>(totals, nb);
    KERNEL_CHECK();
    h1h2_scan3<<<g, 256, 0, st>>>(start, totals, n);
    KERNEL_CHECK();
    h1h2_expand<<<(unsigned)((2 * n + 255) / 256), 256, 0, st>>>(t, start, n, dim, h1, h2);
    KERNEL_CHECK();
    unsigned long long miss = 0;
    HIP_TRY(hipMemcpyAsync(&miss, missing, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (miss != H_EMPTY) return fail(PIL2GL_EINVAL, "Number not included: w:%llu", miss);     // polutils.js:115
    return PIL2GL_OK;
}

extern "C" {

int pil2gl_debug_hint_plan(uint64_t n, uint32_t *outInfo) {
    const u64 nb = hintplan::blocks(n);
    if (nb > 0x7fffffffull) return fail(PIL2GL_EINVAL, "grid too large");
    if (outInfo) {
        outInfo[0] = SCAN_THREADS; outInfo[1] = SCAN_ITEMS; outInfo[2] = SCAN_CHUNK; outInfo[3] = (uint32_t)nb;
        outInfo[4] = (uint32_t)hintplan::totals_per_lane(nb);
        outInfo[5] = n <= hintplan::H1H2_MAX_N ? hintplan::h1h2_capacity_bits(n) : 0;
    }
    return PIL2GL_OK;
}

uint64_t pil2gl_debug_h1h2_home(const uint64_t *words, uint32_t dim, uint64_t capacity) {
    if (!words || (dim != 1 && dim != 3) || !capacity || (capacity & (capacity - 1))) return hintplan::NONE;
    return hintplan::h1h2_home(words, dim, capacity);
}

}  // extern "C"
