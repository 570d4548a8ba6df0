// Stage-2 witness hints on the device: the grand product / grand sum columns
//   calculateZ(F,num,den)  src/helpers/polutils.js:128-143   z[0] = 1, z[i] = z[i-1] * num[i-1] / den[i-1]
//   calculateS(F,num,den)  src/helpers/polutils.js:145-164   s[i] = s[i-1] + num / den[i]        (num: one element)
// called from resolveHint (src/prover/hints_helpers.js:91-114).  The reference walks the column serially with BigInt
// arithmetic after one batch inversion; here a thread inverts its eight denominators together (one field inversion per
// eight rows) and the running product / sum is a three-kernel scan: per-block inclusive scan + block totals, scan of the
// totals, then the fix-up (for the product: shifted by one row, z[0] = 1).  Operands may be base (dim 1) or cubic
// extension (dim 3) columns, row-major; the result is dim 3 if either operand is, else dim 1.  gsum_col is the sum with a column
// numerator; the lookup grand sum further down folds a lookup's sides into the sum's first pass, the grand product behind it a
// permutation's or a connection's terms into the product's, and the plookup section behind that pil1's plookup argument.
#include "common.h"
#include "gl_field.cuh"
#include "hint_plan.h"
#include "logup_sum_plan.h"
#include "range_sum_plan.h"
#include "logup_cluster_plan.h"
#include "grand_prod_plan.h"
#include "plookup_plan.h"
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

// the f terms of a lane's rows folded into its fractions num / den (den never zero; rows at or past n stay as they are).  The terms are the
// outer loop, so that a term's table entries are read once for the lane's rows and the rows' loads of one column are in flight together.
// Job: a kernel argument with t[], nTerms, apow[] and n, read with wave-uniform indices.  keep(u): whether term u takes part (cluster_scan1
// folds one cluster at a time; the other two passes fold every term)
struct EveryTerm { __device__ __forceinline__ bool operator()(u32) const { return true; } };
template <class Job, class Keep = EveryTerm>
__device__ __forceinline__ void logup_fold(const Job &J, u64 base, E3 (&num)[SCAN_ITEMS], E3 (&den)[SCAN_ITEMS], E3 (&loc)[SCAN_ITEMS], Keep keep = Keep{}) {
    for (u32 u = 0; u < J.nTerms; u++) {
        if (!keep(u)) continue;
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
            if (i >= J.n || !(d.v[0] | d.v[1] | d.v[2])) return;               // a zero D_u: the term adds 0 and is left out of the product
            const u64 c = T.sel ? mul(T.sel[i * T.selStride + T.selCol], T.coef) : T.coef;
            num[k] = e3_add(e3_mul(num[k], d), e3_scale(den[k], c));
            den[k] = e3_mul(den[k], d);
        });
    }
}
// the lane's fractions to ratios in loc with one inversion
__device__ __forceinline__ void logup_ratios(E3 (&num)[SCAN_ITEMS], E3 (&den)[SCAN_ITEMS], E3 (&loc)[SCAN_ITEMS]) {
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
}
// the running sum of the lane's ratios in loc, the block-local scan into tmp and the block's total
__device__ __forceinline__ void logup_tail(E3 (&loc)[SCAN_ITEMS], E3 *sh, u64 base, u64 n, u64 *__restrict__ tmp, u64 *__restrict__ totals) {
    E3 run = ident<false>();
    each_item([&](auto k) { run = e3_add(run, loc[k]); loc[k] = run; });      // rows at or past n hold num = 0
    E3 bt;
    const E3 ex = block_exclusive<false>(run, sh, &bt);
    each_item([&](auto k) { const u64 i = base + k; if (i < n) st3(tmp, i, e3_add(ex, loc[k])); });
    if (threadIdx.x == 0) st3(totals, blockIdx.x, bt);
}
__device__ __forceinline__ void logup_finish(E3 (&num)[SCAN_ITEMS], E3 (&den)[SCAN_ITEMS], E3 (&loc)[SCAN_ITEMS], E3 *sh, u64 base, u64 n,
                                             u64 *__restrict__ tmp, u64 *__restrict__ totals) {
    logup_ratios(num, den, loc);
    logup_tail(loc, sh, base, n, tmp, totals);
}

__global__ void __launch_bounds__(SCAN_THREADS) logup_scan1(const LogupJob J, u64 *__restrict__ tmp, u64 *__restrict__ totals) {
    __shared__ E3 sh[SCAN_THREADS];
    const u64 base = (u64)blockIdx.x * SCAN_CHUNK + (u64)threadIdx.x * SCAN_ITEMS;
    // the lane's rows as fractions num / den, den never zero; rows at or past n stay 0 / 1
    E3 num[SCAN_ITEMS], den[SCAN_ITEMS], loc[SCAN_ITEMS];
    each_item([&](auto k) { num[k] = ident<false>(); den[k] = ident<true>(); });
    logup_fold(J, base, num, den, loc);
    logup_finish(num, den, loc, sh, base, J.n, tmp, totals);
}

u64 h_canon(u64 a) { return a >= P ? a - P : a; }

// every launch of a call, on st; the arguments have passed logupplan::check_call() and n > 0, the pointers are the device's
// the f terms of a job (logup_scan1's, range_scan1's): the powers of alpha, each term's table entry with busId + beta
template <class Job>
void logup_fill(Job &J, const pil2gl_logup_term *terms, u32 nTerms, const u64 *alpha, const u64 *beta, u64 n) {
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
}

int logup_launch(const pil2gl_logup_term *terms, u32 nTerms, const u64 *alpha, const u64 *beta, u64 *out, u64 outStride, u64 outCol, u64 n, hipStream_t st) {
    LogupJob J{};
    logup_fill(J, terms, nTerms, alpha, beta, n);
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
// The range-check grand sum (include/pil2gl.h states it; tests/range_sum_ref.py restates it over integers): the lookup grand sum above
// with the table side of a range given as numbers,
//   s[i] = s[i-1] + sum_u coef_u w_u[i] / D_u[i] + sum_r coefR_r [row0_r <= i < row0_r + size_r] m_r[i] / E_r[i],
//   E_r[i] = field(lo_r + (i - row0_r)) alpha + busId_r + beta.
// One fused first pass, range_scan1, beside logup_scan1, sharing its fold of the f terms (logup_fold) and its tail (logup_finish); then
// hint_scan2<false> and hint_scan3<false> as they are.  A range is an arithmetic progression in the extension: with c0 = alpha field(lo) +
// busId + beta made on the host, E at the lane's first in-window row is c0 + alpha (row - row0) -- ONE scaling of alpha by a base value, three
// base products a lane -- and every next row's is E + alpha, an extension addition.  No t column exists; m is loaded only inside the window
// (into loc, which the fold does not need meanwhile), so a range-row costs one 8-byte load where logup_scan1's k = 1 term costs two, and
// 16 base products (coef m, the two extension products and the scaling of the fold) + 3/8 where that term costs 16 + 3.
// The ranges are the outer loop, as the terms are in logup_fold.  Both tables travel as the kernel argument.
// Safety: nothing read from a matrix is used as an address; m is loaded at row i only after row0 <= i < row0 + size <= n.
namespace {

struct RangeTermD {
    const u64 *m;
    u64 stride, col, row0, end;                      // the window: rows row0 .. end - 1
    u64 coef;
    E3 c0;                                           // alpha field(lo) + busId + beta
};
struct RangeJob {
    LogupTerm t[rangesumplan::MAX_F];
    E3 apow[tupleside::MAX_K + 1];                   // apow[e] = alpha^e, e = 1 .. 16
    RangeTermD r[rangesumplan::MAX_RANGES];
    u32 nTerms, nRanges;                             // nTerms: the f terms, 0 .. 8
    u64 n;
};

// the ranges of a lane's rows folded into its fractions, as logup_fold folds the f terms.  Job: with r[], nRanges and apow[] besides;
// keep(r): whether range r takes part
template <class Job, class Keep = EveryTerm>
__device__ __forceinline__ void range_fold(const Job &J, u64 base, E3 (&num)[SCAN_ITEMS], E3 (&den)[SCAN_ITEMS], E3 (&loc)[SCAN_ITEMS], Keep keep = Keep{}) {
    const E3 alpha = J.apow[1];
    for (u32 r = 0; r < J.nRanges; r++) {
        if (!keep(r)) continue;
        const RangeTermD &T = J.r[r];
        const u64 row0 = T.row0, end = T.end, coef = T.coef;
        const u64 first = base > row0 ? base : row0;                            // the lane's first in-window row, if it has one
        const u64 *p = T.m + base * T.stride + T.col;
        each_item([&](auto k) { const u64 i = base + k; if (i >= first && i < end) loc[k].v[0] = p[k * T.stride]; });     // end <= n
        E3 e = e3_add(T.c0, e3_scale(alpha, first - row0));                      // first - row0 < 2^28: a base value
        each_item([&](auto k) {
            const u64 i = base + k;
            if (i < first || i >= end) return;
            const E3 d = e;
            e = e3_add(e, alpha);                                                // the next row's, whether this one is zero or not
            if (!(d.v[0] | d.v[1] | d.v[2])) return;                             // a zero E_r: the range adds 0 and is left out of the product
            num[k] = e3_add(e3_mul(num[k], d), e3_scale(den[k], mul(loc[k].v[0], coef)));
            den[k] = e3_mul(den[k], d);
        });
    }
}

__global__ void __launch_bounds__(SCAN_THREADS) range_scan1(const RangeJob J, u64 *__restrict__ tmp, u64 *__restrict__ totals) {
    __shared__ E3 sh[SCAN_THREADS];
    const u64 base = (u64)blockIdx.x * SCAN_CHUNK + (u64)threadIdx.x * SCAN_ITEMS;
    E3 num[SCAN_ITEMS], den[SCAN_ITEMS], loc[SCAN_ITEMS];
    each_item([&](auto k) { num[k] = ident<false>(); den[k] = ident<true>(); });
    logup_fold(J, base, num, den, loc);
    range_fold(J, base, num, den, loc);
    logup_finish(num, den, loc, sh, base, J.n, tmp, totals);
}

// a job's ranges: each range's table entry with its host-made constant
template <class Job>
void range_fill(Job &J, const pil2gl_range_term *ranges, u32 nR, const u64 *alpha, const u64 *beta) {
    const u64 a[3] = { h_canon(alpha[0]), h_canon(alpha[1]), h_canon(alpha[2]) }, b[3] = { h_canon(beta[0]), h_canon(beta[1]), h_canon(beta[2]) };
    for (u32 r = 0; r < nR; r++) {
        const pil2gl_range_term &R = ranges[r];
        RangeTermD &T = J.r[r];
        T.m = R.m; T.stride = R.mStride; T.col = R.mCol; T.row0 = R.row0; T.end = R.row0 + R.size; T.coef = R.coef[0];
        rangesumplan::gl_c0(R, a, b, h_mul, h_add, T.c0.v);
    }
    J.nRanges = nR;
}

// every launch of a call, on st; the arguments have passed rangesumplan::check_call() and n > 0, the pointers are the device's
int range_sum_launch(const pil2gl_logup_term *terms, u32 nF, const pil2gl_range_term *ranges, u32 nR, const u64 *alpha, const u64 *beta, u64 *out,
                     u64 outStride, u64 outCol, u64 n, hipStream_t st) {
    RangeJob J{};
    logup_fill(J, terms, nF, alpha, beta, n);
    range_fill(J, ranges, nR, alpha, beta);
    const u64 nb = hintplan::blocks(n);
    u64 *tmp, *totals;
    P2_TRY(scratch(SCR_HINT_TMP, n * 3, &tmp));
    P2_TRY(scratch(SCR_HINT_TOTALS, nb * 3, &totals));
    range_scan1<<<(unsigned)nb, SCAN_THREADS, 0, st>>>(J, tmp, totals);
    KERNEL_CHECK();
    hint_scan2<false><<<1, SCAN_THREADS, 0, st>>>(totals, nb);
    KERNEL_CHECK();
    hint_scan3<false><<<(unsigned)((n + 255) / 256), 256, 0, st>>>(tmp, totals, n, 3, out, outStride, outCol);
    KERNEL_CHECK();
    return PIL2GL_OK;
}

int range_sum_check(const pil2gl_logup_term *terms, u64 nF, const pil2gl_range_term *ranges, u64 nR, const u64 *alpha, const u64 *beta, const u64 *out,
                    u64 outStride, u64 outCol, u64 n, bool dev) {
    char why[96];
    if (const char *msg = rangesumplan::check_call(terms, nF, ranges, nR, alpha, beta, out, outStride, outCol, n, 1, dev, why)) return fail(PIL2GL_EINVAL, "%s", msg);
    return PIL2GL_OK;
}

}  // namespace

extern "C" {

int pil2gl_range_sum_plan(uint64_t n, uint64_t nF, uint64_t nR, uint32_t elemWords, uint32_t *outInfo, uint64_t *workBytes) {
    if (workBytes) *workBytes = 0;
    if (const char *msg = rangesumplan::check(n, nF, nR, elemWords)) return fail(PIL2GL_EINVAL, "%s", msg);
    const rangesumplan::Plan p = rangesumplan::plan(n, elemWords);
    if (outInfo) {
        outInfo[0] = p.threads; outInfo[1] = p.items; outInfo[2] = p.blocks; outInfo[3] = p.launches; outInfo[4] = p.depth;
        outInfo[5] = logupplan::out_width(elemWords);
    }
    if (workBytes) *workBytes = p.bytes;
    return PIL2GL_OK;
}

int pil2gl_range_sum_dev(const pil2gl_logup_term *hostTerms, uint64_t nF, const pil2gl_range_term *hostRanges, uint64_t nR, const uint64_t *hostAlpha,
                         const uint64_t *hostBeta, uint64_t *out, uint64_t outStride, uint64_t outCol, uint64_t n, void *stream) {
    P2_TRY(range_sum_check(hostTerms, nF, hostRanges, nR, hostAlpha, hostBeta, out, outStride, outCol, n, true));
    if (!n) return PIL2GL_OK;
    P2_TRY(ensure_init());
    return range_sum_launch(hostTerms, (u32)nF, hostRanges, (u32)nR, hostAlpha, hostBeta, out, outStride, outCol, n, as_stream(stream));
}

// host matrices, each staged up to the last element touched (an m up to its window's last row); out's matrix goes up as it is and comes back
// with the column written
int pil2gl_range_sum(const pil2gl_logup_term *hostTerms, uint64_t nF, const pil2gl_range_term *hostRanges, uint64_t nR, const uint64_t *hostAlpha,
                     const uint64_t *hostBeta, uint64_t *hostOut, uint64_t outStride, uint64_t outCol, uint64_t n) {
    P2_TRY(range_sum_check(hostTerms, nF, hostRanges, nR, hostAlpha, hostBeta, hostOut, outStride, outCol, n, false));
    if (!n) return PIL2GL_OK;
    pil2gl_logup_term terms[rangesumplan::MAX_F];
    pil2gl_range_term ranges[rangesumplan::MAX_RANGES];
    const u64 outWords = tupleside::span_bytes(n, outStride, outCol + 2, 1) / 8;
    u64 total = smapplan::pad16(outWords);
    for (u64 u = 0; u < nF; u++) { terms[u] = hostTerms[u]; total += tupleside::staged_words(terms[u].side, n, terms[u].k, 1); }
    for (u64 r = 0; r < nR; r++) { ranges[r] = hostRanges[r]; total += smapplan::pad16(rangesumplan::m_words(ranges[r], 1)); }
    Stage s(total);
    P2_TRY(s.rc());
    for (u64 u = 0; u < nF; u++) tupleside::stage_side(s, terms[u].side, n, terms[u].k, 1);
    for (u64 r = 0; r < nR; r++) {
        const u64 w = rangesumplan::m_words(ranges[r], 1);
        ranges[r].m = s.put(ranges[r].m, w); s.take(smapplan::pad16(w) - w);
    }
    u64 *dOut = (u64 *)s.put(hostOut, outWords);
    P2_TRY(s.rc());
    P2_TRY(range_sum_launch(terms, (u32)nF, ranges, (u32)nR, hostAlpha, hostBeta, dOut, outStride, outCol, n, 0));
    return s.get(hostOut, dOut, outWords);
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------------------------------
// The clustered logUp sum (include/pil2gl.h states it; tests/logup_cluster_ref.py restates it over integers): the two sums above with the
// terms gathered into clusters, each cluster's part of a row written as a column of its own,
//   im_c[i] = sum_{cluster[u] = c} frac_u[i],     s[i] = s[i-1] + sum_c im_c[i] + sum_{cluster[u] = DIRECT} frac_u[i].
// One fused first pass, cluster_scan1, beside logup_scan1 and range_scan1; then hint_scan2<false> and hint_scan3<false> as they are.  The
// GROUPS are the outer loop -- the clusters 0 .. nIm - 1, then the DIRECT terms if there are any.  For a group the lane folds the group's
// terms of its SCAN_ITEMS rows into fractions num / den with logup_fold and range_fold (a zero denominator is left out, so den is never
// zero), turns them into ratios with ONE e3_inv (logup_ratios), stores them as im_c unless the group is the DIRECT one, and adds them into
// a per-row accumulator; logup_tail then runs the sum over the accumulator.  A row's terms are each folded once, as in the passes above:
// what the im columns add is an e3_inv a lane-group where those passes have one a lane, the ratio's products a group-row, and 24 bytes
// stored a cluster-row.  The cluster ids travel in the kernel argument and are read with wave-uniform indices.
// Safety: nothing read from a matrix is used as an address; a row index is checked against n before any load or store.
namespace {

using logupclusterplan::MAX_GROUPS;

struct ImColD { u64 *base; u64 stride, col; };
struct ClusterJob : RangeJob {
    ImColD im[logupclusterplan::MAX_IM];
    u32 group[MAX_TERMS];                            // the group of term u (f terms, then ranges): its cluster, or nIm for a DIRECT term
    u32 nIm, nGroups;                                // nGroups: nIm, + 1 with a DIRECT term.  Every group has a term
};

__global__ void __launch_bounds__(SCAN_THREADS) cluster_scan1(const ClusterJob J, u64 *__restrict__ tmp, u64 *__restrict__ totals) {
    __shared__ E3 sh[SCAN_THREADS];
    const u64 base = (u64)blockIdx.x * SCAN_CHUNK + (u64)threadIdx.x * SCAN_ITEMS;
    E3 num[SCAN_ITEMS], den[SCAN_ITEMS], loc[SCAN_ITEMS], sum[SCAN_ITEMS];
    each_item([&](auto k) { sum[k] = ident<false>(); });
    for (u32 g = 0; g < J.nGroups; g++) {
        each_item([&](auto k) { num[k] = ident<false>(); den[k] = ident<true>(); });      // every row anew: a group starts from 0 / 1
        logup_fold(J, base, num, den, loc, [&](u32 u) { return J.group[u] == g; });
        range_fold(J, base, num, den, loc, [&](u32 r) { return J.group[J.nTerms + r] == g; });
        logup_ratios(num, den, loc);                    // rows at or past n hold 0 / 1: ratio 0
        if (g < J.nIm) {
            const ImColD &C = J.im[g];
            u64 *p = C.base + base * C.stride + C.col;
            each_item([&](auto k) {
                if (base + k >= J.n) return;
                u64 *o = p + k * C.stride;
                o[0] = loc[k].v[0]; o[1] = loc[k].v[1]; o[2] = loc[k].v[2];
            });
        }
        each_item([&](auto k) { sum[k] = e3_add(sum[k], loc[k]); });
    }
    logup_tail(sum, sh, base, J.n, tmp, totals);
}

// every launch of a call, on st; the arguments have passed logupclusterplan::check_call() and n > 0, the pointers are the device's
int cluster_launch(const pil2gl_logup_term *terms, u32 nF, const pil2gl_range_term *ranges, u32 nR, const u64 *cluster, const pil2gl_logup_im_col *im,
                   u32 nIm, const u64 *alpha, const u64 *beta, u64 *out, u64 outStride, u64 outCol, u64 n, hipStream_t st) {
    ClusterJob J{};
    logup_fill(J, terms, nF, alpha, beta, n);
    range_fill(J, ranges, nR, alpha, beta);
    J.nIm = J.nGroups = nIm;
    for (u32 u = 0; u < nF + nR; u++) {
        J.group[u] = cluster[u] == logupclusterplan::DIRECT ? nIm : (u32)cluster[u];
        if (J.group[u] == nIm) J.nGroups = nIm + 1;
    }
    for (u32 c = 0; c < nIm; c++) J.im[c] = ImColD{ im[c].base, im[c].stride, im[c].col };
    const u64 nb = hintplan::blocks(n);
    u64 *tmp, *totals;
    P2_TRY(scratch(SCR_HINT_TMP, n * 3, &tmp));
    P2_TRY(scratch(SCR_HINT_TOTALS, nb * 3, &totals));
    cluster_scan1<<<(unsigned)nb, SCAN_THREADS, 0, st>>>(J, tmp, totals);
    KERNEL_CHECK();
    hint_scan2<false><<<1, SCAN_THREADS, 0, st>>>(totals, nb);
    KERNEL_CHECK();
    hint_scan3<false><<<(unsigned)((n + 255) / 256), 256, 0, st>>>(tmp, totals, n, 3, out, outStride, outCol);
    KERNEL_CHECK();
    return PIL2GL_OK;
}

int cluster_check(const pil2gl_logup_term *terms, u64 nF, const pil2gl_range_term *ranges, u64 nR, const u64 *cluster, const pil2gl_logup_im_col *im, u64 nIm,
                  const u64 *alpha, const u64 *beta, const u64 *out, u64 outStride, u64 outCol, u64 n, bool dev) {
    char why[96];
    if (const char *msg = logupclusterplan::check_call(terms, nF, ranges, nR, cluster, im, nIm, alpha, beta, out, outStride, outCol, n, 1, dev, why))
        return fail(PIL2GL_EINVAL, "%s", msg);
    return PIL2GL_OK;
}

}  // namespace

extern "C" {

int pil2gl_logup_cluster_plan(uint64_t n, uint64_t nF, uint64_t nR, uint64_t nIm, uint32_t elemWords, uint32_t *outInfo, uint64_t *workBytes) {
    if (workBytes) *workBytes = 0;
    if (const char *msg = logupclusterplan::check(n, nF, nR, nIm, elemWords)) return fail(PIL2GL_EINVAL, "%s", msg);
    const logupclusterplan::Plan p = logupclusterplan::plan(n, elemWords);
    if (outInfo) {
        outInfo[0] = p.threads; outInfo[1] = p.items; outInfo[2] = p.blocks; outInfo[3] = p.launches; outInfo[4] = p.depth;
        outInfo[5] = logupplan::out_width(elemWords);
    }
    if (workBytes) *workBytes = p.bytes;
    return PIL2GL_OK;
}

int pil2gl_logup_cluster_dev(const pil2gl_logup_term *hostTerms, uint64_t nF, const pil2gl_range_term *hostRanges, uint64_t nR, const uint64_t *hostCluster,
                             const pil2gl_logup_im_col *hostIm, uint64_t nIm, const uint64_t *hostAlpha, const uint64_t *hostBeta, uint64_t *out,
                             uint64_t outStride, uint64_t outCol, uint64_t n, void *stream) {
    P2_TRY(cluster_check(hostTerms, nF, hostRanges, nR, hostCluster, hostIm, nIm, hostAlpha, hostBeta, out, outStride, outCol, n, true));
    if (!n) return PIL2GL_OK;
    P2_TRY(ensure_init());
    return cluster_launch(hostTerms, (u32)nF, hostRanges, (u32)nR, hostCluster, hostIm, (u32)nIm, hostAlpha, hostBeta, out, outStride, outCol, n, as_stream(stream));
}

// host matrices: logupclusterplan::host_form stages them, the read ones as range_sum's, every distinct output matrix as it is
int pil2gl_logup_cluster(const pil2gl_logup_term *hostTerms, uint64_t nF, const pil2gl_range_term *hostRanges, uint64_t nR, const uint64_t *hostCluster,
                         const pil2gl_logup_im_col *hostIm, uint64_t nIm, const uint64_t *hostAlpha, const uint64_t *hostBeta, uint64_t *hostOut,
                         uint64_t outStride, uint64_t outCol, uint64_t n) {
    P2_TRY(cluster_check(hostTerms, nF, hostRanges, nR, hostCluster, hostIm, nIm, hostAlpha, hostBeta, hostOut, outStride, outCol, n, false));
    if (!n) return PIL2GL_OK;
    return logupclusterplan::host_form<Stage>(hostTerms, nF, hostRanges, nR, hostIm, nIm, hostOut, outStride, outCol, n, 1,
        [&](const pil2gl_logup_term *t, const pil2gl_range_term *r, const pil2gl_logup_im_col *im, u64 *dOut) {
            return cluster_launch(t, (u32)nF, r, (u32)nR, hostCluster, im, (u32)nIm, hostAlpha, hostBeta, dOut, outStride, outCol, n, 0);
        });
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
// The plookup argument of pil1 (include/pil2gl.h states it; tests/plookup_ref.py restates it over integers):
//   T = H_t or (H_t - beta) selT + beta,   F = H_f or (H_f - T) selF + T,   g = gamma (1 + delta),
//   num[i] = (F[i] + gamma) (T[i] + delta T[i+1] + g) (1 + delta),   den[i] = (h1[i] + delta h2[i] + g) (h2[i] + delta h1[i+1] + g),
//   z[0] = 1, z[i] = z[i-1] num[i-1] / den[i-1],   row n - 1's neighbour is row 0.
// The fold (stage 1) is one kernel, a lane a row, that writes F and T for h1h2.  The product (stage 2) is one fused first pass beside
// gprod_fold_scan1, then hint_scan2<true> and hint_scan3<true> as they are.  A lane takes its SCAN_ITEMS rows and needs T and h1 at nine:
// its eight and the row behind them -- the next lane's first, the next block's first, or row 0 behind row n - 1.  The ninth T is computed
// from the trace like the others (k more loads a lane; no exchange through LDS, which would put a barrier between the loads and the
// products).  N and D of a row are built in registers, the eight D inverted together, a zero D inverting to zero as in hint_scan1, so that a
// zero den factor gives ratio 0; then the block-local product scan into tmp.  Neither num nor den is ever a column.
// Base products a row: 3 (k - 1) a side for H (9/8 of that for t), 3 a selector, 6 for delta T', 6 + 6 for N, 2 x 3 (hDim 1) or 2 x 6
// (hDim 3) for delta h, 6 for D; then gprod_fold_scan1's 18 + 6 + 6 and 1/8 of the lane's e3_inv.
// The job (plookup_plan.h) travels as a kernel argument and is read with wave-uniform indices.
// Safety: nothing read from a matrix is used as an address; a row index is below n before any load (the ninth row is base + 8 < n, or 0).
namespace {

typedef plookupplan::Side PlSide;
typedef plookupplan::HCol PlCol;
typedef plookupplan::GlJob PlJob;
typedef plookupplan::Column PlColumn;

constexpr int PL_ROWS = SCAN_ITEMS + 1;

// the side's H at ROWS rows r[k] (ok[k]: the row exists) and, with a selector, its blend towards to(k); a row that is not there stays 0
template <int ROWS, class To>
__device__ __forceinline__ void pl_side(const PlSide &S, const PlJob &J, const u64 (&r)[PL_ROWS], const bool (&ok)[PL_ROWS], E3 (&v)[ROWS], To to) {
    const std::make_integer_sequence<int, ROWS> rows{};
    const u64 stride = S.stride;
    const u64 *m = (const u64 *)S.base;
    each_item([&](auto k) { v[k] = ident<false>(); }, rows);
    // the columns are the outer loop: a column's loads of the lane's rows are in flight together
    for (u32 j = 0; j + 1 < S.k; j++) {
        const E3 ap = e3_of(J.apow[S.k - 2 - j]);                                // alpha^(k - 1 - j)
        const u64 *p = m + S.cols[j];
        each_item([&](auto k) { if (ok[k]) v[k] = e3_add(v[k], e3_scale(ap, p[r[k] * stride])); }, rows);
    }
    {
        const u64 *p = m + S.cols[S.k - 1];
        each_item([&](auto k) { if (ok[k]) v[k].v[0] = add(v[k].v[0], canon(p[r[k] * stride])); }, rows);
    }
    if (S.sel) {
        const u64 ss = S.selStride;
        const u64 *p = (const u64 *)S.sel + S.selCol;
        each_item([&](auto k) { if (ok[k]) { const E3 b = to(k); v[k] = e3_add(e3_scale(e3_sub(v[k], b), p[r[k] * ss]), b); } }, rows);
    }
}

__device__ __forceinline__ E3 pl_h(const PlCol &c, u32 hDim, u64 row) {
    const u64 *p = (const u64 *)c.base + row * c.stride + c.col;
    return hDim == 3 ? E3{ { canon(p[0]), canon(p[1]), canon(p[2]) } } : E3{ { canon(p[0]), 0, 0 } };
}
// delta x, x an h element: a scaling when h is a base column
__device__ __forceinline__ E3 pl_dh(const E3 &delta, const E3 &x, u32 hDim) { return hDim == 3 ? e3_mul(delta, x) : e3_scale(delta, x.v[0]); }

__global__ void __launch_bounds__(SCAN_THREADS) plookup_fold_scan1(const PlJob J, u64 *__restrict__ tmp, u64 *__restrict__ totals) {
    __shared__ E3 sh[SCAN_THREADS];
    const u64 base = (u64)blockIdx.x * SCAN_CHUNK + (u64)threadIdx.x * SCAN_ITEMS, n = J.n;
    const std::make_integer_sequence<int, PL_ROWS> nine{};
    // the lane's rows and the row behind them; past row n - 1 comes row 0
    u64 r[PL_ROWS];
    bool ok[PL_ROWS];
    each_item([&](auto k) { r[k] = base + k; ok[k] = base + k < n; });
    r[SCAN_ITEMS] = base + SCAN_ITEMS < n ? base + SCAN_ITEMS : 0;
    ok[SCAN_ITEMS] = true;
    const E3 beta = e3_of(J.beta), gamma = e3_of(J.gamma), delta = e3_of(J.delta), g = e3_of(J.g), opd = e3_of(J.onePlusDelta);
    E3 tv[PL_ROWS], num[SCAN_ITEMS], den[SCAN_ITEMS], loc[SCAN_ITEMS];
    pl_side(J.t, J, r, ok, tv, [&](auto) { return beta; });
    pl_side(J.f, J, r, ok, num, [&](auto k) { return tv[k]; });                // F: blended towards T of the same row
    each_item([&](auto k) {
        if (!ok[k]) { num[k] = ident<true>(); return; }                         // rows at or past n stay 1 / 1
        E3 tn = tv[SCAN_ITEMS];
        if constexpr (decltype(k)::value + 1 < SCAN_ITEMS) { if (ok[k + 1]) tn = tv[k + 1]; }
        num[k] = e3_mul(e3_mul(e3_add(num[k], gamma), e3_add(e3_add(tv[k], e3_mul(delta, tn)), g)), opd);
    });
    {
        E3 a[PL_ROWS];
        const u32 hDim = J.hDim;
        each_item([&](auto k) { a[k] = ok[k] ? pl_h(J.h1, hDim, r[k]) : ident<false>(); }, nine);
        each_item([&](auto k) { den[k] = ok[k] ? pl_h(J.h2, hDim, r[k]) : ident<false>(); });
        each_item([&](auto k) {
            if (!ok[k]) { den[k] = ident<true>(); return; }
            E3 an = a[SCAN_ITEMS];
            if constexpr (decltype(k)::value + 1 < SCAN_ITEMS) { if (ok[k + 1]) an = a[k + 1]; }
            const E3 b = den[k];
            den[k] = e3_mul(e3_add(e3_add(a[k], pl_dh(delta, b, hDim)), g), e3_add(e3_add(b, pl_dh(delta, an, hDim)), g));
        });
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
    each_item([&](auto k) { const u64 i = base + k; if (i < n) st3(tmp, i, e3_mul(ex, loc[k])); });
    if (threadIdx.x == 0) st3(totals, blockIdx.x, bt);
}

// the fold: F and T of row i as columns of hDim words; with hDim = 1 the entry has seen kF = kT = 1 and no selT
__global__ void __launch_bounds__(256) plookup_fold_kernel(const PlJob J, u64 *__restrict__ outF, u64 strideF, u64 colF, u64 *__restrict__ outT, u64 strideT, u64 colT) {
    const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
    if (i >= J.n) return;
    const E3 beta = e3_of(J.beta);
    auto side = [&](const PlSide &S, const E3 &to) {
        const u64 *p = (const u64 *)S.base + i * S.stride;
        E3 v = ident<false>();
        for (u32 j = 0; j + 1 < S.k; j++) v = e3_add(v, e3_scale(e3_of(J.apow[S.k - 2 - j]), p[S.cols[j]]));
        v.v[0] = add(v.v[0], canon(p[S.cols[S.k - 1]]));
        if (S.sel) v = e3_add(e3_scale(e3_sub(v, to), ((const u64 *)S.sel)[i * S.selStride + S.selCol]), to);
        return v;
    };
    const E3 T = side(J.t, beta), F = side(J.f, T);
    u64 *f = outF + i * strideF + colF, *t = outT + i * strideT + colT;
    f[0] = F.v[0]; t[0] = T.v[0];
    if (J.hDim == 3) { f[1] = F.v[1]; f[2] = F.v[2]; t[1] = T.v[1]; t[2] = T.v[2]; }
}

// the job of either entry: the challenges canonical, the powers of alpha, g and 1 + delta (gamma and delta null: the fold)
void pl_job(const pil2gl_tuple_side &f, u64 kF, const pil2gl_tuple_side &t, u64 kT, const PlColumn *h1, const PlColumn *h2, u32 hDim, const u64 *alpha,
            const u64 *beta, const u64 *gamma, const u64 *delta, u64 n, PlJob &J) {
    auto canon3 = [](const u64 *x, u64 (&y)[3]) { for (int c = 0; c < 3; c++) y[c] = x ? h_canon(x[c]) : 0; };
    u64 a[3], b[3], ga[3], de[3], g[3], opd[3];
    canon3(alpha, a); canon3(beta, b); canon3(gamma, ga); canon3(delta, de);
    opd[0] = h_add(de[0], 1); opd[1] = de[1]; opd[2] = de[2];
    h_e3_mul(ga, opd, g);
    u64 pw[tupleside::MAX_K - 1][3], cur[3] = { 1, 0, 0 };
    for (u32 e = 0; e < tupleside::MAX_K - 1; e++) {
        h_e3_mul(cur, a, pw[e]);
        for (int c = 0; c < 3; c++) cur[c] = pw[e][c];
    }
    plookupplan::pack(f, kF, t, kT, h1, h2, hDim, pw, b, ga, de, g, opd, n, J);
}

int plookup_prod_launch(const pil2gl_tuple_side &f, u64 kF, const pil2gl_tuple_side &t, u64 kT, const PlColumn &h1, const PlColumn &h2, u32 hDim, const u64 *const *ch,
                        const PlColumn &out, u64 n, hipStream_t st) {
    PlJob J{};
    pl_job(f, kF, t, kT, &h1, &h2, hDim, ch[0], ch[1], ch[2], ch[3], n, J);
    const u64 nb = hintplan::blocks(n);
    u64 *tmp, *totals;
    P2_TRY(scratch(SCR_HINT_TMP, n * 3, &tmp));
    P2_TRY(scratch(SCR_HINT_TOTALS, nb * 3, &totals));
    plookup_fold_scan1<<<(unsigned)nb, SCAN_THREADS, 0, st>>>(J, tmp, totals);
    KERNEL_CHECK();
    hint_scan2<true><<<1, SCAN_THREADS, 0, st>>>(totals, nb);
    KERNEL_CHECK();
    hint_scan3<true><<<(unsigned)((n + 255) / 256), 256, 0, st>>>(tmp, totals, n, 3, (u64 *)out.base, out.stride, out.col);
    KERNEL_CHECK();
    return PIL2GL_OK;
}

int plookup_fold_launch(const pil2gl_tuple_side &f, u64 kF, const pil2gl_tuple_side &t, u64 kT, u32 hDim, const u64 *const *ch, const PlColumn *out, u64 n,
                        hipStream_t st) {
    PlJob J{};
    pl_job(f, kF, t, kT, nullptr, nullptr, hDim, ch[0], ch[1], nullptr, nullptr, n, J);
    plookup_fold_kernel<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(J, (u64 *)out[0].base, out[0].stride, out[0].col, (u64 *)out[1].base, out[1].stride, out[1].col);
    KERNEL_CHECK();
    return PIL2GL_OK;
}

int plookup_check(const pil2gl_tuple_side *f, u64 kF, const pil2gl_tuple_side *t, u64 kT, const PlColumn *read, u32 nRead, u32 hDim, const u64 *const *ch, u32 nCh,
                  const PlColumn *out, u32 nOut, u64 n, bool dev) {
    char why[96];
    if (const char *msg = plookupplan::check_call(f, kF, t, kT, read, nRead, hDim, ch, nCh, out, nOut, n, 1, dev, why)) return fail(PIL2GL_EINVAL, "%s", msg);
    return PIL2GL_OK;
}

}  // namespace

extern "C" {

int pil2gl_plookup_plan(uint64_t n, uint64_t kF, uint64_t kT, uint32_t elemWords, uint32_t *outInfo, uint64_t *workBytes) {
    if (workBytes) *workBytes = 0;
    if (const char *msg = plookupplan::check(n, kF, kT, elemWords)) return fail(PIL2GL_EINVAL, "%s", msg);
    const plookupplan::Plan p = plookupplan::plan(n, elemWords);
    if (outInfo) {
        outInfo[0] = p.threads; outInfo[1] = p.items; outInfo[2] = p.blocks; outInfo[3] = p.launches; outInfo[4] = p.depth;
        outInfo[5] = plookupplan::out_width(elemWords);
    }
    if (workBytes) *workBytes = p.bytes;
    return PIL2GL_OK;
}

int pil2gl_plookup_fold_dev(const pil2gl_tuple_side *hostF, uint64_t kF, const pil2gl_tuple_side *hostT, uint64_t kT, const uint64_t *hostAlpha,
                            const uint64_t *hostBeta, uint32_t hDim, uint64_t *outF, uint64_t strideF, uint64_t colF, uint64_t *outT, uint64_t strideT,
                            uint64_t colT, uint64_t n, void *stream) {
    const u64 *const ch[2] = { hostAlpha, hostBeta };
    const PlColumn out[2] = { { outF, strideF, colF }, { outT, strideT, colT } };
    P2_TRY(plookup_check(hostF, kF, hostT, kT, nullptr, 0, hDim, ch, 2, out, 2, n, true));
    if (!n) return PIL2GL_OK;
    P2_TRY(ensure_init());
    return plookup_fold_launch(*hostF, kF, *hostT, kT, hDim, ch, out, n, as_stream(stream));
}

// host matrices, each staged up to the last element touched; an output's matrix goes up as it is and comes back with the column written
// (outF and outT of one matrix: that matrix once)
int pil2gl_plookup_fold(const pil2gl_tuple_side *hostF, uint64_t kF, const pil2gl_tuple_side *hostT, uint64_t kT, const uint64_t *hostAlpha,
                        const uint64_t *hostBeta, uint32_t hDim, uint64_t *hostOutF, uint64_t strideF, uint64_t colF, uint64_t *hostOutT, uint64_t strideT,
                        uint64_t colT, uint64_t n) {
    const u64 *const ch[2] = { hostAlpha, hostBeta };
    PlColumn out[2] = { { hostOutF, strideF, colF }, { hostOutT, strideT, colT } };
    P2_TRY(plookup_check(hostF, kF, hostT, kT, nullptr, 0, hDim, ch, 2, out, 2, n, false));
    if (!n) return PIL2GL_OK;
    pil2gl_tuple_side f = *hostF, t = *hostT;
    const bool one = hostOutF == hostOutT;
    u64 wF = plookupplan::column_words(out[0], hDim, n, 1), wT = plookupplan::column_words(out[1], hDim, n, 1);
    if (one) wF = wT = wF > wT ? wF : wT;
    Stage s(tupleside::staged_words(f, n, kF, 1) + tupleside::staged_words(t, n, kT, 1) + smapplan::pad16(wF) + (one ? 0 : smapplan::pad16(wT)));
    P2_TRY(s.rc());
    tupleside::stage_side(s, f, n, kF, 1);
    tupleside::stage_side(s, t, n, kT, 1);
    out[0].base = s.put(hostOutF, wF); s.take(smapplan::pad16(wF) - wF);
    out[1].base = one ? out[0].base : s.put(hostOutT, wT);
    P2_TRY(s.rc());
    P2_TRY(plookup_fold_launch(f, kF, t, kT, hDim, ch, out, n, 0));
    P2_TRY(s.get(hostOutF, out[0].base, wF));
    return one ? PIL2GL_OK : s.get(hostOutT, out[1].base, wT);
}

int pil2gl_plookup_prod_dev(const pil2gl_tuple_side *hostF, uint64_t kF, const pil2gl_tuple_side *hostT, uint64_t kT, const uint64_t *h1, uint64_t h1Stride,
                            uint64_t h1Col, const uint64_t *h2, uint64_t h2Stride, uint64_t h2Col, uint32_t hDim, const uint64_t *hostAlpha,
                            const uint64_t *hostBeta, const uint64_t *hostGamma, const uint64_t *hostDelta, uint64_t *out, uint64_t outStride, uint64_t outCol,
                            uint64_t n, void *stream) {
    const u64 *const ch[4] = { hostAlpha, hostBeta, hostGamma, hostDelta };
    const PlColumn h[2] = { { h1, h1Stride, h1Col }, { h2, h2Stride, h2Col } }, o = { out, outStride, outCol };
    P2_TRY(plookup_check(hostF, kF, hostT, kT, h, 2, hDim, ch, 4, &o, 1, n, true));
    if (!n) return PIL2GL_OK;
    P2_TRY(ensure_init());
    return plookup_prod_launch(*hostF, kF, *hostT, kT, h[0], h[1], hDim, ch, o, n, as_stream(stream));
}

int pil2gl_plookup_prod(const pil2gl_tuple_side *hostF, uint64_t kF, const pil2gl_tuple_side *hostT, uint64_t kT, const uint64_t *hostH1, uint64_t h1Stride,
                        uint64_t h1Col, const uint64_t *hostH2, uint64_t h2Stride, uint64_t h2Col, uint32_t hDim, const uint64_t *hostAlpha,
                        const uint64_t *hostBeta, const uint64_t *hostGamma, const uint64_t *hostDelta, uint64_t *hostOut, uint64_t outStride, uint64_t outCol,
                        uint64_t n) {
    const u64 *const ch[4] = { hostAlpha, hostBeta, hostGamma, hostDelta };
    PlColumn h[2] = { { hostH1, h1Stride, h1Col }, { hostH2, h2Stride, h2Col } }, o = { hostOut, outStride, outCol };
    P2_TRY(plookup_check(hostF, kF, hostT, kT, h, 2, hDim, ch, 4, &o, 1, n, false));
    if (!n) return PIL2GL_OK;
    pil2gl_tuple_side f = *hostF, t = *hostT;
    const u64 outWords = plookupplan::column_words(o, 3, n, 1);
    Stage s(tupleside::staged_words(f, n, kF, 1) + tupleside::staged_words(t, n, kT, 1) + smapplan::pad16(plookupplan::column_words(h[0], hDim, n, 1)) +
            smapplan::pad16(plookupplan::column_words(h[1], hDim, n, 1)) + smapplan::pad16(outWords));
    P2_TRY(s.rc());
    tupleside::stage_side(s, f, n, kF, 1);
    tupleside::stage_side(s, t, n, kT, 1);
    plookupplan::stage_column(s, h[0], hDim, n, 1);
    plookupplan::stage_column(s, h[1], hDim, n, 1);
    o.base = s.put(hostOut, outWords);
    P2_TRY(s.rc());
    P2_TRY(plookup_prod_launch(f, kF, t, kT, h[0], h[1], hDim, ch, o, n, 0));
    return s.get(hostOut, o.base, outWords);
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
