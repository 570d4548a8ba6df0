// Division by x^k - beta and evaluation of polynomials over the BN254 scalar field Fr, gfx950: the long-vector field work of the fflonk
// prover's last two steps.  Q.divZh(N, 2^extendBits) of computeQFflonk (fflonk_prover_helpers.js:147-148) is k = N, beta = 1; the
// openings (shplonkjs open, :212) divide by x^k - h^k and by x - y and evaluate the committed polynomials at their opening points
// (k = 1, beta = z: d[0] = p(z)).  All of it is one recurrence over a coefficient vector c[0..n):
//
//     d[i] = c[i] + beta d[i + k]      (d[j] = 0 for j >= n)
//
// d[k..n) is the quotient (coefficient m at position m + k), d[0..k) the remainder.  Position i depends on c[i] and on positions above
// it only, so dst may be src.  Elements are 32 bytes of Montgomery words, canonical in and out, moved as two 16-byte halves as in
// bn_ntt.hip; add and mul are bn_field.cuh's.  Fr arithmetic is exact, so every association of the sums gives the same bytes.
//
// There are k chains (i mod k) of M = ceil(n / k) links.  bnpoly::plan (bn_poly_plan.h) cuts each into S segments of L links; lane
// t = s k + j owns segment s of chain j, so neighbouring lanes are neighbouring chains.
//   reduce   (phase A) a lane runs Horner over its segment, from the top, and leaves the segment's value V[t].  A final partial segment
//            is zero-padded by definition: a lane walks only the links below n, an empty segment leaves zero.
//   carries  (phase B) D[t] = V[t] + beta^L D[t + k] is the same recurrence on S k items: the next level of the plan, in place in V,
//            until a level has a lane per chain.
//   store    (phase C) a lane reruns its segment seeded with beta times its carry D[t + k] and stores every link.
// Two products per element, c read twice, d written once.  With k >= the lane count, or chains no longer than a segment, level 0 is a
// lane per chain and there is nothing else (divZh at k = 2^20, M = 2..8).  Evaluation is reduce at every level, the point index as
// grid.y, and stores nothing but the P results.  The multipliers beta^L, beta^(L L'), ... are computed on the host (bn_params.cpp's
// arithmetic) and staged at the head of the working buffer: there is no exponentiation on the device.
//
// Memory: at small k a lane walks L consecutive links, so neighbouring lanes are L k 32 bytes apart and a wave's load touches 64 lines,
// each of which the lane comes back to on its next steps.  The alternative, staging a wave's chunk through LDS so that global accesses
// are contiguous, was not taken: a link costs a product of about 330 vector instructions per 32 bytes, which
// leaves the kernel issue-bound by estimate; DESIGN.md section 14 has the arithmetic and says what is measured.  The next element is
// loaded before the product that does not need it.
//
// Memory safety does not rest on n, k and L dividing each other: a lane's links are [s L, min((s + 1) L, links of chain j)), every
// element index is j + m k with m below the chain's link count, and a carry is read only for s + 1 < S.
#include "bn_column_stage.h"
#include "bn_elem.cuh"
#include "bn_params.h"
#include "bn_poly_plan.h"

using namespace pil2gl;
using bn::u32;
using bn::unpack;
using bn::st_elem;

namespace {

struct LevelArgs {
    const uint4 *src; uint4 *dst;                    // element i of the level at 2 * i * stride (in 16-byte halves)
    const uint4 *carry;                              // store: D of the next level (the seed of lane t is beta * carry[t + k]), or null
    const uint4 *beta;                               // this level's multiplier
    u64 n, stride, k, M, full, S;                    // full: chains of M links, the others have M - 1
    u32 L;
    u64 srcPitch, dstPitch;                          // per point (grid.y), in 16-byte halves
    u32 betaPitch;                                   // per point, in elements
};

// STORE = false: reduce (dst[t] = the segment's value, dense).  STORE = true: every link of the segment to dst, same addressing as src.
template <bool STORE>
__global__ void __launch_bounds__(bnpoly::THREADS) bn_poly_kernel(LevelArgs a) {
    const u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    const u64 w = a.k < a.n ? a.k : a.n;             // chains that have an element (S > 1 implies n > k)
    if (t >= a.S * w) return;
    u64 s = 0, j = t;
    if (a.S > 1) { s = t / a.k; j = t - s * a.k; }
    const u64 links = a.M - (j >= a.full ? 1 : 0);
    const u64 mBegin = s * a.L;
    const u64 mEnd = mBegin + a.L < links ? mBegin + a.L : links;
    const uint4 *src = a.src + (size_t)blockIdx.y * a.srcPitch;
    uint4 *dst = a.dst + (size_t)blockIdx.y * a.dstPitch;
    if (mBegin >= mEnd) {                            // a segment wholly above n: zero by definition, nothing to store
        if (!STORE) { dst[2 * t] = make_uint4(0, 0, 0, 0); dst[2 * t + 1] = make_uint4(0, 0, 0, 0); }
        return;
    }
    const uint4 *bp = a.beta + 2 * (size_t)blockIdx.y * a.betaPitch;
    u32 b[8], x[8], y[8];
    unpack(bp[0], bp[1], b);
    u64 m = mEnd - 1;
    const size_t step = 2 * (size_t)a.k * a.stride, top = 2 * (size_t)(j + m * a.k) * a.stride;
    const uint4 *ps = src + top;
    uint4 lo = ps[0], hi = ps[1];
    unpack(lo, hi, x);
    if (STORE && a.carry && s + 1 < a.S) {
        const uint4 *cp = a.carry + 2 * (t + a.k);
        unpack(cp[0], cp[1], y);
        bn::fr_mul(y, y, b);
        bn::fr_add(x, y);
    }
    uint4 *pd = dst + top;
    if (STORE) st_elem(pd, x);
    while (m > mBegin) {
        m--;
        ps -= step;
        lo = ps[0]; hi = ps[1];
        bn::fr_mul(x, x, b);
        unpack(lo, hi, y);
        bn::fr_add(x, y);
        if (STORE) { pd -= step; st_elem(pd, x); }
    }
    if (!STORE) st_elem(dst + 2 * t, x);
}

// the multipliers of every level for nPoints values of beta, [point][level] at the head of the working buffer
void level_powers(const bnpoly::Plan &p, const u64 *hostBeta, u32 nPoints, bnp::U256 *out) {
    for (u32 q = 0; q < nPoints; q++) {
        bnp::U256 b;
        for (int i = 0; i < 4; i++) b.w[i] = hostBeta[4 * q + i];
        for (u32 i = 0; i < p.nLevels; i++) {
            out[(size_t)q * bnpoly::MAX_LEVELS + i] = b;
            if (i + 1 < p.nLevels) b = bnp::bn_mont_pow(b, p.lv[i].L);
        }
    }
}

template <bool STORE>
int launch_level(const bnpoly::Level &l, u64 k, u32 nPoints, LevelArgs a, hipStream_t st) {
    a.n = l.n; a.k = k; a.M = l.M; a.full = l.full; a.S = l.S; a.L = l.L;
    const u64 lanes = l.S * (k < l.n ? k : l.n);
    const dim3 grid((unsigned)((lanes + bnpoly::THREADS - 1) / bnpoly::THREADS), nPoints);
    bn_poly_kernel<STORE><<<grid, bnpoly::THREADS, 0, st>>>(a);
    KERNEL_CHECK();
    return PIL2GL_OK;
}

int stage_powers(const bnpoly::Plan &p, const u64 *hostBeta, u32 nPoints, uint4 **base, hipStream_t st) {
    bnp::U256 pw[bnpoly::BETA_ELEMS];
    level_powers(p, hostBeta, nPoints, pw);
    u64 *d;
    P2_TRY(scratch(SCR_BN_POLY, bnpoly::scratch_bytes(p, nPoints) / 8, &d));
    // a pageable-host async copy is staged by the runtime before it returns, so `pw` may go out of scope; the kernels are only enqueued
    HIP_TRY(hipMemcpyAsync(d, pw, (size_t)nPoints * bnpoly::MAX_LEVELS * 32, hipMemcpyHostToDevice, st));
    *base = (uint4 *)d;
    return PIL2GL_OK;
}

int div_launch(const u64 *src, u64 n, u64 stride, u64 k, const u64 *hostBeta, u64 *dst, hipStream_t st) {
    if (n == 0) return PIL2GL_OK;
    const bnpoly::Plan p = bnpoly::plan(n, k);
    uint4 *base;
    P2_TRY(stage_powers(p, hostBeta, 1, &base, st));
    auto values = [&](u32 i) { return base + 2 * (bnpoly::BETA_ELEMS + p.lv[i].off); };
    auto args = [&](u32 i) {                         // level 0 works on the caller's buffers, level i > 0 in place on the values of level i - 1
        LevelArgs a{};
        a.src = i ? values(i - 1) : (const uint4 *)src;
        a.dst = i ? values(i - 1) : (uint4 *)dst;
        a.stride = i ? 1 : stride;
        a.beta = base + 2 * i;
        return a;
    };
    const u32 last = p.nLevels - 1;
    for (u32 i = 0; i < last; i++) {
        LevelArgs a = args(i);
        a.dst = values(i);
        P2_TRY(launch_level<false>(p.lv[i], k, 1, a, st));
    }
    for (u32 i = p.nLevels; i-- > 0;) {
        LevelArgs a = args(i);
        a.carry = i < last ? values(i) : nullptr;
        P2_TRY(launch_level<true>(p.lv[i], k, 1, a, st));
    }
    return PIL2GL_OK;
}

int eval_launch(const u64 *src, u64 n, u64 stride, const u64 *hostPoints, u32 nPoints, u64 *out, hipStream_t st) {
    if (n == 0) {
        HIP_TRY(hipMemsetAsync(out, 0, 32 * (size_t)nPoints, st));
        return PIL2GL_OK;
    }
    const bnpoly::Plan p = bnpoly::plan(n, 1);
    uint4 *base;
    P2_TRY(stage_powers(p, hostPoints, nPoints, &base, st));
    const u64 pitch = 2 * p.valueElems;
    auto values = [&](u32 i) { return base + 2 * (bnpoly::BETA_ELEMS + p.lv[i].off); };
    for (u32 i = 0; i < p.nLevels; i++) {
        LevelArgs a{};
        a.src = i ? values(i - 1) : (const uint4 *)src; a.srcPitch = i ? pitch : 0; a.stride = i ? 1 : stride;
        const bool lastLevel = i + 1 == p.nLevels;   // one lane per point leaves the result
        a.dst = lastLevel ? (uint4 *)out : values(i); a.dstPitch = lastLevel ? 2 : pitch;
        a.beta = base + 2 * i; a.betaPitch = bnpoly::MAX_LEVELS;
        P2_TRY(launch_level<false>(p.lv[i], 1, nPoints, a, st));
    }
    return PIL2GL_OK;
}

int check_div(const u64 *src, u64 n, u64 stride, u64 k, const u64 *hostBeta, const u64 *dst) {
    P2_TRY(check_column(src, n, stride, "src"));
    if (k == 0 || k > bncol::MAX_N) return fail(PIL2GL_EINVAL, "k = %llu: 1 <= k <= 2^28", (unsigned long long)k);
    if (!hostBeta || (n && !dst)) return fail(PIL2GL_EINVAL, "null buffer");
    return PIL2GL_OK;
}
int check_eval(const u64 *src, u64 n, u64 stride, const u64 *hostPoints, u32 nPoints, const u64 *out) {
    P2_TRY(check_column(src, n, stride, "src"));
    if (nPoints == 0 || nPoints > bnpoly::MAX_POINTS) return fail(PIL2GL_EINVAL, "nPoints = %u: 1 <= nPoints <= %u", nPoints, bnpoly::MAX_POINTS);
    if (!hostPoints || !out) return fail(PIL2GL_EINVAL, "null buffer");
    return PIL2GL_OK;
}

}  // namespace

extern "C" {

int pil2gl_debug_bn128_poly_plan(uint64_t n, uint64_t k, uint32_t *outInfo, uint64_t *scratchBytes) {
    if (!outInfo || !scratchBytes) return fail(PIL2GL_EINVAL, "null argument");
    if (const char *m = bncol::check_size(n)) return fail(PIL2GL_EINVAL, "n = %llu: %s", (unsigned long long)n, m);
    if (k == 0 || k > bncol::MAX_N) return fail(PIL2GL_EINVAL, "k = %llu: 1 <= k <= 2^28", (unsigned long long)k);
    const bnpoly::Plan p = bnpoly::plan(n, k);
    outInfo[0] = p.lv[0].L; outInfo[1] = (uint32_t)p.lv[0].S; outInfo[2] = p.nLevels - 1; outInfo[3] = bnpoly::THREADS;
    outInfo[4] = p.lv[0].S > 1 ? 1 : 0;
    *scratchBytes = bnpoly::scratch_bytes(p, 1);
    return PIL2GL_OK;
}

int pil2gl_bn128_poly_div_xk_sub_dev(const uint64_t *src, uint64_t n, uint64_t stride, uint64_t k, const uint64_t hostBeta[4], uint64_t *dst, void *stream) {
    P2_TRY(check_div(src, n, stride, k, hostBeta, dst));
    P2_TRY(ensure_init());
    P2_TRY(check_aligned16({ src, dst }));
    return div_launch(src, n, stride, k, hostBeta, dst, as_stream(stream));
}

int pil2gl_bn128_poly_div_xk_sub(const uint64_t *src, uint64_t n, uint64_t stride, uint64_t k, const uint64_t hostBeta[4], uint64_t *dst) {
    P2_TRY(check_div(src, n, stride, k, hostBeta, dst));
    if (n == 0) return PIL2GL_OK;
    const bncol::Col cols[2] = { { (uintptr_t)src, n, stride, true, false }, { (uintptr_t)dst, n, stride, false, true } };
    ColumnStage s(cols, 2);                          // dst == src: one copy serves both (bn_column.h)
    P2_TRY(s.rc());
    P2_TRY(div_launch(s.dev(0), n, stride, k, hostBeta, s.dev(1), 0));
    return s.copy_back();
}

int pil2gl_bn128_poly_eval_dev(const uint64_t *src, uint64_t n, uint64_t stride, const uint64_t *hostPoints, uint32_t nPoints, uint64_t *out, void *stream) {
    P2_TRY(check_eval(src, n, stride, hostPoints, nPoints, out));
    P2_TRY(ensure_init());
    P2_TRY(check_aligned16({ src, out }));
    return eval_launch(src, n, stride, hostPoints, nPoints, out, as_stream(stream));
}

int pil2gl_bn128_poly_eval(const uint64_t *src, uint64_t n, uint64_t stride, const uint64_t *hostPoints, uint32_t nPoints, uint64_t *out) {
    P2_TRY(check_eval(src, n, stride, hostPoints, nPoints, out));
    if (n == 0) { for (uint32_t i = 0; i < 4 * nPoints; i++) out[i] = 0; return PIL2GL_OK; }
    const bncol::Col col{ (uintptr_t)src, n, stride, true, false };
    ColumnStage s(&col, 1, 4ull * nPoints);          // the results are nPoints elements, no column
    P2_TRY(s.rc());
    uint64_t *dOut = s.stage().take(4ull * nPoints);
    P2_TRY(s.rc());
    P2_TRY(eval_launch(s.dev(0), n, stride, hostPoints, nPoints, dOut, 0));
    return s.stage().get(out, dOut, 4ull * nPoints);
}

}  // extern "C"
