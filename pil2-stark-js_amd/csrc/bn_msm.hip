// Multi-scalar multiplication over BN254 G1, gfx950: the device twin of G1.toAffine(G1.multiExpAffine(bases, scalars)), the commitment step
// of the fflonk prover (fflonk_prover_helpers.js:185,336, fflonk_setup.js:52), for a batch of K packed polynomials over the same bases
// (bn_msm_batch.h; the single MSM is the batch of one polynomial of one slot).  out_k = sum_i s_k,i P_i by the bucket (Pippenger) method,
// one path for every batch (bnp::bn_msm_batch_plan gives the window width c, the windows and how many of them a pass takes):
//
//   per pass of windowsPerPass windows
//     histogram   a lane per point of the whole batch: lane -> (k, i) -> the scalar's element (bn_msm_batch.h); the scalar leaves
//                 Montgomery form (one fr_mul by 1) if it came in it, is recoded into signed digits (bn_msm_recode.h) and counts one into
//                 the bucket (window, k, |digit|) of every non-zero digit of the pass's windows.  Empty slots, zero digits and points at
//                 infinity are dropped here.
//     scan        one workgroup: exclusive prefix sums of the histogram in place, a copy as the scatter's cursors.
//     scatter     the histogram's lanes again: each non-zero digit takes the next slot of its bucket and writes i | sign << 31, i the
//                 index within its polynomial: every polynomial indexes the bases from 0.
//     accumulate  a lane per bucket: its points, fetched by index one ahead of their use, summed by the mixed addition (bn_g1.cuh).  A bucket
//                 that holds all n_k points is slow but no different.  Every bucket of the pass is written, the empty ones as infinity:
//                 nothing of an earlier call or pass is read.
//   reduce        sum_d d B_d of every window of every polynomial (K * nWindows items) by running sums, in levels: a lane takes L
//                 consecutive items (X_i, Y_i) of a window and leaves X' = L sum X_i, Y' = sum Y_i + sum (i mod L + off) X_i, so that
//                 sum_i (Y_i + (i + off) X_i) = sum_seg (Y'_seg + seg X'_seg): the same problem on 1/L of the items, with off = 0.  Level 1
//                 reads the buckets (Y absent, off = 1: bucket i stands for digit i + 1); the last level leaves one Y per window.
//   tail          one wave per polynomial, its lane 0: Horner over the windows (c doublings, one addition each), the inversion for
//                 to-affine, the polynomial's 64 output bytes.
//
// Memory safety does not rest on the sort being right, per polynomial: a list position is clamped to the list, a point index is used only
// below n_k, a bucket index only below the pass's bucket count, and every loop over device-computed bounds runs at most n_k times.
#include "common.h"
#include "bn_params.h"
#include "bn_msm_recode.h"
#include "bn_msm_batch.h"
#include "bn_g1.cuh"
#include "bn_elem.cuh"

using namespace pil2gl;
using bn::u32;
using bn::G1X;
using bn::unpack;

namespace {

constexpr u64 MSM_MAX_N = 1ull << 28;
constexpr u32 ENTRY_INDEX_MASK = 0x7fffffffu;        // n <= 2^28 < 2^31: bit 31 carries the sign
constexpr int POINT_THREADS = 256, BUCKET_THREADS = 64, SCAN_THREADS = 1024;

struct PassParams {
    const uint4 *bases, *scalars;
    u64 nTotal, cap;                                 // point lanes of the batch; cap: entries the list has room for (nTotal * windows of the pass)
    u32 mont, c, nbw, w0, g, nb, K;                  // nb = g * K * nbw buckets in this pass: bucket ((w - w0) * K + k) * nbw + |digit| - 1
    u32 count[bnm::MSM_MAX_POLYS];                   // n_k
    u32 *hist, *cursor, *entries;
    uint4 *buckets;                                  // the pass's first bucket
};

__device__ __forceinline__ void ld_point(const uint4 *p, G1X &v) {
    unpack(p[0], p[1], v.x); unpack(p[2], p[3], v.y); unpack(p[4], p[5], v.zz); unpack(p[6], p[7], v.zzz);
}
__device__ __forceinline__ void st_point(uint4 *p, const G1X &v) {
    p[0] = make_uint4(v.x[0], v.x[1], v.x[2], v.x[3]); p[1] = make_uint4(v.x[4], v.x[5], v.x[6], v.x[7]);
    p[2] = make_uint4(v.y[0], v.y[1], v.y[2], v.y[3]); p[3] = make_uint4(v.y[4], v.y[5], v.y[6], v.y[7]);
    p[4] = make_uint4(v.zz[0], v.zz[1], v.zz[2], v.zz[3]); p[5] = make_uint4(v.zz[4], v.zz[5], v.zz[6], v.zz[7]);
    p[6] = make_uint4(v.zzz[0], v.zzz[1], v.zzz[2], v.zzz[3]); p[7] = make_uint4(v.zzz[4], v.zzz[5], v.zzz[6], v.zzz[7]);
}

// emit(bucket of the pass, negative, index within the polynomial) for every non-zero digit of the batch's point `lane` in the pass's windows
template <class F>
__device__ __forceinline__ void for_each_digit(const PassParams &P, const bnm::MsmBatch &B, u64 lane, F emit) {
    u32 k, i;
    u64 element;
    if (!bnm::msm_batch_locate(B, lane, k, i) || !bnm::msm_batch_element(B, k, i, element)) return;      // an empty slot: the coefficient is 0
    const uint4 *b = P.bases + 4 * (u64)i;
    const uint4 b0 = b[0], b1 = b[1], b2 = b[2], b3 = b[3];
    if (((b0.x | b0.y | b0.z | b0.w) | (b1.x | b1.y | b1.z | b1.w) | (b2.x | b2.y | b2.z | b2.w) | (b3.x | b3.y | b3.z | b3.w)) == 0) return;
    const uint4 *sp = P.scalars + 2 * element;
    u32 s[8];
    unpack(sp[0], sp[1], s);
    if (P.mont) {
        const u32 one[8] = { 1, 0, 0, 0, 0, 0, 0, 0 };
        bn::fr_mul(s, s, one);
    }
    u32 carry = 0;
    const u32 wEnd = P.w0 + P.g;                     // <= nWindows <= MSM_MAX_WINDOWS
    for (u32 w = 0; w < wEnd; w++) {
        const int32_t d = bnm::msm_next_digit(s, carry, P.c);
        if (w < P.w0 || d == 0) continue;
        const u32 mag = (u32)(d < 0 ? -d : d);
        if (mag > P.nbw) continue;                   // only a scalar >= 2^254 gets here: not a valid input, but no index leaves the pass
        emit(((w - P.w0) * P.K + k) * P.nbw + mag - 1, d < 0, i);
    }
}

__global__ void __launch_bounds__(POINT_THREADS) bn_msm_hist_kernel(PassParams P, bnm::MsmBatch B) {
    const u64 lane = (u64)blockIdx.x * POINT_THREADS + threadIdx.x;
    if (lane >= P.nTotal) return;
    for_each_digit(P, B, lane, [&](u32 bucket, bool, u32) { atomicAdd(&P.hist[bucket], 1u); });
}

// hist[0..nb) -> its exclusive prefix sums, hist[nb] = the total; cursor = a copy of the sums.  One workgroup: nb is at most
// bnp::BN_MSM_PASS_CELLS = 2^18, 256 cells per lane, which a single MSM of 2^19 points and more has always given it.
__global__ void __launch_bounds__(SCAN_THREADS) bn_msm_scan_kernel(u32 *hist, u32 *cursor, u32 nb) {
    __shared__ u32 part[SCAN_THREADS];
    const u32 t = threadIdx.x, chunk = (nb + SCAN_THREADS - 1) / SCAN_THREADS;
    const u32 k0 = t * chunk < nb ? t * chunk : nb, k1 = k0 + chunk < nb ? k0 + chunk : nb;
    u32 sum = 0;
    for (u32 k = k0; k < k1; k++) sum += hist[k];
    part[t] = sum;
    __syncthreads();
    for (u32 d = 1; d < SCAN_THREADS; d <<= 1) {
        const u32 v = t >= d ? part[t - d] : 0u;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    u32 run = part[t] - sum;                         // exclusive
    for (u32 k = k0; k < k1; k++) { const u32 h = hist[k]; hist[k] = run; cursor[k] = run; run += h; }
    if (t == SCAN_THREADS - 1) hist[nb] = part[t];
}

__global__ void __launch_bounds__(POINT_THREADS) bn_msm_scatter_kernel(PassParams P, bnm::MsmBatch B) {
    const u64 lane = (u64)blockIdx.x * POINT_THREADS + threadIdx.x;
    if (lane >= P.nTotal) return;
    for_each_digit(P, B, lane, [&](u32 bucket, bool neg, u32 i) {
        const u32 pos = atomicAdd(&P.cursor[bucket], 1u);
        if (pos < P.cap) P.entries[pos] = i | (neg ? ~ENTRY_INDEX_MASK : 0u);
    });
}

__device__ __forceinline__ void ld_base(const PassParams &P, u32 n, u64 pos, u32 x[8], u32 y[8], u32 &entry) {
    entry = P.entries[pos];
    const u64 idx = entry & ENTRY_INDEX_MASK;
    const uint4 *b = P.bases + 4 * (idx < n ? idx : 0);      // an index the scatter cannot have written reads point 0 and is skipped below
    const uint4 b0 = b[0], b1 = b[1], b2 = b[2], b3 = b[3];
    unpack(b0, b1, x); unpack(b2, b3, y);
}

__global__ void __launch_bounds__(BUCKET_THREADS) bn_msm_accumulate_kernel(PassParams P) {
    const u32 b = blockIdx.x * BUCKET_THREADS + threadIdx.x;
    if (b >= P.nb) return;
    const u32 n = P.count[(b / P.nbw) % P.K & (bnm::MSM_MAX_POLYS - 1)];         // the bucket's polynomial: its indices are used only below n_k
    u64 end = P.hist[b + 1], start = P.hist[b];
    if (end > P.cap) end = P.cap;
    if (start > end) start = end;
    if (end - start > n) end = start + n;            // a bucket holds each point at most once
    G1X acc;
    bn::g1_set_inf(acc);
    u32 nx[8], ny[8], nxtEntry = ENTRY_INDEX_MASK;   // the point after the current one, already on its way
#pragma unroll
    for (int l = 0; l < 8; l++) nx[l] = ny[l] = 0;
    if (start < end) ld_base(P, n, start, nx, ny, nxtEntry);
    for (u64 p = start; p < end; p++) {
        u32 x[8], y[8];
        const u32 entry = nxtEntry;
        bn::fq_copy(x, nx); bn::fq_copy(y, ny);
        if (p + 1 < end) ld_base(P, n, p + 1, nx, ny, nxtEntry);
        if ((entry & ENTRY_INDEX_MASK) < n) {
            if (entry & ~ENTRY_INDEX_MASK) bn::fq_neg(y, y);
            bn::g1_madd(acc, x, y);
        }
    }
    st_point(P.buckets + 8 * (u64)b, acc);
}

struct LevelParams {
    const uint4 *xin, *yin;                          // yin = nullptr: level 1 (the buckets)
    uint4 *xout, *yout;
    u32 nWindows, m, L, lShift, off, mOut;           // m items per window in, mOut = ceil(m / L) out; L = 2^lShift
};

__global__ void __launch_bounds__(BUCKET_THREADS) bn_msm_reduce_kernel(LevelParams P) {
    const u32 t = blockIdx.x * BUCKET_THREADS + threadIdx.x;
    if (t >= P.nWindows * P.mOut) return;
    const u32 w = t / P.mOut, seg = t - w * P.mOut;
    G1X run, acc, v;
    bn::g1_set_inf(run); bn::g1_set_inf(acc);
    for (int j = (int)P.L - 1; j >= 0; j--) {
        const u32 i = seg * P.L + (u32)j;
        if (i < P.m) {
            const u64 at = 8 * ((u64)w * P.m + i);
            ld_point(P.xin + at, v);
            bn::g1_add(run, v);
            if (P.yin) { ld_point(P.yin + at, v); bn::g1_add(acc, v); }
        }
        if ((u32)j + P.off >= 1) bn::g1_add(acc, run);
    }
    for (u32 k = 0; k < P.lShift; k++) bn::g1_dbl(run);
    st_point(P.xout + 8 * (u64)t, run);
    st_point(P.yout + 8 * (u64)t, acc);
}

// windows: one point per window of every polynomial (the last level's Y, window w of polynomial k at w * K + k);  out: polynomial
// blockIdx.x's affine sum, 64 bytes each
__global__ void __launch_bounds__(64) bn_msm_tail_kernel(const uint4 *windows, u32 nWindows, u32 K, u32 c, u32 *out) {
    const u32 k = blockIdx.x;
    if (k >= K || threadIdx.x != 0) return;
    G1X r, v;
    bn::g1_set_inf(r);
    for (int w = (int)nWindows - 1; w >= 0; w--) {
        for (u32 j = 0; j < c; j++) bn::g1_dbl(r);
        ld_point(windows + 8 * ((u64)w * K + k), v);
        bn::g1_add(r, v);
    }
    u32 x[8], y[8];
    bn::g1_to_affine(r, x, y);
    for (int i = 0; i < 8; i++) { out[16 * k + i] = x[i]; out[16 * k + 8 + i] = y[i]; }
}

int check_args(const void *bases, const void *scalars, u64 n, u64 stride, const void *out) {
    if (n > MSM_MAX_N) return fail(PIL2GL_EINVAL, "n = %llu: at most 2^28 points", (unsigned long long)n);
    if (stride == 0 || stride >> 32) return fail(PIL2GL_EINVAL, "scalarStride must be in 1..2^32-1");
    if (!out || (n && (!bases || !scalars))) return fail(PIL2GL_EINVAL, "null buffer");
    return PIL2GL_OK;
}

// The batch of a commit call, checked; nTotal = sum n_k, *extent = the elements of scalars the descriptors reach (0 without a point).
int check_commit(const void *bases, u64 nBases, const void *scalars, u64 rowStride, const pil2gl_g1_poly *polys, u32 K, const u32 *slots,
                 const void *out, bnm::MsmBatch &B, u64 &nTotal, u64 &extent, bool buffers = true) {
    if (!out || !polys || !slots) return fail(PIL2GL_EINVAL, "null buffer");
    if (K < 1 || K > bnm::MSM_MAX_POLYS) return fail(PIL2GL_EINVAL, "K = %u polynomials: 1..%u", K, bnm::MSM_MAX_POLYS);
    if (rowStride == 0 || rowStride >> 32) return fail(PIL2GL_EINVAL, "rowStride must be in 1..2^32-1");
    B = bnm::MsmBatch{};
    B.K = K; B.rowStride = (u32)rowStride;
    u32 nSlots = 0;
    nTotal = extent = 0;
    for (u32 k = 0; k < K; k++) {
        const pil2gl_g1_poly &p = polys[k];
        if (p.m < 1 || p.m > bnm::MSM_MAX_SLOTS) return fail(PIL2GL_EINVAL, "polynomial %u: m = %u slots: 1..%u", k, p.m, bnm::MSM_MAX_SLOTS);
        if (nSlots + p.m > bnm::MSM_MAX_TOTAL_SLOTS) return fail(PIL2GL_EINVAL, "more than %u slots in one batch (sum of m)", bnm::MSM_MAX_TOTAL_SLOTS);
        if (p.rows > MSM_MAX_N) return fail(PIL2GL_EINVAL, "more than 2^28 coefficients in one batch");
        if (p.rows * p.m > nBases)
            return fail(PIL2GL_EINVAL, "polynomial %u: m * rows = %u * %llu coefficients, nBases = %llu", k, p.m, (unsigned long long)p.rows, (unsigned long long)nBases);
        nTotal += p.rows * p.m;
        if (nTotal > MSM_MAX_N) return fail(PIL2GL_EINVAL, "more than 2^28 coefficients in one batch");
        if (p.first >> 58) return fail(PIL2GL_EINVAL, "polynomial %u: first = %llu: below 2^58", k, (unsigned long long)p.first);
        u32 top = 0;
        bool any = false;
        for (u32 j = 0; j < p.m; j++) {
            const u32 col = slots[nSlots + j];
            B.slots[nSlots + j] = col;
            if (col == bnm::MSM_EMPTY_SLOT) continue;
            if (col >= rowStride) return fail(PIL2GL_EINVAL, "polynomial %u: slot %u names column %u, rowStride = %llu", k, j, col, (unsigned long long)rowStride);
            any = true;
            if (col > top) top = col;
        }
        if (any && p.rows) extent = std::max(extent, p.first + (p.rows - 1) * rowStride + top + 1);    // < 2^58 + 2^60 + 2^32
        B.first[k] = p.first; B.rows[k] = (u32)p.rows; B.m[k] = p.m;
        nSlots += p.m;
    }
    if (buffers && ((nTotal && !bases) || (extent && !scalars))) return fail(PIL2GL_EINVAL, "null buffer");
    return PIL2GL_OK;
}

// out[k] = the affine sum of polynomial k of the batch, 64 bytes each
int bn_msm_launch(const u64 *bases, const u64 *scalars, const bnm::MsmBatch &B, u32 mont, u64 *out, hipStream_t st) {
    const u32 K = B.K;
    u64 counts[bnm::MSM_MAX_POLYS], nTotal = 0;
    for (u32 k = 0; k < K; k++) { counts[k] = bnm::msm_batch_count(B, k); nTotal += counts[k]; }
    if (nTotal == 0) { HIP_TRY(hipMemsetAsync(out, 0, 64 * (u64)K, st)); return PIL2GL_OK; }
    const bnp::BnMsmPlan plan = bnp::bn_msm_batch_plan(K, counts);
    u64 *work = nullptr;
    P2_TRY(scratch(SCR_BN_MSM, (plan.scratchBytes + 7) / 8, &work));
    char *base = (char *)work;
    uint4 *buckets = (uint4 *)(base + plan.offBuckets);

    PassParams P;
    P.bases = (const uint4 *)bases; P.scalars = (const uint4 *)scalars;
    P.nTotal = nTotal; P.mont = mont ? 1u : 0u; P.c = plan.c; P.nbw = plan.bucketsPerWindow; P.K = K;
    for (u32 k = 0; k < bnm::MSM_MAX_POLYS; k++) P.count[k] = k < K ? (u32)counts[k] : 0u;
    P.hist = (u32 *)(base + plan.offHist); P.cursor = (u32 *)(base + plan.offCursor); P.entries = (u32 *)(base + plan.offEntries);
    const unsigned pointBlocks = (unsigned)((nTotal + POINT_THREADS - 1) / POINT_THREADS);
    for (u32 w0 = 0; w0 < plan.nWindows; w0 += plan.windowsPerPass) {
        P.w0 = w0; P.g = plan.nWindows - w0 < plan.windowsPerPass ? plan.nWindows - w0 : plan.windowsPerPass;
        P.nb = P.g * K * P.nbw; P.cap = nTotal * P.g;
        P.buckets = buckets + 8 * (u64)w0 * K * P.nbw;
        HIP_TRY(hipMemsetAsync(P.hist, 0, ((u64)P.nb + 1) * 4, st));      // per call and per pass: no count survives
        bn_msm_hist_kernel<<<pointBlocks, POINT_THREADS, 0, st>>>(P, B);
        KERNEL_CHECK();
        bn_msm_scan_kernel<<<1, SCAN_THREADS, 0, st>>>(P.hist, P.cursor, P.nb);
        KERNEL_CHECK();
        bn_msm_scatter_kernel<<<pointBlocks, POINT_THREADS, 0, st>>>(P, B);
        KERNEL_CHECK();
        bn_msm_accumulate_kernel<<<(P.nb + BUCKET_THREADS - 1) / BUCKET_THREADS, BUCKET_THREADS, 0, st>>>(P);
        KERNEL_CHECK();
    }

    const u32 items = K * plan.nWindows;             // window w of polynomial k is item w * K + k
    uint4 *lvl[2] = { (uint4 *)(base + plan.offLevelA), (uint4 *)(base + plan.offLevelB) };
    const u64 lvlPoints[2] = { (u64)items * plan.m1, (u64)items * plan.m2 };     // X first, Y after it
    LevelParams L;
    L.nWindows = items; L.m = plan.bucketsPerWindow; L.off = 1;
    L.xin = buckets; L.yin = nullptr;
    const uint4 *windows = nullptr;
    for (int level = 0; !windows; level++) {
        const int o = level & 1;
        L.L = level == 0 ? bnp::BN_MSM_L1 : bnp::BN_MSM_L; L.lShift = level == 0 ? 3 : 4;
        L.mOut = (L.m + L.L - 1) / L.L;
        L.xout = lvl[o]; L.yout = lvl[o] + 8 * lvlPoints[o];
        if ((u64)L.nWindows * L.mOut > lvlPoints[o]) return fail(PIL2GL_EINVAL, "MSM reduction level %d does not fit its buffer", level);
        const u32 lanes = L.nWindows * L.mOut;
        bn_msm_reduce_kernel<<<(lanes + BUCKET_THREADS - 1) / BUCKET_THREADS, BUCKET_THREADS, 0, st>>>(L);
        KERNEL_CHECK();
        if (L.mOut == 1) windows = L.yout;
        L.xin = L.xout; L.yin = L.yout; L.m = L.mOut; L.off = 0;
    }
    bn_msm_tail_kernel<<<K, 64, 0, st>>>(windows, plan.nWindows, K, plan.c, (u32 *)out);
    KERNEL_CHECK();
    return PIL2GL_OK;
}

// the single MSM is the batch of one polynomial of one slot: column 0 of a matrix of `stride` elements per row
bnm::MsmBatch single(u64 n, u64 stride) {
    bnm::MsmBatch B{};
    B.K = 1; B.rowStride = (u32)stride; B.rows[0] = (u32)n; B.m[0] = 1;
    return B;
}

}  // namespace

extern "C" {

int pil2gl_debug_bn128_msm_plan(uint64_t n, uint32_t *out, uint64_t *scratchBytes) {
    if (!out || !scratchBytes) return fail(PIL2GL_EINVAL, "null argument");
    if (n > MSM_MAX_N) return fail(PIL2GL_EINVAL, "n = %llu: at most 2^28 points", (unsigned long long)n);
    const bnp::BnMsmPlan p = bnp::bn_msm_plan(n);
    out[0] = p.c; out[1] = p.nWindows; out[2] = p.bucketsPerWindow; out[3] = p.windowsPerPass;
    *scratchBytes = n ? p.scratchBytes : 0;
    return PIL2GL_OK;
}

int pil2gl_debug_bn128_msm_batch_plan(uint32_t K, const uint64_t *counts, uint32_t *out, uint64_t *scratchBytes) {
    if (!counts || !out || !scratchBytes) return fail(PIL2GL_EINVAL, "null argument");
    if (K < 1 || K > bnm::MSM_MAX_POLYS) return fail(PIL2GL_EINVAL, "K = %u polynomials: 1..%u", K, bnm::MSM_MAX_POLYS);
    u64 nTotal = 0;
    for (u32 k = 0; k < K; k++) {
        if (counts[k] > MSM_MAX_N || (nTotal += counts[k]) > MSM_MAX_N) return fail(PIL2GL_EINVAL, "more than 2^28 coefficients in one batch");
    }
    const bnp::BnMsmPlan p = bnp::bn_msm_batch_plan(K, counts);
    out[0] = p.c; out[1] = p.nWindows; out[2] = p.bucketsPerWindow; out[3] = p.windowsPerPass;
    *scratchBytes = nTotal ? p.scratchBytes : 0;
    return PIL2GL_OK;
}

int pil2gl_debug_bn128_commit_locate(const pil2gl_g1_poly *polys, uint32_t K, const uint32_t *slots, uint64_t rowStride, uint64_t lane, uint64_t out[4]) {
    bnm::MsmBatch B;
    u64 nTotal, extent;
    P2_TRY(check_commit(nullptr, MSM_MAX_N, nullptr, rowStride, polys, K, slots, out, B, nTotal, extent, false));
    u32 k = 0, i = 0;
    out[0] = out[1] = out[2] = out[3] = 0;
    if (!bnm::msm_batch_locate(B, lane, k, i)) return fail(PIL2GL_EINVAL, "lane %llu of %llu", (unsigned long long)lane, (unsigned long long)nTotal);
    out[0] = k; out[1] = i;
    out[2] = bnm::msm_batch_element(B, k, i, out[3]) ? 1 : 0;
    return PIL2GL_OK;
}

int pil2gl_debug_bn128_msm_digits(const uint64_t scalar[4], uint32_t c, int32_t *digits, uint32_t room, uint32_t *nDigits) {
    if (!scalar || !nDigits || (!digits && room)) return fail(PIL2GL_EINVAL, "null argument");
    if (c < bnm::MSM_MIN_C || c > bnm::MSM_MAX_C) return fail(PIL2GL_EINVAL, "window width %u outside %u..%u", c, bnm::MSM_MIN_C, bnm::MSM_MAX_C);
    if (scalar[3] >> (bnm::MSM_SCALAR_BITS - 192)) return fail(PIL2GL_EINVAL, "scalar of more than %u bits", bnm::MSM_SCALAR_BITS);
    const uint32_t nW = (bnm::MSM_SCALAR_BITS + 1 + c - 1) / c;
    *nDigits = nW;
    if (nW > room) return fail(PIL2GL_EINVAL, "%u digits, room for %u", nW, room);
    uint32_t s[8], carry = 0;
    for (int i = 0; i < 4; i++) { s[2 * i] = (uint32_t)scalar[i]; s[2 * i + 1] = (uint32_t)(scalar[i] >> 32); }
    for (uint32_t w = 0; w < nW; w++) digits[w] = bnm::msm_next_digit(s, carry, c);
    return PIL2GL_OK;
}

int pil2gl_bn128_g1_msm_dev(const uint64_t *bases, const uint64_t *scalars, uint64_t n, uint64_t scalarStride, uint32_t scalarsMontgomery,
                            uint64_t *out, void *stream) {
    P2_TRY(check_args(bases, scalars, n, scalarStride, out));
    P2_TRY(ensure_init());
    if ((((uintptr_t)bases | (uintptr_t)scalars) & 15) || ((uintptr_t)out & 7)) return fail(PIL2GL_EINVAL, "bases and scalars must be 16-byte aligned, out 8-byte");
    return bn_msm_launch(bases, scalars, single(n, scalarStride), scalarsMontgomery, out, as_stream(stream));
}

int pil2gl_bn128_g1_msm(const uint64_t *bases, const uint64_t *scalars, uint64_t n, uint64_t scalarStride, uint32_t scalarsMontgomery, uint64_t *out) {
    P2_TRY(check_args(bases, scalars, n, scalarStride, out));
    if (n == 0) { for (int i = 0; i < 8; i++) out[i] = 0; return PIL2GL_OK; }
    const uint64_t nScalarWords = ((n - 1) * scalarStride + 1) * 4;      // up to the last element read
    Stage s(8 * n + nScalarWords + 8);
    P2_TRY(s.rc());
    const uint64_t *dBases = s.put(bases, 8 * n), *dScalars = s.put(scalars, nScalarWords);
    uint64_t *dOut = s.take(8);
    P2_TRY(s.rc());
    P2_TRY(bn_msm_launch(dBases, dScalars, single(n, scalarStride), scalarsMontgomery, dOut, 0));
    return s.get(out, dOut, 8);
}

int pil2gl_bn128_g1_commit_dev(const uint64_t *bases, uint64_t nBases, const uint64_t *scalars, uint64_t rowStride, uint32_t scalarsMontgomery,
                               const pil2gl_g1_poly *polys, uint32_t K, const uint32_t *slots, uint64_t *out, void *stream) {
    bnm::MsmBatch B;
    u64 nTotal, extent;
    P2_TRY(check_commit(bases, nBases, scalars, rowStride, polys, K, slots, out, B, nTotal, extent));
    if ((((uintptr_t)bases | (uintptr_t)scalars) & 15) || ((uintptr_t)out & 7)) return fail(PIL2GL_EINVAL, "bases and scalars must be 16-byte aligned, out 8-byte");
    P2_TRY(ensure_init());
    return bn_msm_launch(bases, scalars, B, scalarsMontgomery, out, as_stream(stream));
}

int pil2gl_bn128_g1_commit(const uint64_t *bases, uint64_t nBases, const uint64_t *scalars, uint64_t rowStride, uint32_t scalarsMontgomery,
                           const pil2gl_g1_poly *polys, uint32_t K, const uint32_t *slots, uint64_t *out) {
    bnm::MsmBatch B;
    u64 nTotal, extent;
    P2_TRY(check_commit(bases, nBases, scalars, rowStride, polys, K, slots, out, B, nTotal, extent));
    if (nTotal == 0) { for (u32 i = 0; i < 8 * K; i++) out[i] = 0; return PIL2GL_OK; }
    u64 nMax = 0;                                    // the bases any polynomial reaches; the scalars up to the last element read
    for (u32 k = 0; k < K; k++) nMax = std::max<u64>(nMax, bnm::msm_batch_count(B, k));
    Stage s(8 * nMax + 4 * extent + 8 * K);
    P2_TRY(s.rc());
    const uint64_t *dBases = s.put(bases, 8 * nMax), *dScalars = s.put(scalars, 4 * extent);
    uint64_t *dOut = s.take(8 * K);
    P2_TRY(s.rc());
    P2_TRY(bn_msm_launch(dBases, dScalars, B, scalarsMontgomery, dOut, 0));
    return s.get(out, dOut, 8 * K);
}

}  // extern "C"
