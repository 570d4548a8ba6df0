// Multi-scalar multiplication over BN254 G1, gfx950: the device twin of G1.toAffine(G1.multiExpAffine(bases, scalars)), the commitment step
// of the fflonk prover (fflonk_prover_helpers.js:185,336, fflonk_setup.js:52).  out = sum_i s_i P_i by the bucket (Pippenger) method, one
// path for every n >= 1 (bnp::bn_msm_plan gives the window width c, the windows and how many of them a pass takes):
//
//   per pass of windowsPerPass windows
//     histogram   a lane per point: the scalar leaves Montgomery form (one fr_mul by 1) if it came in it, is recoded into signed digits
//                 (bn_msm_recode.h) and counts one into the bucket (window, |digit|) of every non-zero digit of the pass's windows.  Zero
//                 digits and points at infinity are dropped here.
//     scan        one workgroup: exclusive prefix sums of the histogram in place, a copy as the scatter's cursors.
//     scatter     the histogram's lanes again: each non-zero digit takes the next slot of its bucket and writes index | sign << 31.
//     accumulate  a lane per bucket: its points, fetched by index one ahead of their use, summed by the mixed addition (bn_g1.cuh).  A bucket
//                 that holds all n points is slow but no different.  Every bucket of the pass is written, the empty ones as infinity:
//                 nothing of an earlier call or pass is read.
//   reduce        sum_k k B_k of every window by running sums, in levels: a lane takes L consecutive items (X_i, Y_i) of a window and leaves
//                 X' = L sum X_i, Y' = sum Y_i + sum (i mod L + off) X_i, so that sum_i (Y_i + (i + off) X_i) = sum_seg (Y'_seg + seg X'_seg):
//                 the same problem on 1/L of the items, with off = 0.  Level 1 reads the buckets (Y absent, off = 1: bucket i stands for
//                 digit i + 1); the last level leaves one Y per window.
//   tail          one lane: Horner over the windows (c doublings, one addition each), the inversion for to-affine, the 64 output bytes.
//
// Memory safety does not rest on the sort being right: a list position is clamped to the list, a point index is used only below n, a
// bucket index only below the pass's bucket count, and every loop over device-computed bounds runs at most n times.
#include "common.h"
#include "bn_params.h"
#include "bn_msm_recode.h"
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
    u64 n, stride, cap;                              // cap: entries the list has room for (n * windows of the pass)
    u32 mont, c, nbw, w0, g, nb;                     // nb = g * nbw buckets in this pass
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

// emit(bucket of the pass, negative) for every non-zero digit of point i in the pass's windows
template <class F>
__device__ __forceinline__ void for_each_digit(const PassParams &P, u64 i, F emit) {
    const uint4 *b = P.bases + 4 * i;
    const uint4 b0 = b[0], b1 = b[1], b2 = b[2], b3 = b[3];
    if (((b0.x | b0.y | b0.z | b0.w) | (b1.x | b1.y | b1.z | b1.w) | (b2.x | b2.y | b2.z | b2.w) | (b3.x | b3.y | b3.z | b3.w)) == 0) return;
    const uint4 *sp = P.scalars + 2 * i * P.stride;
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
        emit((w - P.w0) * P.nbw + mag - 1, d < 0);
    }
}

__global__ void __launch_bounds__(POINT_THREADS) bn_msm_hist_kernel(PassParams P) {
    const u64 i = (u64)blockIdx.x * POINT_THREADS + threadIdx.x;
    if (i >= P.n) return;
    for_each_digit(P, i, [&](u32 bucket, bool) { atomicAdd(&P.hist[bucket], 1u); });
}

// hist[0..nb) -> its exclusive prefix sums, hist[nb] = the total; cursor = a copy of the sums
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

__global__ void __launch_bounds__(POINT_THREADS) bn_msm_scatter_kernel(PassParams P) {
    const u64 i = (u64)blockIdx.x * POINT_THREADS + threadIdx.x;
    if (i >= P.n) return;
    for_each_digit(P, i, [&](u32 bucket, bool neg) {
        const u32 pos = atomicAdd(&P.cursor[bucket], 1u);
        if (pos < P.cap) P.entries[pos] = (u32)i | (neg ? ~ENTRY_INDEX_MASK : 0u);
    });
}

__device__ __forceinline__ void ld_base(const PassParams &P, u64 pos, u32 x[8], u32 y[8], u32 &entry) {
    entry = P.entries[pos];
    const u64 idx = entry & ENTRY_INDEX_MASK;
    const uint4 *b = P.bases + 4 * (idx < P.n ? idx : 0);    // an index the scatter cannot have written reads point 0 and is skipped below
    const uint4 b0 = b[0], b1 = b[1], b2 = b[2], b3 = b[3];
    unpack(b0, b1, x); unpack(b2, b3, y);
}

__global__ void __launch_bounds__(BUCKET_THREADS) bn_msm_accumulate_kernel(PassParams P) {
    const u32 b = blockIdx.x * BUCKET_THREADS + threadIdx.x;
    if (b >= P.nb) return;
    u64 end = P.hist[b + 1], start = P.hist[b];
    if (end > P.cap) end = P.cap;
    if (start > end) start = end;
    if (end - start > P.n) end = start + P.n;        // a bucket holds each point at most once
    G1X acc;
    bn::g1_set_inf(acc);
    u32 nx[8], ny[8], nxtEntry = ENTRY_INDEX_MASK;   // the point after the current one, already on its way
#pragma unroll
    for (int l = 0; l < 8; l++) nx[l] = ny[l] = 0;
    if (start < end) ld_base(P, start, nx, ny, nxtEntry);
    for (u64 p = start; p < end; p++) {
        u32 x[8], y[8];
        const u32 entry = nxtEntry;
        bn::fq_copy(x, nx); bn::fq_copy(y, ny);
        if (p + 1 < end) ld_base(P, p + 1, nx, ny, nxtEntry);
        if ((entry & ENTRY_INDEX_MASK) < P.n) {
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

// windows: one point per window (the last level's Y);  out: the affine sum, 64 bytes
__global__ void __launch_bounds__(64) bn_msm_tail_kernel(const uint4 *windows, u32 nWindows, u32 c, u32 *out) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    G1X r, v;
    bn::g1_set_inf(r);
    for (int w = (int)nWindows - 1; w >= 0; w--) {
        for (u32 k = 0; k < c; k++) bn::g1_dbl(r);
        ld_point(windows + 8 * (u64)w, v);
        bn::g1_add(r, v);
    }
    u32 x[8], y[8];
    bn::g1_to_affine(r, x, y);
    for (int i = 0; i < 8; i++) { out[i] = x[i]; out[8 + i] = y[i]; }
}

int check_args(const void *bases, const void *scalars, u64 n, u64 stride, const void *out) {
    if (n > MSM_MAX_N) return fail(PIL2GL_EINVAL, "n = %llu: at most 2^28 points", (unsigned long long)n);
    if (stride == 0 || stride >> 32) return fail(PIL2GL_EINVAL, "scalarStride must be in 1..2^32-1");
    if (!out || (n && (!bases || !scalars))) return fail(PIL2GL_EINVAL, "null buffer");
    return PIL2GL_OK;
}

int bn_msm_launch(const u64 *bases, const u64 *scalars, u64 n, u64 stride, u32 mont, u64 *out, hipStream_t st) {
    if (n == 0) { HIP_TRY(hipMemsetAsync(out, 0, 64, st)); return PIL2GL_OK; }
    const bnp::BnMsmPlan plan = bnp::bn_msm_plan(n);
    u64 *work = nullptr;
    P2_TRY(scratch(SCR_BN_MSM, (plan.scratchBytes + 7) / 8, &work));
    char *base = (char *)work;
    uint4 *buckets = (uint4 *)(base + plan.offBuckets);

    PassParams P;
    P.bases = (const uint4 *)bases; P.scalars = (const uint4 *)scalars;
    P.n = n; P.stride = stride; P.mont = mont ? 1u : 0u; P.c = plan.c; P.nbw = plan.bucketsPerWindow;
    P.hist = (u32 *)(base + plan.offHist); P.cursor = (u32 *)(base + plan.offCursor); P.entries = (u32 *)(base + plan.offEntries);
    const unsigned pointBlocks = (unsigned)((n + POINT_THREADS - 1) / POINT_THREADS);
    for (u32 w0 = 0; w0 < plan.nWindows; w0 += plan.windowsPerPass) {
        P.w0 = w0; P.g = plan.nWindows - w0 < plan.windowsPerPass ? plan.nWindows - w0 : plan.windowsPerPass;
        P.nb = P.g * P.nbw; P.cap = n * P.g;
        P.buckets = buckets + 8 * (u64)w0 * P.nbw;
        HIP_TRY(hipMemsetAsync(P.hist, 0, ((u64)P.nb + 1) * 4, st));      // per call and per pass: no count survives
        bn_msm_hist_kernel<<<pointBlocks, POINT_THREADS, 0, st>>>(P);
        KERNEL_CHECK();
        bn_msm_scan_kernel<<<1, SCAN_THREADS, 0, st>>>(P.hist, P.cursor, P.nb);
        KERNEL_CHECK();
        bn_msm_scatter_kernel<<<pointBlocks, POINT_THREADS, 0, st>>>(P);
        KERNEL_CHECK();
        bn_msm_accumulate_kernel<<<(P.nb + BUCKET_THREADS - 1) / BUCKET_THREADS, BUCKET_THREADS, 0, st>>>(P);
        KERNEL_CHECK();
    }

    uint4 *lvl[2] = { (uint4 *)(base + plan.offLevelA), (uint4 *)(base + plan.offLevelB) };
    const u64 lvlPoints[2] = { (u64)plan.nWindows * plan.m1, (u64)plan.nWindows * plan.m2 };     // X first, Y after it
    LevelParams L;
    L.nWindows = plan.nWindows; L.m = plan.bucketsPerWindow; L.off = 1;
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
    bn_msm_tail_kernel<<<1, 64, 0, st>>>(windows, plan.nWindows, plan.c, (u32 *)out);
    KERNEL_CHECK();
    return PIL2GL_OK;
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
    return bn_msm_launch(bases, scalars, n, scalarStride, scalarsMontgomery, out, as_stream(stream));
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
    P2_TRY(bn_msm_launch(dBases, dScalars, n, scalarStride, scalarsMontgomery, dOut, 0));
    return s.get(out, dOut, 8);
}

}  // extern "C"
