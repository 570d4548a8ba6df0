// The plookup hint over the BN254 scalar field Fr, gfx950: calculateH1H2(F, f, t) of src/helpers/polutils.js:105-130 with F = curve.Fr,
// the last branch of resolveHint (src/prover/hints_helpers.js:115-121).  The reference builds s = [(t[i], i)] ++ [(f[j], idx_t[f[j]])]
// with idx_t[v] the LAST i with t[i] = v, sorts it stably by the index and reads h1[i] = s[2i], h2[i] = s[2i+1].  Every entry of one
// index carries the same value, so the sorted sequence is "t[i] repeated 1 + cnt[i] times, i = 0 .. n - 1", cnt[i] = #{j : f[j] = t[i]}
// when i is the last occurrence of its value and 0 otherwise.  No sort and no field arithmetic: two elements are the same value exactly
// when their 32 bytes are equal.
//
//   insert   a lane per row of t: an open-addressing table (linear probing, 4-byte slots, bnh1h2::EMPTY or an index into t) from value
//            to the last index holding it: claim an empty slot with a compare-and-swap, or raise the slot of an equal value with an
//            atomic maximum.  A slot never returns to EMPTY and only ever moves between indices of ONE value, so a stale read of it still
//            compares right.
//   count    a lane per row of f: find the slot of f[j], add 1 to cnt[its index]; an EMPTY slot on the way means f[j] is not in t: an
//            atomic minimum of j into the missing cell.
//   -- the host reads the missing cell back (8 bytes) and refuses here; nothing below has been launched then --
//   scan     cnt[i] -> the exclusive running sum of 1 + cnt[i] within a chunk of 2048 groups, in place, and the chunks' totals; one
//            workgroup then turns the at most 2^17 totals into the chunks' first positions.  start(g) = start[g] + totals[g / 2048].
//   expand   a workgroup per 512 output rows (positions P = 1024 b .. P + 1023): ONE search of the whole start() for g0, the group position P
//            falls in -- 256-ary, a probe per lane and a ballot count, at most 4 rounds -- then the starts of the next 1023 groups into
//            LDS (every group holds at least one position, so no later group begins inside the workgroup's positions) and a 10-step
//            search of LDS per position.  A lane takes rows r and r + 256: h1[r] = t[g(2r)], h2[r] = t[g(2r + 1)], the second group
//            being the first or the one after it.
// Which table slot a value ends up in depends on the order the atomics land in; what the slot of a value HOLDS at the end (the largest
// index), the counts and so every output word do not.
//
// Every probe loop runs at most `cap` times whatever the data; the table has at least 2 n slots for at most n values, so an empty slot
// ends every unsuccessful probe long before.  Memory safety rests on no multiple: a lane with i >= n returns or idles at the barriers.
#include "bn_column_stage.h"
#include "bn_h1h2_plan.h"

using namespace pil2gl;

namespace {

using bnh1h2::EMPTY;
using bnh1h2::THREADS;
using bnh1h2::SCAN_ITEMS;
using bnh1h2::SCAN_CHUNK;
using bnh1h2::SCAN_CHUNK_BITS;
using bnh1h2::EXPAND_ROWS;

struct Key { uint4 lo, hi; };

struct Args {
    const uint4 *f; u64 fs;                          // element i of a column at its pointer + 2 i stride (16-byte halves)
    const uint4 *t; u64 ts;
    uint4 *h1; u64 h1s;
    uint4 *h2; u64 h2s;
    u32 *table; u32 mask;                            // cap slots, mask = cap - 1
    u32 *start;                                      // n: counts, then the starts within their chunk
    u32 *totals;                                     // ceil(n / SCAN_CHUNK)
    unsigned long long *missing;
    u32 n, nChunks;
};

__device__ __forceinline__ Key ld_key(const uint4 *col, u64 stride, u32 i) {
    const uint4 *p = col + 2 * (size_t)i * stride;
    return Key{ p[0], p[1] };
}
__device__ __forceinline__ void st_key(uint4 *col, u64 stride, u32 i, const Key &k) {
    uint4 *p = col + 2 * (size_t)i * stride;
    p[0] = k.lo; p[1] = k.hi;
}
// all eight limbs, or two values that differ in one would be one group
__device__ __forceinline__ bool key_eq(const Key &a, const Key &b) {
    return ((a.lo.x ^ b.lo.x) | (a.lo.y ^ b.lo.y) | (a.lo.z ^ b.lo.z) | (a.lo.w ^ b.lo.w) |
            (a.hi.x ^ b.hi.x) | (a.hi.y ^ b.hi.y) | (a.hi.z ^ b.hi.z) | (a.hi.w ^ b.hi.w)) == 0;
}
// 32-bit operations only (the chip has no 64-bit multiply): every limb is xored in and multiplied through, murmur3's finaliser at the end
__device__ __forceinline__ u32 key_hash(const Key &k) {
    const u32 w[8] = { k.lo.x, k.lo.y, k.lo.z, k.lo.w, k.hi.x, k.hi.y, k.hi.z, k.hi.w };
    u32 h = 0x9E3779B9u;
#pragma unroll
    for (int i = 0; i < 8; i++) { h = (h ^ w[i]) * 0x85EBCA6Bu; h ^= h >> 15; }
    h *= 0xC2B2AE35u;
    return h ^ (h >> 16);
}

__global__ void __launch_bounds__(THREADS) bn_h1h2_insert_kernel(Args a) {
    const u32 i = blockIdx.x * THREADS + threadIdx.x;
    if (i >= a.n) return;
    const Key k = ld_key(a.t, a.ts, i);
    u32 s = key_hash(k) & a.mask;
    for (u32 probe = 0; probe <= a.mask; probe++, s = (s + 1) & a.mask) {
        u32 cur = a.table[s];
        if (cur == EMPTY) {
            cur = atomicCAS(&a.table[s], EMPTY, i);
            if (cur == EMPTY) return;                                        // claimed
        }
        if (cur < a.n && key_eq(k, ld_key(a.t, a.ts, cur))) { atomicMax(&a.table[s], i); return; }      // the same value: keep the last index
    }
}

__global__ void __launch_bounds__(THREADS) bn_h1h2_count_kernel(Args a) {
    const u32 j = blockIdx.x * THREADS + threadIdx.x;
    if (j >= a.n) return;
    const Key k = ld_key(a.f, a.fs, j);
    u32 s = key_hash(k) & a.mask;
    for (u32 probe = 0; probe <= a.mask; probe++, s = (s + 1) & a.mask) {
        const u32 cur = a.table[s];
        if (cur >= a.n) break;                                               // EMPTY: not in t
        if (key_eq(k, ld_key(a.t, a.ts, cur))) { atomicAdd(&a.start[cur], 1u); return; }
    }
    atomicMin(a.missing, (unsigned long long)j);                             // "Number not included" (polutils.js:115)
}

// the exclusive scan of the workgroup's THREADS values (LDS, log steps); *total = their sum
__device__ __forceinline__ u32 block_exclusive(u32 v, u32 *sh, u32 *total) {
    sh[threadIdx.x] = v;
    __syncthreads();
    for (u32 d = 1; d < THREADS; d <<= 1) {
        u32 x = sh[threadIdx.x];
        if (threadIdx.x >= d) x += sh[threadIdx.x - d];
        __syncthreads();
        sh[threadIdx.x] = x;
        __syncthreads();
    }
    *total = sh[THREADS - 1];
    return threadIdx.x ? sh[threadIdx.x - 1] : 0;
}

// start[i]: cnt[i] -> sum over the chunk's k < i of (1 + cnt[k]); totals[chunk] = the chunk's sum
__global__ void __launch_bounds__(THREADS) bn_h1h2_scan_kernel(Args a) {
    __shared__ u32 sh[THREADS];
    const u32 base = blockIdx.x * SCAN_CHUNK + threadIdx.x * SCAN_ITEMS;
    u32 loc[SCAN_ITEMS], run = 0;
#pragma unroll
    for (u32 k = 0; k < SCAN_ITEMS; k++) { loc[k] = run; if (base + k < a.n) run += 1 + a.start[base + k]; }
    u32 total;
    const u32 ex = block_exclusive(run, sh, &total);
#pragma unroll
    for (u32 k = 0; k < SCAN_ITEMS; k++) if (base + k < a.n) a.start[base + k] = ex + loc[k];
    if (threadIdx.x == 0) a.totals[blockIdx.x] = total;
}

// totals: the chunks' sums -> the chunks' first positions; one workgroup, a lane per run of ceil(nChunks / THREADS) chunks
__global__ void __launch_bounds__(THREADS) bn_h1h2_totals_kernel(Args a) {
    __shared__ u32 sh[THREADS];
    const u32 per = (a.nChunks + THREADS - 1) / THREADS;
    const u32 b = threadIdx.x * per, e = b + per < a.nChunks ? b + per : a.nChunks;
    u32 run = 0;
    for (u32 c = b; c < e; c++) run += a.totals[c];
    u32 total;
    u32 acc = block_exclusive(run, sh, &total);
    for (u32 c = b; c < e; c++) { const u32 v = a.totals[c]; a.totals[c] = acc; acc += v; }
}

__device__ __forceinline__ u32 group_start(const Args &a, u32 g) { return a.start[g] + a.totals[g >> SCAN_CHUNK_BITS]; }

__global__ void __launch_bounds__(THREADS) bn_h1h2_expand_kernel(Args a) {
    __shared__ u32 sh[2 * EXPAND_ROWS];                                      // sh[j] = start(g0 + 1 + j), EMPTY past the last group
    const u32 row0 = blockIdx.x * EXPAND_ROWS, pos0 = 2 * row0;
    // g0 = the last group with start(g) <= pos0, among [lo, hi); start(0) = 0 keeps lo in it.  A lane probes lo + lane * step: the probes
    // that hold are a prefix, so their count places g0 within one step.  The length falls to ceil(length / 256) whatever the data.
    u32 lo = 0, hi = a.n;
    for (int round = 0; round < 4 && hi - lo > 1; round++) {
        const u32 step = (hi - lo + THREADS - 1) / THREADS;
        const u64 g = (u64)lo + (u64)threadIdx.x * step;
        const int holds = g < hi && group_start(a, (u32)g) <= pos0;
        int c = __syncthreads_count(holds);
        if (c < 1) c = 1;
        lo += (u32)(c - 1) * step;
        if (hi - lo > step) hi = lo + step;
    }
    const u32 g0 = lo;
    for (u32 j = threadIdx.x; j < 2 * EXPAND_ROWS; j += THREADS) {
        const u64 g = (u64)g0 + 1 + j;
        sh[j] = g < a.n ? group_start(a, (u32)g) : EMPTY;
    }
    __syncthreads();
    for (u32 r = row0 + threadIdx.x; r < row0 + EXPAND_ROWS && r < a.n; r += THREADS) {
        const u32 p = 2 * r;
        u32 c = 0;                                                           // the number of j with sh[j] <= p: the starts ascend
#pragma unroll
        for (u32 bit = EXPAND_ROWS; bit > 0; bit >>= 1) if (sh[c + bit - 1] <= p) c += bit;
        const u32 ga = g0 + c;
        const u32 gb = c < 2 * EXPAND_ROWS && sh[c] <= p + 1 ? ga + 1 : ga;  // sh[c] is the first start above p
        const Key ka = ld_key(a.t, a.ts, ga);
        st_key(a.h1, a.h1s, r, ka);
        st_key(a.h2, a.h2s, r, gb == ga ? ka : ld_key(a.t, a.ts, gb));
    }
}

struct Cols {
    const u64 *f; u64 fs; const u64 *t; u64 ts; u64 n; u64 *h1; u64 h1s; u64 *h2; u64 h2s;
};

// everything up to the check, the readback, then the rest; *missing = UINT64_MAX or the lowest j with f[j] not in t
int run(const Cols &c, hipStream_t st, u64 *missing) {
    const bnh1h2::Plan p = bnh1h2::plan(c.n);
    u64 *d = nullptr;
    P2_TRY(scratch(SCR_BN_H1H2, (p.words + 1) / 2, &d));
    u32 *w = (u32 *)d;
    Args a{};
    a.f = (const uint4 *)c.f; a.fs = c.fs; a.t = (const uint4 *)c.t; a.ts = c.ts;
    a.h1 = (uint4 *)c.h1; a.h1s = c.h1s; a.h2 = (uint4 *)c.h2; a.h2s = c.h2s;
    a.table = w + p.tableOff; a.mask = (u32)(p.cap - 1);
    a.start = w + p.startOff; a.totals = w + p.totalsOff; a.missing = (unsigned long long *)(w + p.missingOff);
    a.n = (u32)c.n; a.nChunks = p.scanBlocks;
    HIP_TRY(hipMemsetAsync(a.table, 0xFF, 4 * p.cap, st));
    HIP_TRY(hipMemsetAsync(a.start, 0, 4 * c.n, st));
    HIP_TRY(hipMemsetAsync(a.missing, 0xFF, 8, st));
    bn_h1h2_insert_kernel<<<p.rowBlocks, THREADS, 0, st>>>(a);
    KERNEL_CHECK();
    bn_h1h2_count_kernel<<<p.rowBlocks, THREADS, 0, st>>>(a);
    KERNEL_CHECK();
    unsigned long long miss = 0;
    HIP_TRY(hipMemcpyAsync(&miss, a.missing, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    *missing = miss;
    if (miss != ~0ull) return fail(PIL2GL_EINVAL, "Number not included: w:%llu", miss);      // polutils.js:115; h1, h2 untouched
    bn_h1h2_scan_kernel<<<p.scanBlocks, THREADS, 0, st>>>(a);
    KERNEL_CHECK();
    bn_h1h2_totals_kernel<<<1, THREADS, 0, st>>>(a);
    KERNEL_CHECK();
    bn_h1h2_expand_kernel<<<p.expandBlocks, THREADS, 0, st>>>(a);
    KERNEL_CHECK();
    return PIL2GL_OK;
}

int check(const Cols &c) {
    P2_TRY(check_column(c.f, c.n, c.fs, "f"));
    P2_TRY(check_column(c.t, c.n, c.ts, "t"));
    P2_TRY(check_column(c.h1, c.n, c.h1s, "h1"));
    P2_TRY(check_column(c.h2, c.n, c.h2s, "h2"));
    // an output against an input or the other output: they must share no element (bn_column.h: apart, or two columns of one section)
    auto apart = [&](const void *a, u64 as, const void *b, u64 bs) { return bncol::relation((uintptr_t)a, as, (uintptr_t)b, bs, c.n) == bncol::APART; };
    const bool ok = apart(c.f, c.fs, c.h1, c.h1s) && apart(c.t, c.ts, c.h1, c.h1s) && apart(c.f, c.fs, c.h2, c.h2s) &&
                    apart(c.t, c.ts, c.h2, c.h2s) && apart(c.h1, c.h1s, c.h2, c.h2s);
    if (!ok) return fail(PIL2GL_EINVAL, "an output overlaps an input or the other output (only columns of one section may interleave)");
    return PIL2GL_OK;
}

}  // namespace

extern "C" {

int pil2gl_debug_bn128_h1h2_plan(uint64_t n, uint32_t *outInfo, uint64_t *scratchBytes) {
    if (!outInfo || !scratchBytes) return fail(PIL2GL_EINVAL, "null argument");
    if (const char *m = bncol::check_size(n)) return fail(PIL2GL_EINVAL, "n = %llu: %s", (unsigned long long)n, m);
    const bnh1h2::Plan p = bnh1h2::plan(n);
    outInfo[0] = (uint32_t)p.cap; outInfo[1] = THREADS; outInfo[2] = SCAN_CHUNK; outInfo[3] = p.scanBlocks;
    outInfo[4] = EXPAND_ROWS; outInfo[5] = p.expandBlocks;
    *scratchBytes = n ? bnh1h2::scratch_bytes(p) : 0;
    return PIL2GL_OK;
}

int pil2gl_bn128_h1h2_dev(const uint64_t *f, uint64_t fStride, const uint64_t *t, uint64_t tStride, uint64_t n,
                          uint64_t *h1, uint64_t h1Stride, uint64_t *h2, uint64_t h2Stride, uint64_t *missingRow, void *stream) {
    uint64_t miss = ~0ull;
    if (missingRow) *missingRow = miss;
    const Cols c{ f, fStride, t, tStride, n, h1, h1Stride, h2, h2Stride };
    P2_TRY(check(c));
    if (n == 0) return PIL2GL_OK;
    P2_TRY(check_aligned16({ f, t, h1, h2 }));
    P2_TRY(ensure_init());
    const int rc = run(c, as_stream(stream), &miss);
    if (missingRow) *missingRow = miss;
    return rc;
}

int pil2gl_bn128_h1h2(const uint64_t *f, uint64_t fStride, const uint64_t *t, uint64_t tStride, uint64_t n,
                      uint64_t *h1, uint64_t h1Stride, uint64_t *h2, uint64_t h2Stride, uint64_t *missingRow) {
    uint64_t miss = ~0ull;
    if (missingRow) *missingRow = miss;
    const Cols c{ f, fStride, t, tStride, n, h1, h1Stride, h2, h2Stride };
    P2_TRY(check(c));
    if (n == 0) return PIL2GL_OK;
    // two outputs of one section are one staged range, so that neither copy back undoes the other (bn_column.h)
    const bncol::Col cols[4] = { { (uintptr_t)f, n, fStride, true, false }, { (uintptr_t)t, n, tStride, true, false },
                                 { (uintptr_t)h1, n, h1Stride, false, true }, { (uintptr_t)h2, n, h2Stride, false, true } };
    ColumnStage s(cols, 4);
    P2_TRY(s.rc());
    const int rc = run(Cols{ s.dev(0), fStride, s.dev(1), tStride, n, s.dev(2), h1Stride, s.dev(3), h2Stride }, 0, &miss);
    if (missingRow) *missingRow = miss;
    P2_TRY(rc);
    return s.copy_back();
}

}  // extern "C"
