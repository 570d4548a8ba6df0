// The connection polynomials of a recursion circuit on the device, gfx950: the constant columns S[0 .. nCols) that the compressor and final
// setups build with two host loops (src/compressor/compressor12_setup.js:470-500, compressor18_setup.js:534-560, src/final/final6_setup.js:
// 243-270, final9_setup.js:264-290, finalfflonk_setup.js:136-163 over curve.Fr, test/plonk2pil/plonksetup.js:79-105):
//   S[j][i] = id(i, j) = w^i ks'[j]  (ks'[0] = 1, ks'[j] = ks[j - 1]),  then for every cell (i, j) in row-major order whose signal was seen
//   before: connect(S[first.col], first.row, S[j], i), a swap with the signal's FIRST cell (polutils.js:166).
// Closed form.  With c_0 < c_1 < ... < c_k the cells of one signal in flat order i nCols + j, the swaps leave S[c_m] = id(c_{m-1}) for m >= 1
// and S[c_0] = id(c_k): the first cell always holds the identity of the cell seen last.  So the job is pred[c] = the previous cell with the
// same signal (the group's last cell for its first), and S[c] = id(pred[c]).  The order inside a group is exact: another cycle through the
// same cells is a valid permutation argument with other constant columns, another constant root and another verification key.
//   step 1, pred   init: keys[c] = sMap[c] (0 for an index >= nW, whose flat cell is lowered into the bad cell by an atomic minimum), cells[c] = c.
//                  A stable least-significant-digit radix sort of (key, cell) by key, 8 bits a pass, connplan::Plan::passes passes (the
//                  digits above nW's highest are zero).  A pass: histogram of a workgroup's TILE cells in LDS -> hist[digit][workgroup];
//                  exclusive scan of hist (chunk totals, their scan by one workgroup, the chunks); scatter.  In the scatter wave v of a
//                  workgroup owns cells [v 64 ROUNDS, (v + 1) 64 ROUNDS) of the tile and walks them 64 at a time: the lanes with one digit
//                  find each other with eight ballots, their leader takes popcount slots from the wave's LDS cursor with one atomic, and
//                  a lane's slot is the leader's old value plus the peers below it -- cell order is kept within a round, across rounds,
//                  across waves (cursors start at the exclusive sum over lower waves) and across workgroups (the scanned histogram).
//                  All cells enter, the zero cells as one group that the link step skips: no compaction pass, 16 bytes a cell.
//                  link: sorted position p takes cells[p - 1] when keys[p - 1] is its key, else the last cell of its run, found by
//                  bisection over the sorted keys -- log2(cells) reads whatever the group's size.
//   step 2, fill   tables: hi[t] = w^(t 2^loBits), lo[j][t] = w^t ks'[j], a lane per entry by square and multiply (2^loBits ~ sqrt N entries
//                  a column: no N-element table, no serial chain).  fill: a lane per cell of the N x nCols output, ONE product,
//                  lo[pj][pi mod 2^loBits] hi[pi >> loBits] for (pi, pj) = pred of the cell, the cell itself for rows >= nRows.
// Goldilocks: w and ks' words in [p, 2^64) count as their value mod p, outputs canonical.  Fr: Montgomery words in and out, any 256-bit
// pattern counting as its value mod r, outputs canonical.
//
// Safety: sMap values are only compared and sorted, never used as an address.  The scatter's slots follow from the histogram of the same
// cells and are checked against the cell count all the same; pred entries are checked against it before they index the tables.
// Shared with wtns_exec.hip: the bad-cell report, the cell walk, the fields as template parameters (smap_cells.cuh); grid, overlap, narrowing (smap_plan.h).
#include "common.h"
#include "smap_cells.cuh"
#include "conn_plan.h"
#include <string.h>
#include <vector>

using namespace pil2gl;

namespace {

using namespace smapcells;
using namespace smapplan;
using namespace connplan;

template <class F> struct Consts { typename F::Elem w, ks[MAX_COLS]; };      // w and ks' as the caller gave them, a kernel argument

// ---- step 1: predecessor links ----
__global__ void __launch_bounds__(THREADS) conn_init_kernel(const u32 *__restrict__ sMap, u32 n, u32 nW, u32 *__restrict__ keys, u32 *__restrict__ cells,
                                                            unsigned long long *firstBad) {
    u64 best = NO_BAD;
    for (u64 c = (u64)blockIdx.x * THREADS + threadIdx.x; c < n; c += (u64)gridDim.x * THREADS) {
        u32 s = sMap[c];
        if (s >= nW) { best = c < best ? c : best; s = 0; }
        keys[c] = s;
        cells[c] = (u32)c;
    }
    report_bad(best, firstBad);
}

__global__ void __launch_bounds__(THREADS) conn_hist_kernel(const u32 *__restrict__ keys, u32 n, u32 shift, u32 *__restrict__ hist, u32 nBlocks) {
    __shared__ u32 h[BINS];
    h[threadIdx.x] = 0;
    __syncthreads();
    const u64 first = (u64)blockIdx.x * TILE + threadIdx.x;
    for (u32 r = 0; r < ROUNDS; r++) {
        const u64 idx = first + (u64)r * THREADS;
        if (idx < n) atomicAdd(&h[(keys[idx] >> shift) & (BINS - 1)], 1u);
    }
    __syncthreads();
    hist[(u64)threadIdx.x * nBlocks + blockIdx.x] = h[threadIdx.x];
}

// exclusive prefix of v over the workgroup's lanes and the workgroup's total; every lane arrives
__device__ __forceinline__ u32 block_scan(u32 v, u32 *lds, u32 *total) {
    const u32 t = threadIdx.x;
    lds[t] = v;
    __syncthreads();
    for (u32 o = 1; o < THREADS; o <<= 1) {
        const u32 x = t >= o ? lds[t - o] : 0;
        __syncthreads();
        lds[t] += x;
        __syncthreads();
    }
    const u32 incl = lds[t];
    *total = lds[THREADS - 1];
    __syncthreads();
    return incl - v;
}

__global__ void __launch_bounds__(THREADS) conn_scan_sums_kernel(const u32 *__restrict__ a, u32 len, u32 *__restrict__ sums) {
    __shared__ u32 lds[THREADS];
    const u64 first = (u64)blockIdx.x * SCAN_CHUNK + (u64)threadIdx.x * SCAN_ITEMS;
    u32 v = 0, total;
    for (u32 k = 0; k < SCAN_ITEMS; k++) if (first + k < len) v += a[first + k];
    block_scan(v, lds, &total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// one workgroup: sums -> their exclusive prefix, in place
__global__ void __launch_bounds__(THREADS) conn_scan_top_kernel(u32 *sums, u32 m) {
    __shared__ u32 lds[THREADS];
    u32 carry = 0;
    for (u32 base = 0; base < m; base += THREADS) {
        const u32 idx = base + threadIdx.x;
        const u32 v = idx < m ? sums[idx] : 0;
        u32 total;
        const u32 ex = block_scan(v, lds, &total);
        if (idx < m) sums[idx] = carry + ex;
        carry += total;
    }
}

__global__ void __launch_bounds__(THREADS) conn_scan_apply_kernel(u32 *a, u32 len, const u32 *__restrict__ sums) {
    __shared__ u32 lds[THREADS];
    const u64 first = (u64)blockIdx.x * SCAN_CHUNK + (u64)threadIdx.x * SCAN_ITEMS;
    u32 x[SCAN_ITEMS], v = 0, total;
#pragma unroll
    for (u32 k = 0; k < SCAN_ITEMS; k++) { x[k] = first + k < len ? a[first + k] : 0; v += x[k]; }
    u32 run = block_scan(v, lds, &total) + sums[blockIdx.x];
#pragma unroll
    for (u32 k = 0; k < SCAN_ITEMS; k++) { if (first + k < len) a[first + k] = run; run += x[k]; }
}

__global__ void __launch_bounds__(THREADS) conn_scatter_kernel(const u32 *__restrict__ keysIn, const u32 *__restrict__ cellsIn, u32 n, u32 shift,
                                                               const u32 *__restrict__ hist, u32 nBlocks, u32 *__restrict__ keysOut,
                                                               u32 *__restrict__ cellsOut) {
    __shared__ u32 cur[WAVES][BINS];                 // counts, then the wave's next slot of every digit
    const u32 t = threadIdx.x, wv = t >> 6, lane = t & 63;
    for (u32 v = 0; v < WAVES; v++) cur[v][t] = 0;
    __syncthreads();
    const u64 first = (u64)blockIdx.x * TILE + (u64)wv * (64 * ROUNDS) + lane;
    for (u32 r = 0; r < ROUNDS; r++) {
        const u64 idx = first + 64 * r;
        if (idx < n) atomicAdd(&cur[wv][(keysIn[idx] >> shift) & (BINS - 1)], 1u);
    }
    __syncthreads();
    u32 g = hist[(u64)t * nBlocks + blockIdx.x];     // lane t = digit t: where this workgroup's cells of that digit start
    for (u32 v = 0; v < WAVES; v++) { const u32 c = cur[v][t]; cur[v][t] = g; g += c; }
    __syncthreads();
    for (u32 r = 0; r < ROUNDS; r++) {               // the same trip count for every lane: the ballots need the whole wave
        const u64 idx = first + 64 * r;
        const bool valid = idx < n;
        const u32 key = valid ? keysIn[idx] : 0, d = (key >> shift) & (BINS - 1);
        unsigned long long peers = __ballot(valid);
#pragma unroll
        for (u32 bit = 0; bit < 8; bit++) {
            const bool b = (d >> bit) & 1;
            const unsigned long long bm = __ballot(b);
            peers &= b ? bm : ~bm;
        }
        const unsigned long long below = peers & ((1ull << lane) - 1);
        const int leader = valid ? __ffsll(peers) - 1 : (int)lane;
        u32 old = 0;
        if (valid && below == 0) old = atomicAdd(&cur[wv][d], (u32)__popcll(peers));
        old = __shfl(old, leader, 64);
        const u32 dest = old + (u32)__popcll(below);
        if (valid && dest < n) { keysOut[dest] = key; cellsOut[dest] = cellsIn[idx]; }
    }
}

__global__ void __launch_bounds__(THREADS) conn_link_kernel(const u32 *__restrict__ keys, const u32 *__restrict__ cells, u32 n, u32 *__restrict__ pred) {
    for (u64 p = (u64)blockIdx.x * THREADS + threadIdx.x; p < n; p += (u64)gridDim.x * THREADS) {
        const u32 k = keys[p], c = cells[p];
        if (c >= n) continue;
        u32 from = c;
        if (k) {
            if (p && keys[p - 1] == k) from = cells[p - 1];
            else {                                   // the first of its run: the run's last cell, by bisection (keys ascend, so a key at or after p is k or larger)
                u64 lo = p + 1, hi = n;
                while (lo < hi) { const u64 mid = (lo + hi) >> 1; if (keys[mid] == k) lo = mid + 1; else hi = mid; }
                from = cells[lo - 1];
            }
        }
        pred[c] = from;
    }
}

// ---- step 2: fill ----
template <class F>
__global__ void __launch_bounds__(THREADS) conn_tables_kernel(Consts<F> c, u32 nCols, u32 loBits, u32 hiBits, typename F::Mem *__restrict__ hi,
                                                              typename F::Mem *__restrict__ lo) {
    const u64 nHi = 1ull << hiBits, total = nHi + ((u64)nCols << loBits);
    const typename F::Elem w = F::reduce(c.w);
    for (u64 k = (u64)blockIdx.x * THREADS + threadIdx.x; k < total; k += (u64)gridDim.x * THREADS) {
        if (k < nHi) { F::store(hi, k, F::pow(w, k << loBits)); continue; }
        const u64 e = k - nHi;
        F::store(lo, e, F::mul(F::pow(w, e & ((1ull << loBits) - 1)), F::reduce(c.ks[e >> loBits])));
    }
}

// the cell whose identity value cell (r, j) takes
__device__ __forceinline__ u32 source_cell(const u32 *__restrict__ pred, u64 r, u64 j, u64 nRows, u32 nCols, u32 n) {
    const u64 c = r * nCols + j;
    if (r >= nRows) return (u32)c;                   // only read below: rows past the table keep id of themselves
    const u32 from = pred[c];
    return from < n ? from : (u32)c;
}

template <class F>
__global__ void __launch_bounds__(THREADS) conn_fill_kernel(const u32 *__restrict__ pred, u64 nRows, u32 nCols, u32 n, u64 N, u32 loBits,
                                                            const typename F::Mem *__restrict__ hi, const typename F::Mem *__restrict__ lo,
                                                            typename F::Mem *__restrict__ dst, u64 dstStride, u64 dstOffset) {
    for (CellWalk c((u64)blockIdx.x * THREADS + threadIdx.x, (u64)gridDim.x * THREADS, nCols); c.r < N; c.next()) {
        u64 pi = c.r, pj = c.j;
        if (c.r < nRows) { const u32 from = source_cell(pred, c.r, c.j, nRows, nCols, n); pi = from / nCols; pj = from - pi * nCols; }
        F::store(dst, c.r * dstStride + dstOffset + c.j, F::mul(F::load(lo, (pj << loBits) + (pi & ((1ull << loBits) - 1))), F::load(hi, pi >> loBits)));
    }
}

// ---- host side ----
// every launch of a call, on st; the arguments have passed the checks.  ks1 and w are read before this returns (they travel as kernel arguments).
int launch(const uint32_t *sMap, u64 nRows, u64 nCols, u64 nW, u64 N, const u64 *w, const u64 *ks1, u64 *dst, u64 dstStride, u64 dstOffset,
           void *scratch, const connplan::Plan &p, u32 words, u64 *hostFirstBad, hipStream_t st) {
    char *s = (char *)scratch;
    unsigned long long *bad = (unsigned long long *)(s + p.offBad);
    u32 *keys[2] = { (u32 *)(s + p.offKeys[0]), (u32 *)(s + p.offKeys[1]) }, *cells[2] = { (u32 *)(s + p.offCells[0]), (u32 *)(s + p.offCells[1]) };
    u32 *hist = (u32 *)(s + p.offHist), *sums = (u32 *)(s + p.offSums);
    const u32 n = (u32)p.cells, histLen = BINS * p.sortBlocks;
    if (hostFirstBad) HIP_TRY(hipMemsetAsync(bad, 0xFF, 8, st));
    const u32 *pred = keys[1];
    if (n) {
        conn_init_kernel<<<blocks(n), THREADS, 0, st>>>(sMap, n, (u32)nW, keys[0], cells[0], hostFirstBad ? bad : nullptr);
        KERNEL_CHECK();
        u32 in = 0;
        for (u32 pass = 0; pass < p.passes; pass++, in ^= 1) {
            const u32 shift = 8 * pass;
            conn_hist_kernel<<<p.sortBlocks, THREADS, 0, st>>>(keys[in], n, shift, hist, p.sortBlocks);
            KERNEL_CHECK();
            conn_scan_sums_kernel<<<p.scanChunks, THREADS, 0, st>>>(hist, histLen, sums);
            KERNEL_CHECK();
            conn_scan_top_kernel<<<1, THREADS, 0, st>>>(sums, p.scanChunks);
            KERNEL_CHECK();
            conn_scan_apply_kernel<<<p.scanChunks, THREADS, 0, st>>>(hist, histLen, sums);
            KERNEL_CHECK();
            conn_scatter_kernel<<<p.sortBlocks, THREADS, 0, st>>>(keys[in], cells[in], n, shift, hist, p.sortBlocks, keys[in ^ 1], cells[in ^ 1]);
            KERNEL_CHECK();
        }
        conn_link_kernel<<<blocks(n), THREADS, 0, st>>>(keys[in], cells[in], n, keys[in ^ 1]);
        KERNEL_CHECK();
        pred = keys[in ^ 1];
    }
    auto fillOf = [&](auto field) -> int {             // tables and fill in one field
        typedef decltype(field) F;
        typedef typename F::Mem Mem;
        Consts<F> c{};
        memcpy(&c.w, w, sizeof c.w);
        memcpy(c.ks, ks1, sizeof c.w * nCols);
        Mem *hi = (Mem *)(s + p.offHi), *lo = (Mem *)(s + p.offLo);
        conn_tables_kernel<F><<<blocks(p.tableElems), THREADS, 0, st>>>(c, (u32)nCols, p.loBits, p.hiBits, hi, lo);
        KERNEL_CHECK();
        conn_fill_kernel<F><<<blocks(N * nCols), THREADS, 0, st>>>(pred, nRows, (u32)nCols, n, N, p.loBits, hi, lo, (Mem *)dst, dstStride, dstOffset);
        KERNEL_CHECK();
        return PIL2GL_OK;
    };
    P2_TRY(words == 1 ? fillOf(GlField{}) : fillOf(FrField{}));
    if (hostFirstBad) {
        HIP_TRY(hipMemcpyAsync(hostFirstBad, bad, 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    return PIL2GL_OK;
}

int conn_dev(const uint32_t *sMap, u64 nRows, u64 nCols, u64 nW, u64 N, const u64 *w, const u64 *ks1, u64 *dst, u64 dstStride, u64 dstOffset,
             void *scratch, u64 scratchBytes, u32 words, u64 *hostFirstBad, void *stream) {
    if (hostFirstBad) *hostFirstBad = NO_BAD;
    if (const char *m = connplan::check(nRows, nCols, nW, N, words)) return fail(PIL2GL_EINVAL, "%s", m);
    if (dstStride >> 32 || dstOffset > dstStride || dstStride - dstOffset < nCols)
        return fail(PIL2GL_EINVAL, "dstStride %llu < dstOffset %llu + nCols %llu (or dstStride >= 2^32)", (unsigned long long)dstStride,
                    (unsigned long long)dstOffset, (unsigned long long)nCols);
    if (!nCols) return PIL2GL_OK;
    const connplan::Plan p = connplan::plan(nRows, nCols, nW, N, words);
    if (!dst || !w || !ks1 || !scratch || (p.cells && !sMap)) return fail(PIL2GL_EINVAL, "null buffer");
    if ((uintptr_t)dst & (words == 4 ? 15 : 7) || (uintptr_t)scratch & 15 || (uintptr_t)sMap & 3)
        return fail(PIL2GL_EINVAL, "dst must be %u-byte aligned, the scratch 16-byte, sMap 4-byte", words == 4 ? 16u : 8u);
    if (scratchBytes < p.bytes) return fail(PIL2GL_EINVAL, "the scratch holds %llu bytes, %llu needed", (unsigned long long)scratchBytes, (unsigned long long)p.bytes);
    const u64 dBytes = ((N - 1) * dstStride + dstOffset + nCols) * 8 * words;
    if (meets(dst, dBytes, sMap, 4 * p.cells) || meets(dst, dBytes, scratch, p.bytes)) return fail(PIL2GL_EINVAL, "dst overlaps sMap or the scratch");
    if (meets(scratch, p.bytes, sMap, 4 * p.cells)) return fail(PIL2GL_EINVAL, "the scratch overlaps sMap");
    P2_TRY(ensure_init());
    return launch(sMap, nRows, nCols, nW, N, w, ks1, dst, dstStride, dstOffset, scratch, p, words, hostFirstBad, as_stream(stream));
}

// layout 0: nRows x nCols u64, row-major (an exec file's section); 1: nCols arrays of N u32 one after the other (the setups' sMap)
int conn_host(const void *hostSMap, int layout, u64 nRows, u64 nCols, u64 nW, u64 N, const u64 *w, const u64 *ks1, u64 *hostDst, u32 words) {
    if (const char *m = connplan::check(nRows, nCols, nW, N, words)) return fail(PIL2GL_EINVAL, "%s", m);
    if (layout != PIL2GL_CONN_SMAP_ROWS_U64 && layout != PIL2GL_CONN_SMAP_COLS_U32) return fail(PIL2GL_EINVAL, "the sMap layout is 0 (rows of u64) or 1 (columns of N u32)");
    if (!nCols) return PIL2GL_OK;
    const connplan::Plan p = connplan::plan(nRows, nCols, nW, N, words);
    if (!hostDst || !w || !ks1 || (p.cells && !hostSMap)) return fail(PIL2GL_EINVAL, "null buffer");
    const u64 mapWords = smapplan::packed_words(p.cells);
    std::vector<u64> packed(mapWords);
    u64 badCell, v;
    if (!smapplan::narrow(hostSMap, layout == PIL2GL_CONN_SMAP_COLS_U32, N, nRows, nCols, nW, packed.data(), &badCell, &v))
        return fail(PIL2GL_EINVAL, "sMap cell %llu (row %llu, column %llu) = %llu names no signal (nW = %llu)", (unsigned long long)badCell,
                    (unsigned long long)(badCell / nCols), (unsigned long long)(badCell % nCols), (unsigned long long)v, (unsigned long long)nW);
    const u64 outWords = N * nCols * words;
    if (meets(hostDst, outWords * 8, hostSMap, layout == PIL2GL_CONN_SMAP_ROWS_U64 ? 8 * p.cells : 4 * N * nCols)) return fail(PIL2GL_EINVAL, "dst overlaps sMap");
    Stage s(mapWords + p.bytes / 8 + outWords);
    P2_TRY(s.rc());
    const u64 *dMap = s.put(packed.data(), mapWords);
    u64 *dScratch = s.take(p.bytes / 8), *dDst = s.take(outWords);
    P2_TRY(s.rc());
    P2_TRY(launch((const uint32_t *)dMap, nRows, nCols, nW, N, w, ks1, dDst, nCols, 0, dScratch, p, words, nullptr, 0));
    return s.get(hostDst, dDst, outWords);
}

}  // namespace

extern "C" {

int pil2gl_conn_plan(uint64_t nRows, uint64_t nCols, uint64_t nW, uint64_t N, uint32_t elemWords, uint32_t *outInfo, uint64_t *scratchBytes) {
    if (scratchBytes) *scratchBytes = 0;
    if (const char *m = connplan::check(nRows, nCols, nW, N, elemWords)) return fail(PIL2GL_EINVAL, "%s", m);
    const connplan::Plan p = connplan::plan(nRows, nCols, nW, N, elemWords);
    if (outInfo) {
        outInfo[0] = p.passes; outInfo[1] = THREADS; outInfo[2] = TILE; outInfo[3] = p.sortBlocks; outInfo[4] = p.scanChunks;
        outInfo[5] = p.loBits; outInfo[6] = p.hiBits; outInfo[7] = p.launches;
    }
    if (scratchBytes) *scratchBytes = p.bytes;
    return PIL2GL_OK;
}

int pil2gl_conn_pols_dev(const uint32_t *sMap32, uint64_t nRows, uint64_t nCols, uint64_t nW, uint64_t N, const uint64_t *hostW, const uint64_t *hostKs1,
                         uint64_t *dst, uint64_t dstStride, uint64_t dstOffset, uint64_t *scratch, uint64_t scratchBytes, uint64_t *hostFirstBad,
                         void *stream) {
    return conn_dev(sMap32, nRows, nCols, nW, N, hostW, hostKs1, dst, dstStride, dstOffset, scratch, scratchBytes, 1, hostFirstBad, stream);
}
int pil2gl_bn128_conn_pols_dev(const uint32_t *sMap32, uint64_t nRows, uint64_t nCols, uint64_t nW, uint64_t N, const uint64_t *hostW,
                               const uint64_t *hostKs1, uint64_t *dst, uint64_t dstStride, uint64_t dstOffset, uint64_t *scratch, uint64_t scratchBytes,
                               uint64_t *hostFirstBad, void *stream) {
    return conn_dev(sMap32, nRows, nCols, nW, N, hostW, hostKs1, dst, dstStride, dstOffset, scratch, scratchBytes, 4, hostFirstBad, stream);
}
int pil2gl_conn_pols(const void *hostSMap, int sMapLayout, uint64_t nRows, uint64_t nCols, uint64_t nW, uint64_t N, const uint64_t *hostW,
                     const uint64_t *hostKs1, uint64_t *hostDst) {
    return conn_host(hostSMap, sMapLayout, nRows, nCols, nW, N, hostW, hostKs1, hostDst, 1);
}
int pil2gl_bn128_conn_pols(const void *hostSMap, int sMapLayout, uint64_t nRows, uint64_t nCols, uint64_t nW, uint64_t N, const uint64_t *hostW,
                           const uint64_t *hostKs1, uint64_t *hostDst) {
    return conn_host(hostSMap, sMapLayout, nRows, nCols, nW, N, hostW, hostKs1, hostDst, 4);
}

}  // extern "C"
