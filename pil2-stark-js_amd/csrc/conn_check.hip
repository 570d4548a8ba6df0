// The connection check on the device, gfx950: does a trace meet `{a[0 .. nCols)} connect {S[0 .. nCols)}`, the one identity beyond
// polynomials that compressor12/18.pil.ejs, final6/9.pil.ejs and finalfflonk.pil.ejs state and that the reference checks with pilcom's
// verifyPil (src/compressor/main_compressor_pil_verify.js:36).  With id(i, j) = w^i ks'[j] (ks'[0] = 1) and cells in flat order c = i nCols + j:
// every S[c] must be id(c') of exactly one cell c', and a[c] must equal a[c'], both as field values.
//   tables   hi[t] = w^(t 2^loBits), lo[j][t] = w^t ks'[j]: conn_pols.hip's two-level tables, a lane per entry, so that id(c) is ONE product
//            for any cell (about sqrt N entries a column, no N-element table, no serial chain, no discrete logarithm).
//   build    a lane per cell puts it into the index table (index_table.cuh) under the key id(c), re-derived from a cell by one product.  A
//            cell that meets another of its identity lowers the duplicate cell to the larger of the two: by the table's argument the
//            minimum over all cells is the first cell, in flat order, whose identity an earlier cell already has.
//   check    Goldilocks a lane a cell, Fr two neighbouring lanes a cell, each moving one 16-byte half (wtns_exec.hip's gather): reduce S[c],
//            probe, compare a[c] with a[c'] after reducing both; the smallest failing cell by the wave-minimum rule, one atomic a wave.
//   finish   one workgroup, one lane: partner and kind are recomputed for the winning cell alone, so the three words describe one cell.
// Goldilocks: words in [p, 2^64) count as their value mod p.  Fr: Montgomery words, any 256-bit pattern counting as its value mod r.
//
// Safety: nothing read from S or a is used as an address; a slot's content addresses the tables or a only below the cell count (the hash
// table's `limit`).  Shared: the hash table (index_table.cuh); the bad-cell report, the cell walk and the fields as template parameters
// (smap_cells.cuh); grid and overlap test (smap_plan.h); the table shapes (conn_plan.h).
#include "common.h"
#include "index_table.cuh"
#include "conn_check_plan.h"
#include <string.h>

using namespace pil2gl;

namespace {

using namespace indextable;
using namespace smapplan;
using namespace conncheckplan;

uint64_t g_lastProbe = 0;                            // the longest displacement of the last build (pil2gl_debug_conn_check_probe)

template <class F> struct Consts { typename F::Elem w, ks[connplan::MAX_COLS]; };       // w and ks' as the caller gave them, a kernel argument

template <class F> struct Table {
    u32 *slots; u64 mask;                            // capacity slots, mask = capacity - 1
    u32 cells, nCols, loBits;
    const typename F::Mem *hi, *lo;
};

// id of a cell below t.cells: one product of two table entries
template <class F> __device__ __forceinline__ typename F::Elem id_of(const Table<F> &t, u32 cell) {
    const u32 i = cell / t.nCols, j = cell - i * t.nCols;
    return F::mul(F::load(t.lo, ((u64)j << t.loBits) + (i & ((1u << t.loBits) - 1))), F::load(t.hi, i >> t.loBits));
}

// the cell whose identity is the canonical `key`, EMPTY when there is none; after the build
template <class F> __device__ __forceinline__ u32 lookup(const Table<F> &t, const typename F::Elem &key) {
    return find<1>(t.slots, t.mask, hash_of(key), t.cells, [&](u32 cur) { return same(key, id_of(t, cur)); }).met;
}

// ---- tables: conn_pols.hip's, lo[j][t] = w^t ks'[j] and hi[t] = w^(t 2^loBits) ----
template <class F>
__global__ void __launch_bounds__(THREADS) cc_tables_kernel(Consts<F> c, u32 nCols, u32 loBits, u32 hiBits, typename F::Mem *__restrict__ hi,
                                                            typename F::Mem *__restrict__ lo) {
    const u64 nHi = 1ull << hiBits, total = nHi + ((u64)nCols << loBits);
    const typename F::Elem w = F::reduce(c.w);
    for (u64 k = (u64)blockIdx.x * THREADS + threadIdx.x; k < total; k += (u64)gridDim.x * THREADS) {
        if (k < nHi) { F::store(hi, k, F::pow(w, k << loBits)); continue; }
        const u64 e = k - nHi;
        F::store(lo, e, F::mul(F::pow(w, e & ((1ull << loBits) - 1)), F::reduce(c.ks[e >> loBits])));
    }
}

// ---- build ----
template <class F>
__global__ void __launch_bounds__(THREADS) cc_build_kernel(Table<F> t, unsigned long long *hdr) {
    u64 dup = NO_BAD;
    u32 longest = 0;
    for (u64 c = (u64)blockIdx.x * THREADS + threadIdx.x; c < t.cells; c += (u64)gridDim.x * THREADS) {
        const typename F::Elem key = id_of(t, (u32)c);
        const Hit h = insert<1>(t.slots, t.mask, hash_of(key), (u32)c, t.cells, [&](u32 cur) { return same(key, id_of(t, cur)); });
        longest = h.displaced > longest ? h.displaced : longest;
        if (h.met != EMPTY) {                                                // another cell of this identity: the larger of the two
            const u64 larger = h.met > c ? h.met : c;
            dup = larger < dup ? larger : dup;
        }
    }
    report_bad(dup, hdr + H_DUP);
    report_probe(longest, hdr + H_PROBE);
}

// ---- check ----
// Two kernels, as wtns_exec.hip's gathers: the Fr one moves a cell as two lanes' halves, the Goldilocks one a lane a cell.
__global__ void __launch_bounds__(THREADS) cc_check_gl_kernel(Table<GlField> t, u64 N, const u64 *__restrict__ a, u64 aStride, u64 aOffset,
                                                              const u64 *__restrict__ S, u64 sStride, u64 sOffset, unsigned long long *hdr) {
    u64 best = NO_BAD;
    for (CellWalk c((u64)blockIdx.x * THREADS + threadIdx.x, (u64)gridDim.x * THREADS, t.nCols); c.r < N; c.next()) {
        const u32 p = lookup(t, gl::canon(S[c.r * sStride + sOffset + c.j]));
        bool ok = false;
        if (p < t.cells) {
            const u64 pi = p / t.nCols, pj = p - pi * t.nCols;
            ok = gl::canon(a[c.r * aStride + aOffset + c.j]) == gl::canon(a[pi * aStride + aOffset + pj]);
        }
        const u64 flat = c.r * t.nCols + c.j;
        if (!ok) best = flat < best ? flat : best;
    }
    report_bad(best, hdr + H_FAIL);
}

__device__ __forceinline__ uint4 other_half(const uint4 &mine) {
    uint4 o;
    o.x = __shfl_xor(mine.x, 1, 64); o.y = __shfl_xor(mine.y, 1, 64); o.z = __shfl_xor(mine.z, 1, 64); o.w = __shfl_xor(mine.w, 1, 64);
    return o;
}
// the element whose half h this lane holds and whose other half its neighbour holds, canonical
__device__ __forceinline__ FrField::Elem pair_elem(const uint4 &mine, u32 h) {
    const uint4 other = other_half(mine);
    FrField::Elem x;
    bn::unpack(h ? other : mine, h ? mine : other, x.v);
    bn::reduce256(x.v);
    return x;
}

// lanes 2 c and 2 c + 1 of the launch hold cell c: lane parity = the half it loads; both lanes of a cell probe and judge alike
__global__ void __launch_bounds__(THREADS) cc_check_fr_kernel(Table<FrField> t, u64 N, const uint4 *__restrict__ a, u64 aStride, u64 aOffset,
                                                              const uint4 *__restrict__ S, u64 sStride, u64 sOffset, unsigned long long *hdr) {
    const u32 h = threadIdx.x & 1;
    u64 best = NO_BAD;
    for (CellWalk c(((u64)blockIdx.x * THREADS + threadIdx.x) >> 1, (u64)gridDim.x * (THREADS / 2), t.nCols); c.r < N; c.next()) {
        const u32 p = lookup(t, pair_elem(S[2 * (c.r * sStride + sOffset + c.j) + h], h));
        const bool found = p < t.cells;              // the same for both lanes of a cell
        uint4 mine = make_uint4(0, 0, 0, 0), theirs = make_uint4(0, 0, 0, 0);
        if (found) {
            const u64 pi = p / t.nCols, pj = p - pi * t.nCols;
            mine = a[2 * (c.r * aStride + aOffset + c.j) + h];
            theirs = a[2 * (pi * aStride + aOffset + pj) + h];
        }
        const FrField::Elem x = pair_elem(mine, h), y = pair_elem(theirs, h);
        const u64 flat = c.r * t.nCols + c.j;
        if (!found || !same(x, y)) best = flat < best ? flat : best;
    }
    report_bad(best, hdr + H_FAIL);
}

// ---- finish: the report's three words from the two minima ----
template <class F>
__global__ void __launch_bounds__(64) cc_finish_kernel(Table<F> t, const typename F::Mem *__restrict__ S, u64 sStride, u64 sOffset,
                                                       unsigned long long *hdr) {
    if (threadIdx.x) return;
    const u64 dup = hdr[H_DUP], bad = hdr[H_FAIL];
    u64 cell = NO_BAD, partner = NO_BAD, kind = CLEAN;
    if (dup < t.cells) {
        cell = dup; kind = IDS_NOT_DISTINCT;
        const u32 p = lookup(t, id_of(t, (u32)dup));                         // the slot kept the group's smallest cell
        if (p < t.cells) partner = p;
    } else if (bad < t.cells) {
        cell = bad;
        const u64 i = bad / t.nCols, j = bad - i * t.nCols;
        const u32 p = lookup(t, F::reduce(F::load(S, i * sStride + sOffset + j)));
        if (p < t.cells) { partner = p; kind = VALUES_DIFFER; } else kind = NAMES_NO_CELL;
    }
    hdr[H_CELL] = cell; hdr[H_PARTNER] = partner; hdr[H_KIND] = kind;
}

// ---- host side ----
void clean(u64 *report) { if (report) { report[0] = report[1] = NO_BAD; report[2] = CLEAN; } }

// every launch of a call, on st; the arguments have passed the checks.  Blocks for the report.
template <class F>
int launch_field(const u64 *a, u64 aStride, u64 aOffset, const u64 *S, u64 sStride, u64 sOffset, u64 N, u64 nCols, const u64 *w, const u64 *ks1,
                 void *scratch, const Plan &p, u64 *hostReport, hipStream_t st) {
    typedef typename F::Mem Mem;
    char *s = (char *)scratch;
    unsigned long long *hdr = (unsigned long long *)(s + p.offHeader);
    Mem *hi = (Mem *)(s + p.offHi), *lo = (Mem *)(s + p.offLo);
    Consts<F> c{};
    memcpy(&c.w, w, sizeof c.w);
    memcpy(c.ks, ks1, sizeof c.w * nCols);
    const Table<F> t{ (u32 *)(s + p.offTable), p.capacity - 1, (u32)p.cells, (u32)nCols, p.loBits, hi, lo };
    static_assert(HEADER_BYTES % 16 == 0, "the table follows the header");
    HIP_TRY(hipMemsetAsync(s + p.offHeader, 0xFF, HEADER_BYTES + 4 * p.capacity, st));      // header and table are neighbours: all ones, EMPTY
    HIP_TRY(hipMemsetAsync(hdr + H_PROBE, 0, 8, st));
    cc_tables_kernel<F><<<blocks(p.tableElems), THREADS, 0, st>>>(c, (u32)nCols, p.loBits, p.hiBits, hi, lo);
    KERNEL_CHECK();
    cc_build_kernel<F><<<p.buildBlocks, THREADS, 0, st>>>(t, hdr);
    KERNEL_CHECK();
    if constexpr (sizeof(Mem) == 8)
        cc_check_gl_kernel<<<p.checkBlocks, THREADS, 0, st>>>(t, N, a, aStride, aOffset, S, sStride, sOffset, hdr);
    else
        cc_check_fr_kernel<<<p.checkBlocks, THREADS, 0, st>>>(t, N, (const uint4 *)a, aStride, aOffset, (const uint4 *)S, sStride, sOffset, hdr);
    KERNEL_CHECK();
    cc_finish_kernel<F><<<1, 64, 0, st>>>(t, (const Mem *)S, sStride, sOffset, hdr);
    KERNEL_CHECK();
    u64 out[4];                                      // the report and the longest probe
    HIP_TRY(hipMemcpyAsync(out, hdr, sizeof out, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    memcpy(hostReport, out, 24);
    g_lastProbe = out[H_PROBE];
    return PIL2GL_OK;
}

int launch(const u64 *a, u64 aStride, u64 aOffset, const u64 *S, u64 sStride, u64 sOffset, u64 N, u64 nCols, const u64 *w, const u64 *ks1,
           void *scratch, const Plan &p, u32 words, u64 *hostReport, hipStream_t st) {
    return words == 1 ? launch_field<GlField>(a, aStride, aOffset, S, sStride, sOffset, N, nCols, w, ks1, scratch, p, hostReport, st)
                      : launch_field<FrField>(a, aStride, aOffset, S, sStride, sOffset, N, nCols, w, ks1, scratch, p, hostReport, st);
}

int check_dev(const u64 *a, u64 aStride, u64 aOffset, const u64 *S, u64 sStride, u64 sOffset, u64 N, u64 nCols, const u64 *w, const u64 *ks1,
              void *scratch, u64 scratchBytes, u32 words, u64 *hostReport, void *stream) {
    clean(hostReport);
    if (const char *m = conncheckplan::check(N, nCols, words)) return fail(PIL2GL_EINVAL, "%s", m);
    if (!hostReport) return fail(PIL2GL_EINVAL, "null hostReport");
    if (const char *m = check_columns(aStride, aOffset, nCols)) return fail(PIL2GL_EINVAL, "a: %s", m);
    if (const char *m = check_columns(sStride, sOffset, nCols)) return fail(PIL2GL_EINVAL, "S: %s", m);
    if (!nCols) return PIL2GL_OK;
    const Plan p = conncheckplan::plan(N, nCols, words);
    if (!a || !S || !w || !ks1 || !scratch) return fail(PIL2GL_EINVAL, "null buffer");
    if (((uintptr_t)a | (uintptr_t)S) & (words == 4 ? 15 : 7) || (uintptr_t)scratch & 15)
        return fail(PIL2GL_EINVAL, "a and S must be %u-byte aligned, the scratch 16-byte", words == 4 ? 16u : 8u);
    if (scratchBytes < p.bytes) return fail(PIL2GL_EINVAL, "the scratch holds %llu bytes, %llu needed", (unsigned long long)scratchBytes, (unsigned long long)p.bytes);
    if (meets(scratch, p.bytes, a, span_bytes(N, nCols, aStride, aOffset, words)) || meets(scratch, p.bytes, S, span_bytes(N, nCols, sStride, sOffset, words)))
        return fail(PIL2GL_EINVAL, "the scratch overlaps a or S");
    P2_TRY(ensure_init());
    return launch(a, aStride, aOffset, S, sStride, sOffset, N, nCols, w, ks1, scratch, p, words, hostReport, as_stream(stream));
}

// hostA, hostS: N x nCols elements each, row-major
int check_host(const u64 *hostA, const u64 *hostS, u64 N, u64 nCols, const u64 *w, const u64 *ks1, u32 words, u64 *hostReport) {
    clean(hostReport);
    if (const char *m = conncheckplan::check(N, nCols, words)) return fail(PIL2GL_EINVAL, "%s", m);
    if (!hostReport) return fail(PIL2GL_EINVAL, "null hostReport");
    if (!nCols) return PIL2GL_OK;
    if (!hostA || !hostS || !w || !ks1) return fail(PIL2GL_EINVAL, "null buffer");
    const Plan p = conncheckplan::plan(N, nCols, words);
    const u64 n = p.cells * words, part = pad16(n);                          // staged parts start on 16 bytes
    Stage s(p.bytes / 8 + 2 * part);
    P2_TRY(s.rc());
    u64 *dScratch = s.take(p.bytes / 8);
    const u64 *dA = s.put(hostA, n);
    s.take(part - n);
    const u64 *dS = s.put(hostS, n);
    s.take(part - n);
    P2_TRY(s.rc());
    return launch(dA, nCols, 0, dS, nCols, 0, N, nCols, w, ks1, dScratch, p, words, hostReport, 0);
}

}  // namespace

extern "C" {

int pil2gl_conn_check_plan(uint64_t N, uint64_t nCols, uint32_t elemWords, uint32_t *outInfo, uint64_t *scratchBytes) {
    if (scratchBytes) *scratchBytes = 0;
    if (const char *m = conncheckplan::check(N, nCols, elemWords)) return fail(PIL2GL_EINVAL, "%s", m);
    const Plan p = conncheckplan::plan(N, nCols, elemWords);
    if (outInfo) {
        outInfo[0] = p.capBits; outInfo[1] = THREADS; outInfo[2] = p.loBits; outInfo[3] = p.hiBits; outInfo[4] = p.buildBlocks;
        outInfo[5] = p.checkBlocks; outInfo[6] = p.lanesPerCell; outInfo[7] = LAUNCHES;
    }
    if (scratchBytes) *scratchBytes = p.bytes;
    return PIL2GL_OK;
}

int pil2gl_conn_check_dev(const uint64_t *a, uint64_t aStride, uint64_t aOffset, const uint64_t *S, uint64_t sStride, uint64_t sOffset, uint64_t N,
                          uint64_t nCols, const uint64_t *hostW, const uint64_t *hostKs1, uint64_t *scratch, uint64_t scratchBytes,
                          uint64_t *hostReport, void *stream) {
    return check_dev(a, aStride, aOffset, S, sStride, sOffset, N, nCols, hostW, hostKs1, scratch, scratchBytes, 1, hostReport, stream);
}
int pil2gl_bn128_conn_check_dev(const uint64_t *a, uint64_t aStride, uint64_t aOffset, const uint64_t *S, uint64_t sStride, uint64_t sOffset, uint64_t N,
                                uint64_t nCols, const uint64_t *hostW, const uint64_t *hostKs1, uint64_t *scratch, uint64_t scratchBytes,
                                uint64_t *hostReport, void *stream) {
    return check_dev(a, aStride, aOffset, S, sStride, sOffset, N, nCols, hostW, hostKs1, scratch, scratchBytes, 4, hostReport, stream);
}
int pil2gl_conn_check(const uint64_t *hostA, const uint64_t *hostS, uint64_t N, uint64_t nCols, const uint64_t *hostW, const uint64_t *hostKs1,
                      uint64_t *hostReport) {
    return check_host(hostA, hostS, N, nCols, hostW, hostKs1, 1, hostReport);
}
int pil2gl_bn128_conn_check(const uint64_t *hostA, const uint64_t *hostS, uint64_t N, uint64_t nCols, const uint64_t *hostW, const uint64_t *hostKs1,
                            uint64_t *hostReport) {
    return check_host(hostA, hostS, N, nCols, hostW, hostKs1, 4, hostReport);
}

uint64_t pil2gl_debug_conn_check_probe(void) { return g_lastProbe; }

}  // extern "C"
