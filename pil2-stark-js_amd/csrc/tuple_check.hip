// The lookup and permutation checks on the device, gfx950: does a trace meet `selF {f0..fk-1} in selT {t0..tk-1}` (mode 0, plookup) or
// `selF {f0..fk-1} is selT {t0..tk-1}` (mode 1, permutation), as statements about the trace: no challenge, no field arithmetic beyond
// making an element canonical.  The statement is include/pil2gl.h's; tests/tuple_check_ref.py restates it as one dictionary.
//   the table  open addressing, linear probing, ONE table over both sides' selected rows.  A slot holds a 32-bit row index (t row i as i, f
//            row i as n + i, EMPTY = 2^32 - 1), never the key: the key is re-read from the matrix the index names and reduced, so no claimed
//            slot has a half-written key and a slot costs the same over Fr as over Goldilocks.  Beside each slot: the counter (cntT low half,
//            cntF high half) and the smallest selected f row of the tuple.
//   build    a lane per row of either side: hash the k canonical elements, find or claim the tuple's slot -- atomicCAS claims an EMPTY slot,
//            an equal tuple lowers the slot's content by atomicMin (a slot never moves and its content only falls, so after the build it is
//            the tuple's smallest t row when t has it, else n + its smallest f row) -- then one atomicAdd to the counter and, for an f row
//            above the slot's smallest f row so far, nothing, else one atomicMin.
//   judge    every selected row finds its slot again, reads the counter and applies the mode's criterion; the smallest failing row of each
//            side by the wave-minimum rule, one atomic a wave that saw one (smap_cells.cuh report_bad).
//   finish   one workgroup, one lane: f before t, then kind, partner and both counts re-read for the winning tuple alone, so the five words
//            describe one tuple.  Counts, minima and slot contents are sums and minima: none depends on the order in which atomics land.
// One kernel template each over smap_cells.cuh's GlField / FrField, a lane per row in both: a row's k elements are not neighbours in
// memory (cols is any list), so wtns_exec.hip's lane pair per element has no contiguous 32 bytes to split; FrField::load moves an element
// as two 16-byte halves.
//
// Safety: nothing read from f, t or a selector is used as an address.  A slot's content is checked against 2 n before it indexes a matrix;
// every probe loop runs at most `capacity` times whatever the data.  Plain vector loads and stores and global atomics only.
#include "common.h"
#include "smap_cells.cuh"
#include "tuple_check_plan.h"
#include <string.h>

using namespace pil2gl;

namespace {

using namespace smapcells;
using namespace smapplan;
using namespace tuplecheckplan;

constexpr u32 EMPTY = 0xFFFFFFFFu;
uint64_t g_lastProbe = 0;                            // the longest displacement of the last build (pil2gl_debug_tuple_check_probe)

// one side as the caller gave it: the matrix, and the selector column of a matrix of its own (sel null: every row is selected)
template <class F> struct Side { const typename F::Mem *base, *sel; u64 stride, selStride, selCol; };

template <class F> struct Job {
    Side<F> t, f;
    u32 tCols[MAX_K], fCols[MAX_K];
    u32 n, k, mode;
    u32 *slots, *minF;
    unsigned long long *counts;
    u64 mask;                                        // capacity - 1
};

// ---- what the two fields do not share: zero and equality of canonical elements, their limbs for the hash ----
__device__ __forceinline__ bool is_zero(u64 a) { return a == 0; }
__device__ __forceinline__ bool is_zero(const FrField::Elem &a) { return bn::is_zero(a.v); }
__device__ __forceinline__ bool same(u64 a, u64 b) { return a == b; }
__device__ __forceinline__ bool same(const FrField::Elem &a, const FrField::Elem &b) {
    return ((a.v[0] ^ b.v[0]) | (a.v[1] ^ b.v[1]) | (a.v[2] ^ b.v[2]) | (a.v[3] ^ b.v[3]) |
            (a.v[4] ^ b.v[4]) | (a.v[5] ^ b.v[5]) | (a.v[6] ^ b.v[6]) | (a.v[7] ^ b.v[7])) == 0;
}
__device__ __forceinline__ void absorb(TupleHash &x, u64 e) { x.absorb((u32)e); x.absorb((u32)(e >> 32)); }
__device__ __forceinline__ void absorb(TupleHash &x, const FrField::Elem &e) {
#pragma unroll
    for (int i = 0; i < 8; i++) x.absorb(e.v[i]);
}

// rows are numbered as the slots hold them: idx < n is row idx of t, n <= idx < 2 n row idx - n of f
template <class F> __device__ __forceinline__ bool selected(const Job<F> &J, u32 idx) {
    const bool isF = idx >= J.n;
    const typename F::Mem *sel = isF ? J.f.sel : J.t.sel;
    if (!sel) return true;
    const u64 i = isF ? idx - J.n : idx;
    return !is_zero(F::reduce(F::load(sel, i * (isF ? J.f.selStride : J.t.selStride) + (isF ? J.f.selCol : J.t.selCol))));
}
// element j of the tuple of row idx < 2 n, canonical
template <class F> __device__ __forceinline__ typename F::Elem elem_of(const Job<F> &J, u32 idx, u32 j) {
    const bool isF = idx >= J.n;
    const u64 i = isF ? idx - J.n : idx;
    return F::reduce(F::load(isF ? J.f.base : J.t.base, i * (isF ? J.f.stride : J.t.stride) + (isF ? J.fCols[j] : J.tCols[j])));
}
template <class F> __device__ __forceinline__ bool same_tuple(const Job<F> &J, u32 a, u32 b) {
    for (u32 j = 0; j < J.k; j++)
        if (!same(elem_of(J, a, j), elem_of(J, b, j))) return false;
    return true;
}
template <class F> __device__ __forceinline__ u64 home_of(const Job<F> &J, u32 idx) {
    TupleHash x;
    for (u32 j = 0; j < J.k; j++) absorb(x, elem_of(J, idx, j));
    return x.finish() & J.mask;
}

// the slot that holds the tuple of row idx, NONE when no slot does; after the build
template <class F> __device__ __forceinline__ u64 find(const Job<F> &J, u32 idx) {
    u64 s = home_of(J, idx);
    for (u64 probe = 0; probe <= J.mask; probe++, s = (s + 1) & J.mask) {
        const u32 cur = J.slots[s];
        if (cur >= 2 * J.n) return NONE;             // an empty slot ends the run
        if (cur == idx || same_tuple(J, idx, cur)) return s;
    }
    return NONE;
}

// ---- build ----
template <class F>
__global__ void __launch_bounds__(THREADS) tc_build_kernel(Job<F> J, unsigned long long *hdr) {
    const u64 rows = 2ull * J.n;
    u32 longest = 0;
    for (u64 r = (u64)blockIdx.x * THREADS + threadIdx.x; r < rows; r += (u64)gridDim.x * THREADS) {
        const u32 idx = (u32)r;
        if (!selected(J, idx)) continue;
        u64 s = home_of(J, idx);
        bool placed = false;
        for (u64 probe = 0; probe <= J.mask; probe++, s = (s + 1) & J.mask) {
            u32 cur = J.slots[s];
            if (cur == EMPTY) {
                cur = atomicCAS(&J.slots[s], EMPTY, idx);
                if (cur == EMPTY) {                                              // claimed, `probe` slots past its home
                    longest = (u32)probe > longest ? (u32)probe : longest;
                    placed = true;
                    break;
                }
            }
            if (cur < rows && same_tuple(J, idx, cur)) {                         // the same tuple: the slot keeps the smaller row
                if (idx < cur) atomicMin(&J.slots[s], idx);
                placed = true;
                break;
            }
        }
        if (!placed) continue;                                                   // the load factor is at most 1 / 2: not reached
        const bool isF = idx >= J.n;
        atomicAdd(&J.counts[s], isF ? 1ull << 32 : 1ull);
        if (isF && J.minF[s] > idx - J.n) atomicMin(&J.minF[s], idx - J.n);      // what was read only falls: skipping is safe
    }
    for (int o = 32; o > 0; o >>= 1) { const u32 other = __shfl_xor(longest, o, 64); longest = other > longest ? other : longest; }
    if ((threadIdx.x & 63) == 0 && longest) atomicMax(hdr + H_PROBE, (unsigned long long)longest);
}

// ---- judge ----
template <class F>
__global__ void __launch_bounds__(THREADS) tc_judge_kernel(Job<F> J, unsigned long long *hdr) {
    const u64 rows = 2ull * J.n;
    u64 badF = NO_BAD, badT = NO_BAD;
    // a lookup judges f alone
    for (u64 r = (J.mode == MODE_LOOKUP ? J.n : 0) + (u64)blockIdx.x * THREADS + threadIdx.x; r < rows; r += (u64)gridDim.x * THREADS) {
        const u32 idx = (u32)r;
        if (!selected(J, idx)) continue;
        const u64 s = find(J, idx);
        const u64 c = s == NONE ? 0 : J.counts[s];
        const u32 cntT = (u32)c, cntF = (u32)(c >> 32);
        if (idx >= J.n) {
            const u64 i = idx - J.n;
            if (J.mode == MODE_LOOKUP ? cntT == 0 : cntF > cntT) badF = i < badF ? i : badF;
        } else if (cntT > cntF) badT = idx < badT ? idx : badT;
    }
    report_bad(badF, hdr + H_FAIL_F);
    report_bad(badT, hdr + H_FAIL_T);
}

// ---- finish: the report's five words from the two minima ----
template <class F>
__global__ void __launch_bounds__(64) tc_finish_kernel(Job<F> J, unsigned long long *hdr) {
    if (threadIdx.x) return;
    const u64 bf = hdr[H_FAIL_F], bt = hdr[H_FAIL_T];
    u64 kind = CLEAN, row = NONE, partner = NONE, cntF = 0, cntT = 0;
    const bool onF = bf < J.n;                                                   // a failing row of f goes before any of t
    if (onF || bt < J.n) {
        row = onF ? bf : bt;
        const u64 s = find(J, (u32)(onF ? J.n + bf : bt));
        if (s != NONE) {
            const u64 c = J.counts[s];
            cntT = (u32)c; cntF = c >> 32;
            const u32 p = onF ? J.slots[s] : J.minF[s];                          // the tuple's smallest row on the other side, if any
            if (p < J.n) partner = p;
        }
        kind = !onF ? T_MORE_THAN_F : cntT ? F_MORE_THAN_T : F_NOT_IN_T;
    }
    hdr[H_KIND] = kind; hdr[H_ROW] = row; hdr[H_PARTNER] = partner; hdr[H_CNT_F] = cntF; hdr[H_CNT_T] = cntT;
}

// ---- host side ----
void clean(u64 *report) { if (report) { report[0] = CLEAN; report[1] = report[2] = NONE; report[3] = report[4] = 0; } }

// one side as the entries take it
struct HostSide { const u64 *base; u64 stride; const u64 *cols; const u64 *sel; u64 selStride, selCol; };

// every launch of a call, on st; the arguments have passed the checks.  Blocks for the report.
template <class F>
int launch_field(const HostSide &f, const HostSide &t, u64 n, u32 k, u32 mode, void *scratch, const Plan &p, u64 *hostReport, hipStream_t st) {
    typedef typename F::Mem Mem;
    char *s = (char *)scratch;
    unsigned long long *hdr = (unsigned long long *)(s + p.offHeader);
    Job<F> J{};
    J.t = Side<F>{ (const Mem *)t.base, (const Mem *)t.sel, t.stride, t.selStride, t.selCol };
    J.f = Side<F>{ (const Mem *)f.base, (const Mem *)f.sel, f.stride, f.selStride, f.selCol };
    for (u32 j = 0; j < k; j++) { J.tCols[j] = (u32)t.cols[j]; J.fCols[j] = (u32)f.cols[j]; }
    J.n = (u32)n; J.k = k; J.mode = mode;
    J.slots = (u32 *)(s + p.offSlots); J.minF = (u32 *)(s + p.offMinF);
    J.counts = (unsigned long long *)(s + p.offCounts);
    J.mask = p.capacity - 1;
    static_assert(HEADER_BYTES % 16 == 0, "the slots follow the header");
    HIP_TRY(hipMemsetAsync(s + p.offHeader, 0xFF, HEADER_BYTES + 8 * p.capacity, st));      // header, slots and minF are neighbours: all ones, EMPTY
    HIP_TRY(hipMemsetAsync(s + p.offCounts, 0, 8 * p.capacity, st));
    HIP_TRY(hipMemsetAsync(hdr + H_PROBE, 0, 8, st));
    tc_build_kernel<F><<<p.blocks, THREADS, 0, st>>>(J, hdr);
    KERNEL_CHECK();
    tc_judge_kernel<F><<<p.blocks, THREADS, 0, st>>>(J, hdr);
    KERNEL_CHECK();
    tc_finish_kernel<F><<<1, 64, 0, st>>>(J, hdr);
    KERNEL_CHECK();
    u64 out[REPORT_WORDS + 1];                       // the report and the longest probe
    HIP_TRY(hipMemcpyAsync(out, hdr, sizeof out, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    memcpy(hostReport, out, 8 * REPORT_WORDS);
    g_lastProbe = out[H_PROBE];
    return PIL2GL_OK;
}

int launch(const HostSide &f, const HostSide &t, u64 n, u32 k, u32 mode, void *scratch, const Plan &p, u32 words, u64 *hostReport, hipStream_t st) {
    return words == 1 ? launch_field<GlField>(f, t, n, k, mode, scratch, p, hostReport, st)
                      : launch_field<FrField>(f, t, n, k, mode, scratch, p, hostReport, st);
}

// what both forms refuse about the shape: 0, or the code after fail()
int check_shape(const HostSide &f, const HostSide &t, u64 n, u64 k, u32 mode, u32 words, u64 *hostReport) {
    if (const char *m = tuplecheckplan::check(n, k, words, mode)) return fail(PIL2GL_EINVAL, "%s", m);
    if (!hostReport) return fail(PIL2GL_EINVAL, "null hostReport");
    if (const char *m = check_columns(n, f.stride, f.cols, k)) return fail(PIL2GL_EINVAL, "f: %s", m);
    if (const char *m = check_columns(n, t.stride, t.cols, k)) return fail(PIL2GL_EINVAL, "t: %s", m);
    if (f.sel) if (const char *m = check_columns(n, f.selStride, &f.selCol, 1)) return fail(PIL2GL_EINVAL, "selF: %s", m);
    if (t.sel) if (const char *m = check_columns(n, t.selStride, &t.selCol, 1)) return fail(PIL2GL_EINVAL, "selT: %s", m);
    return PIL2GL_OK;
}

int check_dev(const HostSide &f, const HostSide &t, u64 n, u64 k, u32 mode, void *scratch, u64 scratchBytes, u32 words, u64 *hostReport, void *stream) {
    clean(hostReport);
    P2_TRY(check_shape(f, t, n, k, mode, words, hostReport));
    if (!n) return PIL2GL_OK;
    const Plan p = tuplecheckplan::plan(n);
    if (!f.base || !t.base || !scratch) return fail(PIL2GL_EINVAL, "null buffer");
    if (((uintptr_t)f.base | (uintptr_t)t.base | (uintptr_t)f.sel | (uintptr_t)t.sel | (uintptr_t)scratch) & 15)
        return fail(PIL2GL_EINVAL, "f, t, the selectors and the scratch must be 16-byte aligned");
    if (scratchBytes < p.bytes) return fail(PIL2GL_EINVAL, "the scratch holds %llu bytes, %llu needed", (unsigned long long)scratchBytes, (unsigned long long)p.bytes);
    if (meets(scratch, p.bytes, f.base, span_bytes(n, f.stride, top_column(f.cols, k), words)) ||
        meets(scratch, p.bytes, t.base, span_bytes(n, t.stride, top_column(t.cols, k), words)) ||
        (f.sel && meets(scratch, p.bytes, f.sel, span_bytes(n, f.selStride, f.selCol, words))) ||
        (t.sel && meets(scratch, p.bytes, t.sel, span_bytes(n, t.selStride, t.selCol, words))))
        return fail(PIL2GL_EINVAL, "the scratch overlaps f, t or a selector");
    P2_TRY(ensure_init());
    return launch(f, t, n, (u32)k, mode, scratch, p, words, hostReport, as_stream(stream));
}

// host matrices, each staged up to the last element touched
int check_host(HostSide f, HostSide t, u64 n, u64 k, u32 mode, u32 words, u64 *hostReport) {
    clean(hostReport);
    P2_TRY(check_shape(f, t, n, k, mode, words, hostReport));
    if (!n) return PIL2GL_OK;
    if (!f.base || !t.base) return fail(PIL2GL_EINVAL, "null buffer");
    const Plan p = tuplecheckplan::plan(n);
    const u64 nF = span_bytes(n, f.stride, top_column(f.cols, k), words) / 8, nT = span_bytes(n, t.stride, top_column(t.cols, k), words) / 8;
    const u64 nSF = f.sel ? span_bytes(n, f.selStride, f.selCol, words) / 8 : 0, nST = t.sel ? span_bytes(n, t.selStride, t.selCol, words) / 8 : 0;
    Stage s(p.bytes / 8 + pad16(nF) + pad16(nT) + pad16(nSF) + pad16(nST));                // staged parts start on 16 bytes
    P2_TRY(s.rc());
    u64 *dScratch = s.take(p.bytes / 8);
    const u64 *parts[4];
    const u64 *host[4] = { f.base, t.base, f.sel, t.sel };
    const u64 len[4] = { nF, nT, nSF, nST };
    for (int i = 0; i < 4; i++) { parts[i] = s.put(host[i], len[i]); s.take(pad16(len[i]) - len[i]); }
    P2_TRY(s.rc());
    f.base = parts[0]; t.base = parts[1]; f.sel = parts[2]; t.sel = parts[3];
    return launch(f, t, n, (u32)k, mode, dScratch, p, words, hostReport, 0);
}

}  // namespace

extern "C" {

int pil2gl_tuple_check_plan(uint64_t n, uint64_t k, uint32_t elemWords, uint32_t mode, uint32_t *outInfo, uint64_t *scratchBytes) {
    if (scratchBytes) *scratchBytes = 0;
    if (const char *m = tuplecheckplan::check(n, k, elemWords, mode)) return fail(PIL2GL_EINVAL, "%s", m);
    const Plan p = tuplecheckplan::plan(n);
    if (outInfo) {
        outInfo[0] = p.capBits; outInfo[1] = THREADS; outInfo[2] = p.blocks; outInfo[3] = LAUNCHES; outInfo[4] = HEADER_BYTES;
        outInfo[5] = (uint32_t)((p.offCounts + 8 * p.capacity - p.offSlots) >> p.capBits);
    }
    if (scratchBytes) *scratchBytes = p.bytes;
    return PIL2GL_OK;
}

uint64_t pil2gl_debug_tuple_home(const uint64_t *words, uint64_t k, uint32_t elemWords, uint64_t capacity) {
    if (!words || k < 1 || k > MAX_K || (elemWords != 1 && elemWords != 4) || !capacity || (capacity & (capacity - 1))) return NONE;
    return tuplecheckplan::home(words, k, elemWords, capacity);
}

uint64_t pil2gl_debug_tuple_check_probe(void) { return g_lastProbe; }

#define TUPLE_ARGS const uint64_t *f, uint64_t fStride, const uint64_t *hostFCols, const uint64_t *t, uint64_t tStride, const uint64_t *hostTCols, \
                   const uint64_t *selF, uint64_t selFStride, uint64_t selFCol, const uint64_t *selT, uint64_t selTStride, uint64_t selTCol,    \
                   uint64_t n, uint64_t k, uint32_t mode
#define TUPLE_SIDES HostSide{ f, fStride, hostFCols, selF, selFStride, selFCol }, HostSide{ t, tStride, hostTCols, selT, selTStride, selTCol }

int pil2gl_tuple_check_dev(TUPLE_ARGS, uint64_t *scratch, uint64_t scratchBytes, uint64_t *hostReport, void *stream) {
    return check_dev(TUPLE_SIDES, n, k, mode, scratch, scratchBytes, 1, hostReport, stream);
}
int pil2gl_bn128_tuple_check_dev(TUPLE_ARGS, uint64_t *scratch, uint64_t scratchBytes, uint64_t *hostReport, void *stream) {
    return check_dev(TUPLE_SIDES, n, k, mode, scratch, scratchBytes, 4, hostReport, stream);
}
int pil2gl_tuple_check(TUPLE_ARGS, uint64_t *hostReport) { return check_host(TUPLE_SIDES, n, k, mode, 1, hostReport); }
int pil2gl_bn128_tuple_check(TUPLE_ARGS, uint64_t *hostReport) { return check_host(TUPLE_SIDES, n, k, mode, 4, hostReport); }

}  // extern "C"
