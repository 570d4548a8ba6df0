// The lookup and permutation checks on the device, gfx950: does a trace meet `selF {f0..fk-1} in selT {t0..tk-1}` (mode 0, plookup) or
// `selF {f0..fk-1} is selT {t0..tk-1}` (mode 1, permutation), as statements about the trace: no challenge, no field arithmetic beyond
// making an element canonical.  The statement is include/pil2gl.h's; tests/tuple_check_ref.py restates it as one dictionary.
//   the table  ONE index table (index_table.cuh) over both sides' selected rows, t row i as index i, f row i as n + i; the key is the row's
//            tuple, re-read from the matrix the index names and reduced.  Beside each slot: the counter (cntT low half, cntF high half) and
//            the smallest selected f row of the tuple.
//   build    a lane per row of either side puts its row into the table (after the build a slot holds the tuple's smallest t row when t has
//            it, else n + its smallest f row), then one atomicAdd to the counter and, for an f row above the slot's smallest f row so far,
//            nothing, else one atomicMin.
//   judge    every selected row finds its slot again, reads the counter and applies the mode's criterion; the smallest failing row of each
//            side by the wave-minimum rule, one atomic a wave that saw one (smap_cells.cuh report_bad).
//   finish   one workgroup, one lane: f before t, then kind, partner and both counts re-read for the winning tuple alone, so the five words
//            describe one tuple.  Counts, minima and slot contents are sums and minima: none depends on the order in which atomics land.
// One kernel template each over smap_cells.cuh's GlField / FrField, a lane per row in both: a row's k elements are not neighbours in
// memory (cols is any list), so wtns_exec.hip's lane pair per element has no contiguous 32 bytes to split; FrField::load moves an element
// as two 16-byte halves.
//
// Safety: nothing read from f, t or a selector is used as an address.  A slot's content is checked against 2 n before it indexes a matrix
// (the table's `limit`).  Plain vector loads and stores and global atomics only.
#include "common.h"
#include "tuple_side.cuh"
#include "tuple_check_plan.h"
#include <string.h>

using namespace pil2gl;

namespace {

using namespace tupleside;
using namespace smapplan;
using namespace tuplecheckplan;

uint64_t g_lastProbe = 0;                            // the longest displacement of the last build (pil2gl_debug_tuple_check_probe)

template <class F> struct Job {
    Side<F> t, f;
    u32 n, k, mode;
    u32 *slots, *minF;
    unsigned long long *counts;
    u64 mask;                                        // capacity - 1
};

// Rows are numbered as the slots hold them: idx < n is row idx of t, n <= idx < 2 n row idx - n of f.  A lane's idx and the index it
// meets in a slot may lie on either side, so the side is chosen per lane -- field by field, a select between two kernel arguments that
// every lane loads alike.  A per-lane choice between the two Side structs would load each field, the column list above all, per lane.
template <class F> __device__ __forceinline__ bool selected(const Job<F> &J, u32 idx) {
    const bool isF = idx >= J.n;
    const typename F::Mem *sel = isF ? J.f.sel : J.t.sel;
    if (!sel) return true;
    const u64 i = isF ? idx - J.n : idx;
    return !is_zero(F::reduce(F::load(sel, i * (isF ? J.f.selStride : J.t.selStride) + (isF ? J.f.selCol : J.t.selCol))));
}
// element j of the tuple of row idx < 2 n, canonical: what tuple_side.cuh's same_tuple and home_of read a Job by
template <class F> __device__ __forceinline__ typename F::Elem elem_of(const Job<F> &J, u64 idx, u32 j) {
    const u32 r = (u32)idx;
    const bool isF = r >= J.n;
    const u64 i = isF ? r - J.n : r;
    return F::reduce(F::load(isF ? J.f.base : J.t.base, i * (isF ? J.f.stride : J.t.stride) + (isF ? J.f.cols[j] : J.t.cols[j])));
}

// the slot that holds the tuple of row idx, NONE when no slot does; after the build
template <class F> __device__ __forceinline__ u64 find_row(const Job<F> &J, u32 idx) {
    return find<1>(J.slots, J.mask, home_of(J, idx, J.k, J.mask), 2 * J.n, [&](u32 cur) { return cur == idx || same_tuple(J, idx, J, cur, J.k); }).slot;
}

// ---- build ----
template <class F>
__global__ void __launch_bounds__(THREADS) tc_build_kernel(Job<F> J, unsigned long long *hdr) {
    const u64 rows = 2ull * J.n;
    u32 longest = 0;
    for (u64 r = (u64)blockIdx.x * THREADS + threadIdx.x; r < rows; r += (u64)gridDim.x * THREADS) {
        const u32 idx = (u32)r;
        if (!selected(J, idx)) continue;
        const Hit h = insert<1>(J.slots, J.mask, home_of(J, idx, J.k, J.mask), idx, (u32)rows, [&](u32 cur) { return same_tuple(J, idx, J, cur, J.k); });
        if (h.slot == NONE) continue;                                            // the load factor is at most 1 / 2: not reached
        longest = h.displaced > longest ? h.displaced : longest;
        const u64 s = h.slot;
        const bool isF = idx >= J.n;
        atomicAdd(&J.counts[s], isF ? 1ull << 32 : 1ull);
        if (isF && J.minF[s] > idx - J.n) atomicMin(&J.minF[s], idx - J.n);      // what was read only falls: skipping is safe
    }
    report_probe(longest, hdr + H_PROBE);
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
        const u64 s = find_row(J, idx);
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
        const u64 s = find_row(J, (u32)(onF ? J.n + bf : bt));
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

typedef pil2gl_tuple_side HostSide;

// every launch of a call, on st; the arguments have passed the checks.  Blocks for the report.
template <class F>
int launch_field(const HostSide &f, const HostSide &t, u64 n, u32 k, u32 mode, void *scratch, const Plan &p, u64 *hostReport, hipStream_t st) {
    char *s = (char *)scratch;
    unsigned long long *hdr = (unsigned long long *)(s + p.offHeader);
    Job<F> J{};
    J.t = device_side<F>(t, k);
    J.f = device_side<F>(f, k);
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
    char why[80];
    if (check_side("f", f, n, k, why) || check_side("t", t, n, k, why)) return fail(PIL2GL_EINVAL, "%s", why);
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
    for (const HostSide *side : { &f, &t })                                     // an absent selector has no bytes and meets nothing
        if (meets(scratch, p.bytes, side->base, matrix_bytes(*side, n, k, words)) || meets(scratch, p.bytes, side->sel, sel_bytes(*side, n, words)))
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
    Stage s(p.bytes / 8 + staged_words(f, n, k, words) + staged_words(t, n, k, words));
    P2_TRY(s.rc());
    u64 *dScratch = s.take(p.bytes / 8);
    stage_side(s, f, n, k, words);
    stage_side(s, t, n, k, words);
    P2_TRY(s.rc());
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
    return indextable::home(words, k, elemWords, capacity);
}

uint64_t pil2gl_debug_tuple_check_probe(void) { return g_lastProbe; }

#define TUPLE_ARGS const uint64_t *f, uint64_t fStride, const uint64_t *hostFCols, const uint64_t *t, uint64_t tStride, const uint64_t *hostTCols, \
                   const uint64_t *selF, uint64_t selFStride, uint64_t selFCol, const uint64_t *selT, uint64_t selTStride, uint64_t selTCol,    \
                   uint64_t n, uint64_t k, uint32_t mode
#define TUPLE_SIDES pil2gl_tuple_side{ f, fStride, hostFCols, selF, selFStride, selFCol }, pil2gl_tuple_side{ t, tStride, hostTCols, selT, selTStride, selTCol }

int pil2gl_tuple_check_dev(TUPLE_ARGS, uint64_t *scratch, uint64_t scratchBytes, uint64_t *hostReport, void *stream) {
    return check_dev(TUPLE_SIDES, n, k, mode, scratch, scratchBytes, 1, hostReport, stream);
}
int pil2gl_bn128_tuple_check_dev(TUPLE_ARGS, uint64_t *scratch, uint64_t scratchBytes, uint64_t *hostReport, void *stream) {
    return check_dev(TUPLE_SIDES, n, k, mode, scratch, scratchBytes, 4, hostReport, stream);
}
int pil2gl_tuple_check(TUPLE_ARGS, uint64_t *hostReport) { return check_host(TUPLE_SIDES, n, k, mode, 1, hostReport); }
int pil2gl_bn128_tuple_check(TUPLE_ARGS, uint64_t *hostReport) { return check_host(TUPLE_SIDES, n, k, mode, 4, hostReport); }

}  // extern "C"
