// The multiplicity column of a lookup on the device, gfx950: for `selF_s {f_s} in selT {t}`, s < nF, the stage-1 witness column m that a
// pil2 grand sum  sum selF / (f + gamma) - sum m / (t + gamma) = 0  needs: m[j] = how many selected rows of all f sides hold the tuple of
// row j of t, written at the tuple's smallest selected row of t, 0 at every other row.  The statement is include/pil2gl.h's;
// tests/lookup_mult_ref.py restates it as one dictionary.  tuple_check.hip says whether the lookup holds; this unit produces what proves it.
//   the table  an index table (index_table.cuh) over t's selected rows only, the key a row's tuple, re-read from t and reduced.  Slots lie
//            two words apart: a slot is 8 bytes, the tuple's smallest selected row of t and beside it the counter.
//   init     every slot to (EMPTY, 0), the header to (no failing row, 0 matched, probe 0): one launch instead of two memsets, because row and
//            counter are neighbours and start from different bytes.  (mult_column.cuh's init kernel, with the slot pair as its fill)
//   build    a lane per row of t puts its row into the table.
//   count    one launch a side of f, a lane per row: find the tuple's slot; add 1 to its counter, or note the row as failing.  Lanes of a wave
//            that reached the same slot are merged before the atomic (below).  The wave's smallest failing (side << 32 | row) goes up by
//            one atomicMin a wave that saw one (smap_cells.cuh report_bad), the wave's matched rows by one atomicAdd.  The walk over the
//            rows and that report are mult_column.cuh's count_rows, shared with range_mult.hip.
//   write    a lane per row of t: find the slot again; the count when the slot's row is this row, else 0; unselected rows 0.  Over Fr the
//            count goes through one Montgomery product with R^2.
// The report's four words are made on the host from the header's two (mult_column_plan.h, as are the checks of a call's buffers).
// Counters and `matched` are sums, the slot rows and the failing pair minima: neither m nor the report depends on the order in which
// atomics land (the probe figure, a debug value, does).
//
// The merge: a range check sends every row of f to a handful of counters.  Up to MERGE_ROUNDS times the wave takes its first lane with an
// add still to make, reads that lane's slot (v_readlane), ballots the lanes on the same slot and lets the first lane add their number in
// ONE atomic; lanes left after the rounds add 1 each.  One tuple: one atomic a wave instead of 64 on one address.  All distinct: four
// rounds of a readlane, a compare and a ballot retire four lanes, the other sixty add as before.  No LDS.  (wave_merge.cuh, shared with range_mult.hip)
//
// Safety: nothing read from f, t or a selector is used as an address.  A slot's row is checked against n before it indexes t (the table's
// `limit`).  Plain vector loads and stores and global atomics only.
#include "common.h"
#include "tuple_side.cuh"
#include "lookup_mult_plan.h"
#include "mult_column.cuh"
#include "wave_merge.cuh"
#include <string.h>

using namespace pil2gl;

namespace {

using namespace tupleside;
using namespace smapplan;
using namespace lookupmultplan;
using namespace multcolumn;

uint64_t g_lastProbe = 0;                            // the longest displacement of the last build (pil2gl_debug_lookup_mult_probe)

template <class F> struct Job {
    Side<F> t;
    u32 n, k;
    u32 *slots;                                      // slot s: its row at [2 s], its counter at [2 s + 1]
    u64 mask;                                        // capacity - 1
};

// the slot that holds the tuple of row i of S, NONE when no slot does; after the build.  self: the row itself when S is t, else EMPTY
template <class F> __device__ __forceinline__ u64 find_row(const Job<F> &J, const Side<F> &S, u64 i, u32 self) {
    return find<2>(J.slots, J.mask, home_of(S, i, J.k, J.mask), J.n, [&](u32 cur) { return cur == self || same_tuple(S, i, J.t, cur, J.k); }).slot;
}

// ---- build ----
template <class F>
__global__ void __launch_bounds__(THREADS) lm_build_kernel(Job<F> J, unsigned long long *hdr) {
    u32 longest = 0;
    for (u64 r = (u64)blockIdx.x * THREADS + threadIdx.x; r < J.n; r += (u64)gridDim.x * THREADS) {
        if (!selected(J.t, r)) continue;
        const Hit h = insert<2>(J.slots, J.mask, home_of(J.t, r, J.k, J.mask), (u32)r, J.n, [&](u32 cur) { return same_tuple(J.t, r, J.t, cur, J.k); });
        longest = h.displaced > longest ? h.displaced : longest;
    }
    report_probe(longest, hdr + H_PROBE);
}

// ---- count: the rows of one side of f ----
template <class F>
__global__ void __launch_bounds__(THREADS) lm_count_kernel(Job<F> J, Side<F> f, u32 side, unsigned long long *hdr) {
    count_rows<THREADS>(f, side, J.n, hdr, [&](u64 r, bool live) {
        const u64 s = live ? find_row(J, f, r, EMPTY) : NONE;
        wavemerge::add_merged<2, 1>(J.slots, (u32)s, s != NONE);                      // a slot's number is below 2^30; the counter lies beside it
        return s != NONE;
    });
}

// ---- write: m for every row of t ----
template <class F>
__global__ void __launch_bounds__(THREADS) lm_write_kernel(Job<F> J, typename F::Mem *m, u64 mStride, u64 mCol) {
    for (u64 r = (u64)blockIdx.x * THREADS + threadIdx.x; r < J.n; r += (u64)gridDim.x * THREADS) {
        u32 c = 0;
        if (selected(J.t, r)) {
            const u64 s = find_row(J, J.t, r, (u32)r);
            if (s != NONE && J.slots[2 * s] == (u32)r) c = J.slots[2 * s + 1];
        }
        F::store(m, r * mStride + mCol, as_element<F>(c));
    }
}

// ---- host side ----
// every launch of a call, on st; the arguments have passed the checks.  Blocks for the report.
template <class F>
int launch_field(const HostSide *f, u32 nF, const HostSide &t, const Out &out, u64 n, u32 k, void *scratch, const Plan &p, u64 *hostReport, hipStream_t st) {
    char *s = (char *)scratch;
    unsigned long long *hdr = (unsigned long long *)(s + p.offHeader);
    Job<F> J{};
    J.t = device_side<F>(t, k);
    J.n = (u32)n; J.k = k;
    J.slots = (u32 *)(s + p.offSlots);
    J.mask = p.capacity - 1;
    const u64 quads = p.bytes / 16;
    mc_init_kernel<<<blocks(quads), THREADS, 0, st>>>((uint4 *)s, quads, make_uint4(EMPTY, 0, EMPTY, 0));
    KERNEL_CHECK();
    lm_build_kernel<F><<<p.blocks, THREADS, 0, st>>>(J, hdr);
    KERNEL_CHECK();
    for (u32 i = 0; i < nF; i++) {
        lm_count_kernel<F><<<p.blocks, THREADS, 0, st>>>(J, device_side<F>(f[i], k), i, hdr);
        KERNEL_CHECK();
    }
    lm_write_kernel<F><<<p.blocks, THREADS, 0, st>>>(J, (typename F::Mem *)out.m, out.stride, out.col);
    KERNEL_CHECK();
    u64 h[HEADER_WORDS_USED];
    HIP_TRY(hipMemcpyAsync(h, hdr, sizeof h, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    report_of(h, hostReport);
    g_lastProbe = h[H_PROBE];
    return PIL2GL_OK;
}

int launch(const HostSide *f, u32 nF, const HostSide &t, const Out &out, u64 n, u32 k, void *scratch, const Plan &p, u32 words, u64 *hostReport, hipStream_t st) {
    return words == 1 ? launch_field<GlField>(f, nF, t, out, n, k, scratch, p, hostReport, st)
                      : launch_field<FrField>(f, nF, t, out, n, k, scratch, p, hostReport, st);
}

// what both forms refuse: 0, or the code after fail().  dev: the pointers are the device's -- aligned, and beside a scratch
int check_call(const HostSide *f, u64 nF, const HostSide *t, const Out &out, u64 n, u64 k, u32 words, u64 *hostReport, bool dev, const void *scratch,
               u64 scratchBytes) {
    if (const char *msg = lookupmultplan::check(n, k, nF, words)) return fail(PIL2GL_EINVAL, "%s", msg);
    if (!hostReport) return fail(PIL2GL_EINVAL, "null hostReport");
    if (!f || !t) return fail(PIL2GL_EINVAL, "null sides");
    char why[80];
    if (check_side("t", *t, n, k, why)) return fail(PIL2GL_EINVAL, "%s", why);
    for (u64 i = 0; i < nF; i++) {
        const char name[4] = { 'f', ' ', (char)('0' + i), 0 };                  // nF <= MAX_SIDES = 8: one digit
        if (check_side(name, f[i], n, k, why)) return fail(PIL2GL_EINVAL, "%s", why);
    }
    if (const char *msg = check_columns(n, out.stride, &out.col, 1)) return fail(PIL2GL_EINVAL, "m: %s", msg);
    if (!n) return PIL2GL_OK;
    Reads all;                                       // t, its selector, then each side of f and its selector
    all.add(*t, k);
    for (u64 i = 0; i < nF; i++) all.add(f[i], k);
    char buffers[128];
    if (const char *msg = check_buffers(all, out, n, words, dev, scratch, scratchBytes, lookupmultplan::plan(n, nF).bytes, "t, every f", "t, an f", buffers))
        return fail(PIL2GL_EINVAL, "%s", msg);
    return PIL2GL_OK;
}

int mult_dev(const HostSide *f, u64 nF, const HostSide *t, const Out &out, u64 n, u64 k, void *scratch, u64 scratchBytes, u32 words, u64 *hostReport, void *stream) {
    clean(hostReport);
    P2_TRY(check_call(f, nF, t, out, n, k, words, hostReport, true, scratch, scratchBytes));
    if (!n) return PIL2GL_OK;
    P2_TRY(ensure_init());
    return launch(f, (u32)nF, *t, out, n, (u32)k, scratch, lookupmultplan::plan(n, nF), words, hostReport, as_stream(stream));
}

// host matrices, each staged up to the last element touched; m's matrix goes up as it is and comes back with the column written
int mult_host(const HostSide *f, u64 nF, const HostSide *t, const Out &out, u64 n, u64 k, u32 words, u64 *hostReport) {
    clean(hostReport);
    P2_TRY(check_call(f, nF, t, out, n, k, words, hostReport, false, nullptr, 0));
    if (!n) return PIL2GL_OK;
    const Plan p = lookupmultplan::plan(n, nF);
    HostSide sides[1 + MAX_SIDES];
    sides[0] = *t;
    for (u64 i = 0; i < nF; i++) sides[1 + i] = f[i];
    return staged(sides, 1 + (u32)nF, k, out, n, words, p.bytes, [&](const Out &dOut, u64 *dScratch) {
        return launch(sides + 1, (u32)nF, sides[0], dOut, n, (u32)k, dScratch, p, words, hostReport, 0);
    });
}

}  // namespace

extern "C" {

int pil2gl_lookup_mult_plan(uint64_t n, uint64_t k, uint64_t nF, uint32_t elemWords, uint32_t *outInfo, uint64_t *scratchBytes) {
    if (scratchBytes) *scratchBytes = 0;
    if (const char *msg = lookupmultplan::check(n, k, nF, elemWords)) return fail(PIL2GL_EINVAL, "%s", msg);
    const Plan p = lookupmultplan::plan(n, nF);
    if (outInfo) {
        outInfo[0] = p.capBits; outInfo[1] = THREADS; outInfo[2] = p.blocks; outInfo[3] = p.launches; outInfo[4] = HEADER_BYTES; outInfo[5] = SLOT_BYTES;
    }
    if (scratchBytes) *scratchBytes = p.bytes;
    return PIL2GL_OK;
}

uint64_t pil2gl_debug_lookup_mult_probe(void) { return g_lastProbe; }

int pil2gl_lookup_mult_dev(const pil2gl_tuple_side *hostF, uint64_t nF, const pil2gl_tuple_side *hostT, uint64_t *m, uint64_t mStride, uint64_t mCol,
                           uint64_t n, uint64_t k, uint64_t *scratch, uint64_t scratchBytes, uint64_t *hostReport, void *stream) {
    return mult_dev(hostF, nF, hostT, Out{ m, mStride, mCol }, n, k, scratch, scratchBytes, 1, hostReport, stream);
}
int pil2gl_bn128_lookup_mult_dev(const pil2gl_tuple_side *hostF, uint64_t nF, const pil2gl_tuple_side *hostT, uint64_t *m, uint64_t mStride, uint64_t mCol,
                                 uint64_t n, uint64_t k, uint64_t *scratch, uint64_t scratchBytes, uint64_t *hostReport, void *stream) {
    return mult_dev(hostF, nF, hostT, Out{ m, mStride, mCol }, n, k, scratch, scratchBytes, 4, hostReport, stream);
}
int pil2gl_lookup_mult(const pil2gl_tuple_side *hostF, uint64_t nF, const pil2gl_tuple_side *hostT, uint64_t *hostM, uint64_t mStride, uint64_t mCol,
                       uint64_t n, uint64_t k, uint64_t *hostReport) {
    return mult_host(hostF, nF, hostT, Out{ hostM, mStride, mCol }, n, k, 1, hostReport);
}
int pil2gl_bn128_lookup_mult(const pil2gl_tuple_side *hostF, uint64_t nF, const pil2gl_tuple_side *hostT, uint64_t *hostM, uint64_t mStride, uint64_t mCol,
                             uint64_t n, uint64_t k, uint64_t *hostReport) {
    return mult_host(hostF, nF, hostT, Out{ hostM, mStride, mCol }, n, k, 4, hostReport);
}

}  // extern "C"
