// The multiplicity column of a lookup on the device, gfx950: for `selF_s {f_s} in selT {t}`, s < nF, the stage-1 witness column m that a
// pil2 grand sum  sum selF / (f + gamma) - sum m / (t + gamma) = 0  needs: m[j] = how many selected rows of all f sides hold the tuple of
// row j of t, written at the tuple's smallest selected row of t, 0 at every other row.  The statement is include/pil2gl.h's;
// tests/lookup_mult_ref.py restates it as one dictionary.  tuple_check.hip says whether the lookup holds; this unit produces what proves it.
//   the table  an index table (index_table.cuh) over t's selected rows only, the key a row's tuple, re-read from t and reduced.  Slots lie
//            two words apart: a slot is 8 bytes, the tuple's smallest selected row of t and beside it the counter.
//   init     every slot to (EMPTY, 0), the header to (no failing row, 0 matched, probe 0): one launch instead of two memsets, because row and
//            counter are neighbours and start from different bytes.
//   build    a lane per row of t puts its row into the table.
//   count    one launch a side of f, a lane per row: find the tuple's slot; add 1 to its counter, or note the row as failing.  Lanes of a wave
//            that reached the same slot are merged before the atomic (below).  The wave's smallest failing (side << 32 | row) goes up by
//            one atomicMin a wave that saw one (smap_cells.cuh report_bad), the wave's matched rows by one atomicAdd.
//   write    a lane per row of t: find the slot again; the count when the slot's row is this row, else 0; unselected rows 0.  Over Fr the
//            count goes through one Montgomery product with R^2.
// The report's four words are made on the host from the header's two.  Counters and `matched` are sums, the slot rows and the failing pair
// minima: neither m nor the report depends on the order in which atomics land (the probe figure, a debug value, does).
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
#include "wave_merge.cuh"
#include <string.h>

using namespace pil2gl;

namespace {

using namespace tupleside;
using namespace smapplan;
using namespace lookupmultplan;

uint64_t g_lastProbe = 0;                            // the longest displacement of the last build (pil2gl_debug_lookup_mult_probe)

template <class F> struct Job {
    Side<F> t;
    u32 n, k;
    u32 *slots;                                      // slot s: its row at [2 s], its counter at [2 s + 1]
    u64 mask;                                        // capacity - 1
};

// a count below 2^32 in canonical form: itself over Goldilocks, count R mod r over Fr
template <class F> __device__ __forceinline__ typename F::Elem as_element(u32 c);
template <> __device__ __forceinline__ u64 as_element<GlField>(u32 c) { return c; }
template <> __device__ __forceinline__ FrField::Elem as_element<FrField>(u32 c) {
    FrField::Elem r2, x = { { c, 0, 0, 0, 0, 0, 0, 0 } };
    if (!c) return x;
    bn::ld_r2(r2.v);
    return FrField::mul(r2, x);
}

// the slot that holds the tuple of row i of S, NONE when no slot does; after the build.  self: the row itself when S is t, else EMPTY
template <class F> __device__ __forceinline__ u64 find_row(const Job<F> &J, const Side<F> &S, u64 i, u32 self) {
    return find<2>(J.slots, J.mask, home_of(S, i, J.k, J.mask), J.n, [&](u32 cur) { return cur == self || same_tuple(S, i, J.t, cur, J.k); }).slot;
}

// ---- init: header and slots ----
__global__ void __launch_bounds__(THREADS) lm_init_kernel(uint4 *buf, u64 quads) {
    static_assert(HEADER_BYTES == 64 && H_FAIL == 0 && H_MATCHED == 1, "the first 16 bytes: no failing pair, nothing matched");
    for (u64 q = (u64)blockIdx.x * THREADS + threadIdx.x; q < quads; q += (u64)gridDim.x * THREADS)
        buf[q] = q == 0 ? make_uint4(EMPTY, EMPTY, 0, 0) : q < HEADER_BYTES / 16 ? make_uint4(0, 0, 0, 0) : make_uint4(EMPTY, 0, EMPTY, 0);
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
    u64 bad = NO_BAD;
    u32 matched = 0;
    // whole workgroups walk the rows, so that every lane of a wave reaches the merge
    for (u64 first = (u64)blockIdx.x * THREADS; first < J.n; first += (u64)gridDim.x * THREADS) {
        const u64 r = first + threadIdx.x;
        const bool live = r < J.n && selected(f, r);
        const u64 s = live ? find_row(J, f, r, EMPTY) : NONE;
        const bool hit = s != NONE;
        if (live && !hit) bad = r < bad ? r : bad;
        matched += hit;
        wavemerge::add_merged<2, 1>(J.slots, (u32)s, hit);                           // a slot's number is below 2^30; the counter lies beside it
    }
    report_bad(bad == NO_BAD ? NO_BAD : (u64)side << 32 | bad, hdr + H_FAIL);
    for (int o = 32; o > 0; o >>= 1) matched += __shfl_xor(matched, o, 64);
    if ((threadIdx.x & 63) == 0 && matched) atomicAdd(hdr + H_MATCHED, (unsigned long long)matched);
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
typedef pil2gl_tuple_side HostSide;
struct Out { u64 *m; u64 stride, col; };

void clean(u64 *report) { if (report) { report[0] = CLEAN; report[1] = report[2] = NONE; report[3] = 0; } }

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
    lm_init_kernel<<<blocks(quads), THREADS, 0, st>>>((uint4 *)s, quads);
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
    const bool failed = h[H_FAIL] != NONE;
    hostReport[0] = failed ? F_NOT_IN_T : CLEAN;
    hostReport[1] = failed ? h[H_FAIL] >> 32 : NONE;
    hostReport[2] = failed ? h[H_FAIL] & 0xFFFFFFFFull : NONE;
    hostReport[3] = h[H_MATCHED];
    g_lastProbe = h[H_PROBE];
    return PIL2GL_OK;
}

int launch(const HostSide *f, u32 nF, const HostSide &t, const Out &out, u64 n, u32 k, void *scratch, const Plan &p, u32 words, u64 *hostReport, hipStream_t st) {
    return words == 1 ? launch_field<GlField>(f, nF, t, out, n, k, scratch, p, hostReport, st)
                      : launch_field<FrField>(f, nF, t, out, n, k, scratch, p, hostReport, st);
}

// the matrices a call reads: t, its selector, then each side of f and its selector; at most 2 + 2 MAX_SIDES
struct Reads { ReadMatrix r[2 + 2 * MAX_SIDES]; u32 count = 0; };
void add_reads(Reads &all, const HostSide &s, u64 k) {
    all.r[all.count++] = ReadMatrix{ s.base, s.stride, s.hostCols, k };
    if (s.sel) all.r[all.count++] = ReadMatrix{ s.sel, s.selStride, &s.selCol, 1 };
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
    Reads all;
    add_reads(all, *t, k);
    for (u64 i = 0; i < nF; i++) add_reads(all, f[i], k);
    uintptr_t bits = (uintptr_t)out.m | (uintptr_t)scratch;
    bool null = !out.m || (dev && !scratch);
    for (u32 i = 0; i < all.count; i++) { bits |= (uintptr_t)all.r[i].base; null = null || !all.r[i].base; }
    if (null) return fail(PIL2GL_EINVAL, "null buffer");
    if (dev && (bits & 15)) return fail(PIL2GL_EINVAL, "t, every f, the selectors, m and the scratch must be 16-byte aligned");
    if (dev) {
        const Plan p = lookupmultplan::plan(n, nF);
        if (scratchBytes < p.bytes) return fail(PIL2GL_EINVAL, "the scratch holds %llu bytes, %llu needed", (unsigned long long)scratchBytes, (unsigned long long)p.bytes);
        bool hit = meets(scratch, p.bytes, out.m, span_bytes(n, out.stride, out.col, words));
        for (u32 i = 0; i < all.count; i++) hit = hit || meets(scratch, p.bytes, all.r[i].base, span_bytes(n, all.r[i].stride, top_column(all.r[i].cols, all.r[i].k), words));
        if (hit) return fail(PIL2GL_EINVAL, "the scratch overlaps t, an f, a selector or m");
    }
    for (u32 i = 0; i < all.count; i++)
        if (!m_allowed(out.m, out.stride, out.col, all.r[i], n, words))
            return fail(PIL2GL_EINVAL, "m overlaps a matrix that is read: it may only be a column of that matrix (its base, its stride) that is not read");
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
    const u64 mWords = span_bytes(n, out.stride, out.col, words) / 8;
    u64 total = p.bytes / 8 + pad16(mWords);
    for (u64 i = 0; i <= nF; i++) total += staged_words(sides[i], n, k, words);
    Stage s(total);
    P2_TRY(s.rc());
    u64 *dScratch = s.take(p.bytes / 8);
    for (u64 i = 0; i <= nF; i++) stage_side(s, sides[i], n, k, words);
    const Out dOut{ (u64 *)s.put(out.m, mWords), out.stride, out.col };
    P2_TRY(s.rc());
    P2_TRY(launch(sides + 1, (u32)nF, sides[0], dOut, n, (u32)k, dScratch, p, words, hostReport, 0));
    return s.get(out.m, dOut.m, mWords);
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
