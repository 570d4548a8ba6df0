// Multiplicity sessions on the device, gfx950: the column m of a table that lives in an AIR of its own, counted over the f sides of OTHER
// AIRs as their instances arrive -- lookup_mult.hip's and range_mult.hip's one call (init, count, write) cut into open, add and write, the
// counters staying in the caller's working buffer between the calls.  The statement is include/pil2gl.h's; tests/mult_session_ref.py
// restates it over Python integers.  Both table kinds and both fields live here; the one-shot units keep their kernels and their layout.
//   open     the header and the counters (mult_column.cuh's init kernel; the debug form fills every counter with a seed).  A lookup
//            session then builds the index table (index_table.cuh) over t's selected rows, a lane per row of t.  Slots lie four words
//            apart: the tuple's smallest selected row of t, a word unused, the 64-bit counter -- a probe and the add that follows it meet
//            one cache line, where a counter array of its own would cost every matched row a second line.
//   add      one lane first: the last add's matched rows into the session's total, the failing pair to none, matched to 0 -- the add's
//            own report without a word coming back to the host before the report itself.  Then one count launch a side WITH ROWS, its
//            grid from that side's rows (mult_session_plan.h count_blocks): a side of 100 rows launches one workgroup whatever the table,
//            a side of 2^28 rows against a table of 5 the whole grid.  The row walk and what a wave hands up are mult_column.cuh's
//            count_rows; a row's counter is range_decode.cuh's, or the table's find.
//              lookup, range path 1   wave_merge.cuh's merged add in 64 bits on the global counters
//              range path 0           a workgroup's `size` counters in LDS stay 32 bits (a launch gives a workgroup fewer than 2^28 rows);
//                                     after a barrier every non-zero one goes up by ONE 64-bit global atomic
//   write    lookup: a lane per row of t finds its slot again: the counter when the slot's row is this row, else 0.  range: a lane per row
//            of m, the counter of row - row0 inside the table, 0 outside.  The count becomes an element by as_element64: itself over
//            Goldilocks, one Montgomery product of its two words with R^2 over Fr.  Does not end the session.
// Counters and `matched` are sums, slot rows and the failing pair minima: nothing depends on the order in which atomics land.
//
// Safety: nothing read from f, t or a selector becomes an address before its bound check: a counter's index is used only after its
// comparison with size, a slot's row only below nT (the table's `limit`).  Every loop is bounded by a row count, size or the capacity.
// Plain vector loads and stores, global atomics and, on range path 0, LDS atomics only.
#include "common.h"
#include "tuple_side.cuh"
#include "mult_session_plan.h"
#include "mult_column.cuh"
#include "range_decode.cuh"
#include "wave_merge.cuh"
#include <string.h>

using namespace pil2gl;

namespace {

using namespace tupleside;
using namespace smapplan;
using namespace multsessionplan;
using namespace multcolumn;
using namespace rangedecode;

typedef unsigned long long ull;

u32 g_lastGrids[MAX_SIDES] = {};                     // the workgroups of the last add's count launches, a side (pil2gl_debug_mult_session_grids)

// a count below 2^64 in canonical form (Goldilocks: below p, the statement's limit): itself, or count R mod r over Fr
template <class F> __device__ __forceinline__ typename F::Elem as_element64(u64 c);
template <> __device__ __forceinline__ u64 as_element64<GlField>(u64 c) { return c; }
template <> __device__ __forceinline__ FrField::Elem as_element64<FrField>(u64 c) {
    FrField::Elem r2, x = { { (u32)c, (u32)(c >> 32), 0, 0, 0, 0, 0, 0 } };
    if (!c) return x;
    bn::ld_r2(r2.v);
    return FrField::mul(r2, x);
}

// ---- add, its first launch: one lane closes the last add ----
__global__ void ms_begin_kernel(ull *hdr) {
    hdr[H_TOTAL] += hdr[H_MATCHED];
    hdr[H_MATCHED] = 0;
    hdr[H_FAIL] = NONE;
}

// ---- the lookup session's table ----
template <class F> struct Table {
    Side<F> t;
    u32 n, k;
    u32 *slots;                                      // slot s: its row at [4 s], its counter the 64-bit word at [4 s + 2]
    u64 mask;                                        // capacity - 1
};

// the slot that holds the tuple of row i of S, NONE when no slot does; after the build.  self: the row itself when S is t, else EMPTY
template <class F> __device__ __forceinline__ u64 find_row(const Table<F> &T, const Side<F> &S, u64 i, u32 self) {
    return find<SLOT_WORDS>(T.slots, T.mask, home_of(S, i, T.k, T.mask), T.n, [&](u32 cur) { return cur == self || same_tuple(S, i, T.t, cur, T.k); }).slot;
}

template <class F>
__global__ void __launch_bounds__(THREADS) ms_build_kernel(Table<F> T) {
    for (u64 r = (u64)blockIdx.x * THREADS + threadIdx.x; r < T.n; r += (u64)gridDim.x * THREADS) {
        if (!selected(T.t, r)) continue;
        insert<SLOT_WORDS>(T.slots, T.mask, home_of(T.t, r, T.k, T.mask), (u32)r, T.n, [&](u32 cur) { return same_tuple(T.t, r, T.t, cur, T.k); });
    }
}

// the `rows` rows of one side of f against the table
template <class F>
__global__ void __launch_bounds__(THREADS) ms_lookup_count_kernel(Table<F> T, Side<F> f, u32 side, u32 rows, ull *hdr) {
    count_rows<THREADS>(f, side, rows, hdr, [&](u64 r, bool live) {
        const u64 s = live ? find_row(T, f, r, EMPTY) : NONE;
        wavemerge::add_merged64<SLOT_WORDS / 2, COUNTER_WORD / 2>((ull *)T.slots, (u32)s, s != NONE);     // a slot's number is below 2^30
        return s != NONE;
    });
}

template <class F>
__global__ void __launch_bounds__(THREADS) ms_lookup_write_kernel(Table<F> T, typename F::Mem *m, u64 mStride, u64 mCol) {
    for (u64 r = (u64)blockIdx.x * THREADS + threadIdx.x; r < T.n; r += (u64)gridDim.x * THREADS) {
        u64 c = 0;
        if (selected(T.t, r)) {
            const u64 s = find_row(T, T.t, r, (u32)r);
            if (s != NONE && T.slots[SLOT_WORDS * s] == (u32)r) c = ((const ull *)T.slots)[SLOT_WORDS / 2 * s + COUNTER_WORD / 2];
        }
        F::store(m, r * mStride + mCol, as_element64<F>(c));
    }
}

// ---- the range session ----
// path 0: the rows of one side of f into the workgroup's own 32-bit counters, then one 64-bit atomic a non-zero counter
template <class F>
__global__ void __launch_bounds__(LDS_THREADS) ms_range_count_lds_kernel(Side<F> f, u32 side, Range<F> rg, u32 rows, ull *counters, ull *hdr) {
    extern __shared__ u32 local[];                   // rg.size counters
    for (u32 j = threadIdx.x; j < rg.size; j += LDS_THREADS) local[j] = 0;
    __syncthreads();
    count_rows<LDS_THREADS>(f, side, rows, hdr, [&](u64 r, bool live) {
        u32 idx = 0;
        const bool hit = live && decode(f, r, rg, idx);
        if (hit) atomicAdd(&local[idx], 1u);
        return hit;
    });
    __syncthreads();
    for (u32 j = threadIdx.x; j < rg.size; j += LDS_THREADS) {
        const u32 c = local[j];
        if (c) atomicAdd(&counters[j], (ull)c);
    }
}

// path 1: onto the global counters
template <class F>
__global__ void __launch_bounds__(THREADS) ms_range_count_global_kernel(Side<F> f, u32 side, Range<F> rg, u32 rows, ull *counters, ull *hdr) {
    count_rows<THREADS>(f, side, rows, hdr, [&](u64 r, bool live) {
        u32 idx = 0;
        const bool hit = live && decode(f, r, rg, idx);
        wavemerge::add_merged64<1, 0>(counters, idx, hit);                            // idx < size where hit
        return hit;
    });
}

template <class F>
__global__ void __launch_bounds__(THREADS) ms_range_write_kernel(const ull *counters, u32 n, u32 row0, u32 size, typename F::Mem *m, u64 mStride, u64 mCol) {
    for (u64 r = (u64)blockIdx.x * THREADS + threadIdx.x; r < n; r += (u64)gridDim.x * THREADS) {
        const u64 j = r - row0;                      // wraps to a huge value below row0
        const u64 c = r >= row0 && j < size ? counters[j] : 0;
        F::store(m, r * mStride + mCol, as_element64<F>(c));
    }
}

// ---- host side ----
ull *header(void *scratch) { return (ull *)scratch; }                                // offHeader is 0 in both plans

int init(void *scratch, u64 bytes, uint4 fill, hipStream_t st) {
    const u64 quads = bytes / 16;
    mc_init_kernel<<<blocks(quads), THREADS, 0, st>>>((uint4 *)scratch, quads, fill);
    KERNEL_CHECK();
    return PIL2GL_OK;
}

// the add's report: blocks until the header's words are on the host
int fetch_report(void *scratch, u64 *hostReport, hipStream_t st) {
    u64 h[2];
    HIP_TRY(hipMemcpyAsync(h, header(scratch), sizeof h, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    report_of(h, hostReport);
    return PIL2GL_OK;
}

// the session's matched rows: with a hostTotal the call blocks for it
int fetch_total(void *scratch, u64 *hostTotal, hipStream_t st) {
    if (!hostTotal) return PIL2GL_OK;
    u64 h[HEADER_WORDS_USED];
    HIP_TRY(hipMemcpyAsync(h, header(scratch), sizeof h, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    *hostTotal = h[H_TOTAL] + h[H_MATCHED];
    return PIL2GL_OK;
}

template <class F> Table<F> table_of(const HostSide &t, u64 nT, u32 k, void *scratch, const LookupPlan &p) {
    Table<F> T{};
    T.t = device_side<F>(t, k);
    T.n = (u32)nT; T.k = k;
    T.slots = (u32 *)((char *)scratch + p.offSlots);
    T.mask = p.capacity - 1;
    return T;
}

// what every entry of a lookup session refuses about the table and the scratch; spans: the matrices the call touches beside t.  nT > 0
int check_lookup_call(const HostSide *t, u64 nT, u64 k, u32 words, Spans &spans, const void *scratch, u64 scratchBytes) {
    char why[80], buffers[128];
    if (check_side("t", *t, nT, k, why)) return fail(PIL2GL_EINVAL, "%s", why);
    spans.add(*t, nT, k, words);
    if (const char *msg = check_spans(spans, scratch, scratchBytes, plan_lookup(nT).bytes, buffers)) return fail(PIL2GL_EINVAL, "%s", msg);
    return PIL2GL_OK;
}

template <class F> int lookup_open_field(const HostSide &t, u64 nT, u32 k, void *scratch, const LookupPlan &p, u64 seed, hipStream_t st) {
    P2_TRY(init(scratch, p.bytes, make_uint4(EMPTY, 0, (u32)seed, (u32)(seed >> 32)), st));
    ms_build_kernel<F><<<p.blocks, THREADS, 0, st>>>(table_of<F>(t, nT, k, scratch, p));
    KERNEL_CHECK();
    return PIL2GL_OK;
}

int lookup_open(const HostSide *t, u64 nT, u64 k, void *scratch, u64 scratchBytes, void *stream, u32 words, u64 seed) {
    if (const char *msg = check_lookup(nT, k, words)) return fail(PIL2GL_EINVAL, "%s", msg);
    if (!t) return fail(PIL2GL_EINVAL, "null sides");
    if (!nT) return PIL2GL_OK;
    Spans spans;
    P2_TRY(check_lookup_call(t, nT, k, words, spans, scratch, scratchBytes));
    P2_TRY(ensure_init());
    const LookupPlan p = plan_lookup(nT);
    return words == 1 ? lookup_open_field<GlField>(*t, nT, (u32)k, scratch, p, seed, as_stream(stream))
                      : lookup_open_field<FrField>(*t, nT, (u32)k, scratch, p, seed, as_stream(stream));
}

template <class F>
int lookup_add_field(const HostSide &t, u64 nT, u32 k, const HostSide *f, const u64 *rows, u32 nF, void *scratch, const LookupPlan &p, u64 *hostReport, hipStream_t st) {
    const Table<F> T = table_of<F>(t, nT, k, scratch, p);
    ms_begin_kernel<<<1, 1, 0, st>>>(header(scratch));
    KERNEL_CHECK();
    memset(g_lastGrids, 0, sizeof g_lastGrids);
    for (u32 i = 0; i < nF; i++) {
        g_lastGrids[i] = rows[i] ? count_blocks(rows[i], PATH_GLOBAL) : 0;
        if (!rows[i]) continue;
        ms_lookup_count_kernel<F><<<g_lastGrids[i], THREADS, 0, st>>>(T, device_side<F>(f[i], k), i, (u32)rows[i], header(scratch));
        KERNEL_CHECK();
    }
    return fetch_report(scratch, hostReport, st);
}

int lookup_add(const HostSide *t, u64 nT, u64 k, const HostSide *f, const u64 *rows, u64 nF, void *scratch, u64 scratchBytes, u64 *hostReport, void *stream, u32 words) {
    clean(hostReport);
    if (const char *msg = check_lookup(nT, k, words)) return fail(PIL2GL_EINVAL, "%s", msg);
    if (!hostReport) return fail(PIL2GL_EINVAL, "null hostReport");
    if (!t) return fail(PIL2GL_EINVAL, "null sides");
    char why[80];
    if (const char *msg = check_add_sides(f, rows, nF, k, why)) return fail(PIL2GL_EINVAL, "%s", msg);
    if (!nT) return PIL2GL_OK;
    Spans spans;
    for (u64 i = 0; i < nF; i++) spans.add(f[i], rows[i], k, words);
    P2_TRY(check_lookup_call(t, nT, k, words, spans, scratch, scratchBytes));
    P2_TRY(ensure_init());
    const LookupPlan p = plan_lookup(nT);
    return words == 1 ? lookup_add_field<GlField>(*t, nT, (u32)k, f, rows, (u32)nF, scratch, p, hostReport, as_stream(stream))
                      : lookup_add_field<FrField>(*t, nT, (u32)k, f, rows, (u32)nF, scratch, p, hostReport, as_stream(stream));
}

template <class F> int lookup_write_field(const HostSide &t, u64 nT, u32 k, const Out &out, void *scratch, const LookupPlan &p, hipStream_t st) {
    ms_lookup_write_kernel<F><<<p.blocks, THREADS, 0, st>>>(table_of<F>(t, nT, k, scratch, p), (typename F::Mem *)out.m, out.stride, out.col);
    KERNEL_CHECK();
    return PIL2GL_OK;
}

int lookup_write(const HostSide *t, u64 nT, u64 k, const Out &out, void *scratch, u64 scratchBytes, u64 *hostTotal, void *stream, u32 words) {
    if (hostTotal) *hostTotal = 0;
    if (const char *msg = check_lookup(nT, k, words)) return fail(PIL2GL_EINVAL, "%s", msg);
    if (!t) return fail(PIL2GL_EINVAL, "null sides");
    if (const char *msg = check_columns(nT, out.stride, &out.col, 1)) return fail(PIL2GL_EINVAL, "m: %s", msg);
    if (!nT) return PIL2GL_OK;
    Spans spans;
    P2_TRY(check_lookup_call(t, nT, k, words, spans, scratch, scratchBytes));
    const LookupPlan p = plan_lookup(nT);
    if (const char *msg = check_m(out, nT, words, t, k, scratch, p.bytes)) return fail(PIL2GL_EINVAL, "%s", msg);
    P2_TRY(ensure_init());
    const hipStream_t st = as_stream(stream);
    P2_TRY(words == 1 ? lookup_write_field<GlField>(*t, nT, (u32)k, out, scratch, p, st) : lookup_write_field<FrField>(*t, nT, (u32)k, out, scratch, p, st));
    return fetch_total(scratch, hostTotal, st);
}

// ---- the range session's entries ----
int range_open(u64 size, void *scratch, u64 scratchBytes, void *stream, u64 seed) {
    if (const char *msg = check_range(size, 1)) return fail(PIL2GL_EINVAL, "%s", msg);
    char buffers[128];
    const RangePlan p = plan_range(size);
    if (const char *msg = check_spans(Spans(), scratch, scratchBytes, p.bytes, buffers)) return fail(PIL2GL_EINVAL, "%s", msg);
    P2_TRY(ensure_init());
    return init(scratch, p.bytes, make_uint4((u32)seed, (u32)(seed >> 32), (u32)seed, (u32)(seed >> 32)), as_stream(stream));
}

template <class F>
int range_add_field(int64_t lo, u64 size, const HostSide *f, const u64 *rows, u32 nF, void *scratch, const RangePlan &p, u64 *hostReport, hipStream_t st) {
    ull *counters = (ull *)((char *)scratch + p.offCounters);
    const Range<F> rg = device_range<F>(lo, size);
    ms_begin_kernel<<<1, 1, 0, st>>>(header(scratch));
    KERNEL_CHECK();
    memset(g_lastGrids, 0, sizeof g_lastGrids);
    for (u32 i = 0; i < nF; i++) {
        const u32 grid = g_lastGrids[i] = rows[i] ? count_blocks(rows[i], p.path) : 0;
        if (!rows[i]) continue;
        if (p.path == PATH_LDS) ms_range_count_lds_kernel<F><<<grid, LDS_THREADS, 4 * p.ldsCounters, st>>>(device_side<F>(f[i], 1), i, rg, (u32)rows[i], counters, header(scratch));
        else ms_range_count_global_kernel<F><<<grid, THREADS, 0, st>>>(device_side<F>(f[i], 1), i, rg, (u32)rows[i], counters, header(scratch));
        KERNEL_CHECK();
    }
    return fetch_report(scratch, hostReport, st);
}

int range_add(int64_t lo, u64 size, const HostSide *f, const u64 *rows, u64 nF, void *scratch, u64 scratchBytes, u64 *hostReport, void *stream, u32 words, u32 force) {
    clean(hostReport);
    if (const char *msg = check_range(size, words, force)) return fail(PIL2GL_EINVAL, "%s", msg);
    if (!hostReport) return fail(PIL2GL_EINVAL, "null hostReport");
    char why[80], buffers[128];
    if (const char *msg = check_add_sides(f, rows, nF, 1, why)) return fail(PIL2GL_EINVAL, "%s", msg);
    Spans spans;
    for (u64 i = 0; i < nF; i++) spans.add(f[i], rows[i], 1, words);
    const RangePlan p = plan_range(size, force);
    if (const char *msg = check_spans(spans, scratch, scratchBytes, p.bytes, buffers)) return fail(PIL2GL_EINVAL, "%s", msg);
    P2_TRY(ensure_init());
    return words == 1 ? range_add_field<GlField>(lo, size, f, rows, (u32)nF, scratch, p, hostReport, as_stream(stream))
                      : range_add_field<FrField>(lo, size, f, rows, (u32)nF, scratch, p, hostReport, as_stream(stream));
}

int range_write(u64 size, u64 row0, const Out &out, u64 nM, void *scratch, u64 scratchBytes, u64 *hostTotal, void *stream, u32 words) {
    if (hostTotal) *hostTotal = 0;
    if (const char *msg = check_range(size, words)) return fail(PIL2GL_EINVAL, "%s", msg);
    if (nM > MAX_N) return fail(PIL2GL_EINVAL, "nM must be at most 2^28 rows");
    if (const char *msg = rangemultplan::check_rows(nM, size, row0)) return fail(PIL2GL_EINVAL, "%s", msg);
    if (const char *msg = check_columns(nM, out.stride, &out.col, 1)) return fail(PIL2GL_EINVAL, "m: %s", msg);
    char buffers[128];
    const RangePlan p = plan_range(size);
    if (const char *msg = check_spans(Spans(), scratch, scratchBytes, p.bytes, buffers)) return fail(PIL2GL_EINVAL, "%s", msg);
    if (const char *msg = check_m(out, nM, words, nullptr, 0, scratch, p.bytes)) return fail(PIL2GL_EINVAL, "%s", msg);
    P2_TRY(ensure_init());
    const hipStream_t st = as_stream(stream);
    const ull *counters = (const ull *)((char *)scratch + p.offCounters);
    if (words == 1) ms_range_write_kernel<GlField><<<blocks(nM), THREADS, 0, st>>>(counters, (u32)nM, (u32)row0, (u32)size, (GlField::Mem *)out.m, out.stride, out.col);
    else ms_range_write_kernel<FrField><<<blocks(nM), THREADS, 0, st>>>(counters, (u32)nM, (u32)row0, (u32)size, (FrField::Mem *)out.m, out.stride, out.col);
    KERNEL_CHECK();
    return fetch_total(scratch, hostTotal, st);
}

void plan_words(uint32_t *outInfo, u32 first, u32 threads, u32 fullBlocks, u32 launches, u32 unitBytes) {
    if (!outInfo) return;
    outInfo[0] = first; outInfo[1] = threads; outInfo[2] = fullBlocks; outInfo[3] = launches; outInfo[4] = HEADER_BYTES; outInfo[5] = unitBytes;
}

}  // namespace

extern "C" {

int pil2gl_lookup_session_plan(uint64_t nT, uint64_t k, uint32_t elemWords, uint32_t *outInfo, uint64_t *scratchBytes) {
    if (scratchBytes) *scratchBytes = 0;
    if (const char *msg = check_lookup(nT, k, elemWords)) return fail(PIL2GL_EINVAL, "%s", msg);
    const LookupPlan p = plan_lookup(nT);
    plan_words(outInfo, p.capBits, THREADS, count_blocks(MAX_N, PATH_GLOBAL), LOOKUP_LAUNCHES, SLOT_BYTES);
    if (scratchBytes) *scratchBytes = p.bytes;
    return PIL2GL_OK;
}
int pil2gl_debug_range_session_plan(uint64_t size, uint32_t elemWords, uint32_t path, uint32_t *outInfo, uint64_t *scratchBytes) {
    if (scratchBytes) *scratchBytes = 0;
    if (const char *msg = check_range(size, elemWords, path)) return fail(PIL2GL_EINVAL, "%s", msg);
    const RangePlan p = plan_range(size, path);
    plan_words(outInfo, p.path, p.threads, count_blocks(MAX_N, p.path), RANGE_LAUNCHES, COUNTER_BYTES);
    if (scratchBytes) *scratchBytes = p.bytes;
    return PIL2GL_OK;
}
int pil2gl_range_session_plan(uint64_t size, uint32_t elemWords, uint32_t *outInfo, uint64_t *scratchBytes) {
    return pil2gl_debug_range_session_plan(size, elemWords, PATH_AUTO, outInfo, scratchBytes);
}

void pil2gl_debug_mult_session_grids(uint32_t *outGrids) {
    if (outGrids) memcpy(outGrids, g_lastGrids, sizeof g_lastGrids);
}

int pil2gl_lookup_session_open_dev(const pil2gl_tuple_side *hostT, uint64_t nT, uint64_t k, uint64_t *scratch, uint64_t scratchBytes, void *stream) {
    return lookup_open(hostT, nT, k, scratch, scratchBytes, stream, 1, 0);
}
int pil2gl_bn128_lookup_session_open_dev(const pil2gl_tuple_side *hostT, uint64_t nT, uint64_t k, uint64_t *scratch, uint64_t scratchBytes, void *stream) {
    return lookup_open(hostT, nT, k, scratch, scratchBytes, stream, 4, 0);
}
int pil2gl_debug_lookup_session_open_dev(const pil2gl_tuple_side *hostT, uint64_t nT, uint64_t k, uint64_t *scratch, uint64_t scratchBytes, void *stream,
                                         uint32_t elemWords, uint64_t seed) {
    return lookup_open(hostT, nT, k, scratch, scratchBytes, stream, elemWords, seed);
}
int pil2gl_range_session_open_dev(uint64_t size, uint64_t *scratch, uint64_t scratchBytes, void *stream) { return range_open(size, scratch, scratchBytes, stream, 0); }
int pil2gl_debug_range_session_open_dev(uint64_t size, uint64_t *scratch, uint64_t scratchBytes, void *stream, uint64_t seed) {
    return range_open(size, scratch, scratchBytes, stream, seed);
}

int pil2gl_lookup_session_add_dev(const pil2gl_tuple_side *hostT, uint64_t nT, uint64_t k, const pil2gl_tuple_side *hostF, const uint64_t *hostRows, uint64_t nF,
                                  uint64_t *scratch, uint64_t scratchBytes, uint64_t *hostReport, void *stream) {
    return lookup_add(hostT, nT, k, hostF, hostRows, nF, scratch, scratchBytes, hostReport, stream, 1);
}
int pil2gl_bn128_lookup_session_add_dev(const pil2gl_tuple_side *hostT, uint64_t nT, uint64_t k, const pil2gl_tuple_side *hostF, const uint64_t *hostRows,
                                        uint64_t nF, uint64_t *scratch, uint64_t scratchBytes, uint64_t *hostReport, void *stream) {
    return lookup_add(hostT, nT, k, hostF, hostRows, nF, scratch, scratchBytes, hostReport, stream, 4);
}
int pil2gl_range_session_add_dev(int64_t lo, uint64_t size, const pil2gl_tuple_side *hostF, const uint64_t *hostRows, uint64_t nF, uint64_t *scratch,
                                 uint64_t scratchBytes, uint64_t *hostReport, void *stream) {
    return range_add(lo, size, hostF, hostRows, nF, scratch, scratchBytes, hostReport, stream, 1, PATH_AUTO);
}
int pil2gl_bn128_range_session_add_dev(int64_t lo, uint64_t size, const pil2gl_tuple_side *hostF, const uint64_t *hostRows, uint64_t nF, uint64_t *scratch,
                                       uint64_t scratchBytes, uint64_t *hostReport, void *stream) {
    return range_add(lo, size, hostF, hostRows, nF, scratch, scratchBytes, hostReport, stream, 4, PATH_AUTO);
}
int pil2gl_debug_range_session_add_dev(int64_t lo, uint64_t size, const pil2gl_tuple_side *hostF, const uint64_t *hostRows, uint64_t nF, uint64_t *scratch,
                                       uint64_t scratchBytes, uint64_t *hostReport, void *stream, uint32_t elemWords, uint32_t path) {
    return range_add(lo, size, hostF, hostRows, nF, scratch, scratchBytes, hostReport, stream, elemWords, path);
}

int pil2gl_lookup_session_write_dev(const pil2gl_tuple_side *hostT, uint64_t nT, uint64_t k, uint64_t *m, uint64_t mStride, uint64_t mCol, uint64_t *scratch,
                                    uint64_t scratchBytes, uint64_t *hostTotal, void *stream) {
    return lookup_write(hostT, nT, k, Out{ m, mStride, mCol }, scratch, scratchBytes, hostTotal, stream, 1);
}
int pil2gl_bn128_lookup_session_write_dev(const pil2gl_tuple_side *hostT, uint64_t nT, uint64_t k, uint64_t *m, uint64_t mStride, uint64_t mCol,
                                          uint64_t *scratch, uint64_t scratchBytes, uint64_t *hostTotal, void *stream) {
    return lookup_write(hostT, nT, k, Out{ m, mStride, mCol }, scratch, scratchBytes, hostTotal, stream, 4);
}
int pil2gl_range_session_write_dev(uint64_t size, uint64_t row0, uint64_t *m, uint64_t mStride, uint64_t mCol, uint64_t nM, uint64_t *scratch,
                                   uint64_t scratchBytes, uint64_t *hostTotal, void *stream) {
    return range_write(size, row0, Out{ m, mStride, mCol }, nM, scratch, scratchBytes, hostTotal, stream, 1);
}
int pil2gl_bn128_range_session_write_dev(uint64_t size, uint64_t row0, uint64_t *m, uint64_t mStride, uint64_t mCol, uint64_t nM, uint64_t *scratch,
                                         uint64_t scratchBytes, uint64_t *hostTotal, void *stream) {
    return range_write(size, row0, Out{ m, mStride, mCol }, nM, scratch, scratchBytes, hostTotal, stream, 4);
}

}  // extern "C"
