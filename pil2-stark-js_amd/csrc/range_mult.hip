// The multiplicity column of a range check on the device, gfx950: for `selF_s f_s in [lo, lo + size)`, s < nF, the column m that
// lookup_mult.hip would give on the materialised range column -- cnt(j) = how many selected rows of all f sides hold lo + j, written at row
// row0 + j of m, 0 at every other row -- without that column: the table is an arithmetic progression, the counter of a value v is v - lo,
// and there is nothing to hash, probe or build.  The statement is include/pil2gl.h's; tests/range_mult_ref.py restates it.
//   init     the counters and the header to zero, the failing pair to none: 16 bytes a lane (mult_column.cuh's init kernel, filling zero).
//   count    one launch a side of f, so that the side's column is a kernel argument.  A lane decodes its row: the element made canonical
//            (over Fr one Montgomery product by 1 first: the normal form), minus lo as a FIELD element, compared with size as a full element.
//            Only a difference below size becomes a counter's index.
//              path 0  size <= the planner's threshold: a workgroup zeroes `size` counters in LDS, its lanes add there, and after a barrier
//                      every non-zero counter goes to the global array by one atomic.  A wave's lanes on one counter serialise in the LDS
//                      unit, at a cost measured below that of the wave merge in front of the add, so the add is plain.
//              path 1  larger ranges: lookup_mult.hip's merged add (wave_merge.cuh) on the global counters.  No LDS.
//            The wave's smallest failing (side << 32 | row) goes up by one atomicMin a wave that saw one (smap_cells.cuh report_bad), the
//            wave's matched rows by one atomicAdd.  Whole workgroups walk the rows, so that every lane reaches the wave-level steps:
//            the walk and that report are mult_column.cuh's count_rows, shared with lookup_mult.hip.
//   write    a lane per row of m: the counter of row - row0 inside the table, 0 outside.  Over Fr the count goes through one Montgomery
//            product with R^2, as lookup_mult.hip's write does (mult_column.cuh's as_element).
// The report's four words are made on the host from the header's two (mult_column_plan.h, as are the checks of a call's buffers).  Counters and `matched` are sums, the failing pair a minimum: neither m
// nor the report depends on the order in which atomics land.
//
// Safety: a counter's index is used only after its comparison with size; nothing else read from a matrix is used as an address; every loop is
// bounded by n or size.  Plain vector loads and stores, global atomics and, on path 0, LDS atomics only.
#include "common.h"
#include "tuple_side.cuh"
#include "range_mult_plan.h"
#include "mult_column.cuh"
#include "range_decode.cuh"
#include "wave_merge.cuh"

using namespace pil2gl;

namespace {

using namespace tupleside;
using namespace smapplan;
using namespace rangemultplan;
using namespace multcolumn;
using namespace rangedecode;                         // the range as the kernels take it and a row's counter in it (shared with mult_session.hip)

// ---- count, path 0: the rows of one side of f into the workgroup's own counters ----
template <class F>
__global__ void __launch_bounds__(LDS_THREADS) rm_count_lds_kernel(Side<F> f, u32 side, Range<F> rg, u32 n, u32 *counters, unsigned long long *hdr) {
    extern __shared__ u32 local[];                   // rg.size counters
    for (u32 j = threadIdx.x; j < rg.size; j += LDS_THREADS) local[j] = 0;
    __syncthreads();
    count_rows<LDS_THREADS>(f, side, n, hdr, [&](u64 r, bool live) {
        u32 idx = 0;
        const bool hit = live && decode(f, r, rg, idx);
        if (hit) atomicAdd(&local[idx], 1u);
        return hit;
    });
    __syncthreads();
    for (u32 j = threadIdx.x; j < rg.size; j += LDS_THREADS) {
        const u32 c = local[j];
        if (c) atomicAdd(&counters[j], c);
    }
}

// ---- count, path 1: the rows of one side of f onto the global counters ----
template <class F>
__global__ void __launch_bounds__(THREADS) rm_count_global_kernel(Side<F> f, u32 side, Range<F> rg, u32 n, u32 *counters, unsigned long long *hdr) {
    count_rows<THREADS>(f, side, n, hdr, [&](u64 r, bool live) {
        u32 idx = 0;
        const bool hit = live && decode(f, r, rg, idx);
        wavemerge::add_merged<1, 0>(counters, idx, hit);                              // idx < size where hit
        return hit;
    });
}

// ---- write: m for every row ----
template <class F>
__global__ void __launch_bounds__(THREADS) rm_write_kernel(const u32 *counters, u32 n, u32 row0, u32 size, typename F::Mem *m, u64 mStride, u64 mCol) {
    for (u64 r = (u64)blockIdx.x * THREADS + threadIdx.x; r < n; r += (u64)gridDim.x * THREADS) {
        const u64 j = r - row0;                      // wraps to a huge value below row0
        const u32 c = r >= row0 && j < size ? counters[j] : 0;
        F::store(m, r * mStride + mCol, as_element<F>(c));
    }
}

// ---- host side ----
struct Call { int64_t lo; u64 size, row0, n; u32 nF, words, force; };

// every launch of a call, on st; the arguments have passed the checks.  Blocks for the report.
template <class F>
int launch_field(const HostSide *f, const Call &c, const Out &out, void *scratch, const Plan &p, u64 *hostReport, hipStream_t st) {
    char *s = (char *)scratch;
    unsigned long long *hdr = (unsigned long long *)(s + p.offHeader);
    u32 *counters = (u32 *)(s + p.offCounters);
    const Range<F> rg = device_range<F>(c.lo, c.size);
    const u64 quads = p.bytes / 16;
    mc_init_kernel<<<blocks(quads), THREADS, 0, st>>>((uint4 *)s, quads, make_uint4(0, 0, 0, 0));
    KERNEL_CHECK();
    for (u32 i = 0; i < c.nF; i++) {
        if (p.path == PATH_LDS) rm_count_lds_kernel<F><<<p.blocks, LDS_THREADS, 4 * p.ldsCounters, st>>>(device_side<F>(f[i], 1), i, rg, (u32)c.n, counters, hdr);
        else rm_count_global_kernel<F><<<p.blocks, THREADS, 0, st>>>(device_side<F>(f[i], 1), i, rg, (u32)c.n, counters, hdr);
        KERNEL_CHECK();
    }
    rm_write_kernel<F><<<blocks(c.n), THREADS, 0, st>>>(counters, (u32)c.n, (u32)c.row0, (u32)c.size, (typename F::Mem *)out.m, out.stride, out.col);
    KERNEL_CHECK();
    u64 h[2];
    HIP_TRY(hipMemcpyAsync(h, hdr, sizeof h, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    report_of(h, hostReport);
    return PIL2GL_OK;
}

int launch(const HostSide *f, const Call &c, const Out &out, void *scratch, const Plan &p, u64 *hostReport, hipStream_t st) {
    return c.words == 1 ? launch_field<GlField>(f, c, out, scratch, p, hostReport, st) : launch_field<FrField>(f, c, out, scratch, p, hostReport, st);
}

// what both forms refuse: 0, or the code after fail().  dev: the pointers are the device's -- aligned, and beside a scratch
int check_call(const HostSide *f, const Call &c, const Out &out, u64 *hostReport, bool dev, const void *scratch, u64 scratchBytes) {
    if (const char *msg = rangemultplan::check(c.n, c.size, c.nF, c.words, c.force)) return fail(PIL2GL_EINVAL, "%s", msg);
    if (!hostReport) return fail(PIL2GL_EINVAL, "null hostReport");
    if (!f) return fail(PIL2GL_EINVAL, "null sides");
    char why[80];
    for (u32 i = 0; i < c.nF; i++) {
        const char name[4] = { 'f', ' ', (char)('0' + i), 0 };                  // nF <= MAX_SIDES = 8: one digit
        if (check_side(name, f[i], c.n, 1, why)) return fail(PIL2GL_EINVAL, "%s", why);
    }
    if (const char *msg = check_columns(c.n, out.stride, &out.col, 1)) return fail(PIL2GL_EINVAL, "m: %s", msg);
    if (!c.n) return PIL2GL_OK;
    if (const char *msg = check_rows(c.n, c.size, c.row0)) return fail(PIL2GL_EINVAL, "%s", msg);
    Reads all;                                       // each side of f and its selector
    for (u32 i = 0; i < c.nF; i++) all.add(f[i], 1);
    char buffers[128];
    if (const char *msg = check_buffers(all, out, c.n, c.words, dev, scratch, scratchBytes, rangemultplan::plan(c.n, c.size, c.nF, c.force).bytes, "every f", "an f", buffers))
        return fail(PIL2GL_EINVAL, "%s", msg);
    return PIL2GL_OK;
}

int range_dev(const HostSide *f, const Call &c, const Out &out, void *scratch, u64 scratchBytes, u64 *hostReport, void *stream) {
    clean(hostReport);
    P2_TRY(check_call(f, c, out, hostReport, true, scratch, scratchBytes));
    if (!c.n) return PIL2GL_OK;
    P2_TRY(ensure_init());
    return launch(f, c, out, scratch, rangemultplan::plan(c.n, c.size, c.nF, c.force), hostReport, as_stream(stream));
}

// host matrices, each staged up to the last element touched; m's matrix goes up as it is and comes back with the column written
int range_host(const HostSide *f, const Call &c, const Out &out, u64 *hostReport) {
    clean(hostReport);
    P2_TRY(check_call(f, c, out, hostReport, false, nullptr, 0));
    if (!c.n) return PIL2GL_OK;
    const Plan p = rangemultplan::plan(c.n, c.size, c.nF, c.force);
    HostSide sides[MAX_SIDES];
    for (u32 i = 0; i < c.nF; i++) sides[i] = f[i];
    return staged(sides, c.nF, 1, out, c.n, c.words, p.bytes, [&](const Out &dOut, u64 *dScratch) { return launch(sides, c, dOut, dScratch, p, hostReport, 0); });
}

// nF as the checks take it: anything above 8 is refused there
Call call_of(u64 nF, int64_t lo, u64 size, u64 row0, u64 n, u32 words, u32 force) {
    return Call{ lo, size, row0, n, (u32)(nF > MAX_SIDES ? MAX_SIDES + 1 : nF), words, force };
}

}  // namespace

extern "C" {

int pil2gl_debug_range_mult_plan(uint64_t n, uint64_t size, uint64_t nF, uint32_t elemWords, uint32_t path, uint32_t *outInfo, uint64_t *scratchBytes) {
    if (scratchBytes) *scratchBytes = 0;
    if (const char *msg = rangemultplan::check(n, size, nF, elemWords, path)) return fail(PIL2GL_EINVAL, "%s", msg);
    const Plan p = rangemultplan::plan(n, size, nF, path);
    if (outInfo) {
        outInfo[0] = p.path; outInfo[1] = p.threads; outInfo[2] = p.blocks; outInfo[3] = p.launches; outInfo[4] = HEADER_BYTES; outInfo[5] = p.ldsCounters;
    }
    if (scratchBytes) *scratchBytes = p.bytes;
    return PIL2GL_OK;
}
int pil2gl_range_mult_plan(uint64_t n, uint64_t size, uint64_t nF, uint32_t elemWords, uint32_t *outInfo, uint64_t *scratchBytes) {
    return pil2gl_debug_range_mult_plan(n, size, nF, elemWords, PATH_AUTO, outInfo, scratchBytes);
}

int pil2gl_debug_range_mult_dev(const pil2gl_tuple_side *hostF, uint64_t nF, int64_t lo, uint64_t size, uint64_t row0, uint64_t *m, uint64_t mStride,
                                uint64_t mCol, uint64_t n, uint64_t *scratch, uint64_t scratchBytes, uint64_t *hostReport, void *stream, uint32_t elemWords,
                                uint32_t path) {
    return range_dev(hostF, call_of(nF, lo, size, row0, n, elemWords, path), Out{ m, mStride, mCol }, scratch, scratchBytes, hostReport, stream);
}
int pil2gl_range_mult_dev(const pil2gl_tuple_side *hostF, uint64_t nF, int64_t lo, uint64_t size, uint64_t row0, uint64_t *m, uint64_t mStride, uint64_t mCol,
                          uint64_t n, uint64_t *scratch, uint64_t scratchBytes, uint64_t *hostReport, void *stream) {
    return range_dev(hostF, call_of(nF, lo, size, row0, n, 1, PATH_AUTO), Out{ m, mStride, mCol }, scratch, scratchBytes, hostReport, stream);
}
int pil2gl_bn128_range_mult_dev(const pil2gl_tuple_side *hostF, uint64_t nF, int64_t lo, uint64_t size, uint64_t row0, uint64_t *m, uint64_t mStride,
                                uint64_t mCol, uint64_t n, uint64_t *scratch, uint64_t scratchBytes, uint64_t *hostReport, void *stream) {
    return range_dev(hostF, call_of(nF, lo, size, row0, n, 4, PATH_AUTO), Out{ m, mStride, mCol }, scratch, scratchBytes, hostReport, stream);
}
int pil2gl_range_mult(const pil2gl_tuple_side *hostF, uint64_t nF, int64_t lo, uint64_t size, uint64_t row0, uint64_t *hostM, uint64_t mStride, uint64_t mCol,
                      uint64_t n, uint64_t *hostReport) {
    return range_host(hostF, call_of(nF, lo, size, row0, n, 1, PATH_AUTO), Out{ hostM, mStride, mCol }, hostReport);
}
int pil2gl_bn128_range_mult(const pil2gl_tuple_side *hostF, uint64_t nF, int64_t lo, uint64_t size, uint64_t row0, uint64_t *hostM, uint64_t mStride,
                            uint64_t mCol, uint64_t n, uint64_t *hostReport) {
    return range_host(hostF, call_of(nF, lo, size, row0, n, 4, PATH_AUTO), Out{ hostM, mStride, mCol }, hostReport);
}

}  // extern "C"
