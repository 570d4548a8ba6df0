// Device half of the multiplicity column m, gfx950, what lookup_mult.hip and range_mult.hip share: a count as an element of either field,
// the init of the working buffer, the row walk of a count kernel with what its lanes hand up at its end, and the staging of the
// host-pointer entries.  How a row finds its counter, and the write kernels, are each unit's own.  The host half is mult_column_plan.h.
#pragma once
#include "common.h"
#include "tuple_side.cuh"
#include "mult_column_plan.h"

namespace multcolumn {

using namespace pil2gl;
using namespace tupleside;
using namespace smapplan;

typedef pil2gl_tuple_side HostSide;

// a count below 2^32 in canonical form: itself over Goldilocks, count R mod r over Fr (one Montgomery product with R^2)
template <class F> __device__ __forceinline__ typename F::Elem as_element(u32 c);
template <> __device__ __forceinline__ u64 as_element<GlField>(u32 c) { return c; }
template <> __device__ __forceinline__ FrField::Elem as_element<FrField>(u32 c) {
    FrField::Elem r2, x = { { c, 0, 0, 0, 0, 0, 0, 0 } };
    if (!c) return x;
    bn::ld_r2(r2.v);
    return FrField::mul(r2, x);
}

// ---- init: the header to (no failing pair, nothing matched, zeroes), every 16 bytes behind it to `fill` ----
static __global__ void __launch_bounds__(THREADS) mc_init_kernel(uint4 *buf, u64 quads, uint4 fill) {
    static_assert(HEADER_BYTES == 64 && H_FAIL == 0 && H_MATCHED == 1, "the first 16 bytes: no failing pair, nothing matched");
    for (u64 q = (u64)blockIdx.x * THREADS + threadIdx.x; q < quads; q += (u64)gridDim.x * THREADS)
        buf[q] = q == 0 ? make_uint4(~0u, ~0u, 0, 0) : q < HEADER_BYTES / 16 ? make_uint4(0, 0, 0, 0) : fill;
}

// what a count kernel's lanes hand up at its end: the wave's smallest failing (side << 32 | row) by one atomicMin a wave that saw one
// (smap_cells.cuh report_bad), the wave's matched rows by one atomicAdd; every lane of the wave arrives here
__device__ __forceinline__ void report(u64 bad, u32 matched, u32 side, unsigned long long *hdr) {
    report_bad(bad == NO_BAD ? NO_BAD : (u64)side << 32 | bad, hdr + H_FAIL);
    for (int o = 32; o > 0; o >>= 1) matched += __shfl_xor(matched, o, 64);
    if ((threadIdx.x & 63) == 0 && matched) atomicAdd(hdr + H_MATCHED, (unsigned long long)matched);
}

// The rows of one side of f, for a count kernel of LANES lanes a workgroup.  Whole workgroups walk the rows, so that every lane of a wave
// reaches the wave-level steps of the add and of the report.  add(r, live): r < n is selected when live; finds the row's counter, makes
// the add (every lane calls it, a dead one adds nothing) and returns whether the row hit.
template <u32 LANES, class F, class Add>
__device__ __forceinline__ void count_rows(const Side<F> &f, u32 side, u64 n, unsigned long long *hdr, Add &&add) {
    u64 bad = NO_BAD;
    u32 matched = 0;
    for (u64 first = (u64)blockIdx.x * LANES; first < n; first += (u64)gridDim.x * LANES) {
        const u64 r = first + threadIdx.x;
        const bool live = r < n && selected(f, r);
        const bool hit = add(r, live);
        if (live && !hit) bad = r < bad ? r : bad;
        matched += hit;
    }
    report(bad, matched, side, hdr);
}

// The host-pointer entries: `count` host sides of k columns (the first may be t) staged up to the last element touched, behind a scratch
// of scratchBytes; m's matrix goes up as it is and comes back with the column written.  sides become the device's;
// launch(dOut, dScratch) makes the call's launches and its report.
template <class Launch>
int staged(HostSide *sides, u32 count, u64 k, const Out &out, u64 n, u32 words, u64 scratchBytes, Launch &&launch) {
    const u64 mWords = span_bytes(n, out.stride, out.col, words) / 8;
    u64 total = scratchBytes / 8 + pad16(mWords);
    for (u32 i = 0; i < count; i++) total += staged_words(sides[i], n, k, words);
    Stage s(total);
    P2_TRY(s.rc());
    u64 *dScratch = s.take(scratchBytes / 8);
    for (u32 i = 0; i < count; i++) stage_side(s, sides[i], n, k, words);
    const Out dOut{ (u64 *)s.put(out.m, mWords), out.stride, out.col };
    P2_TRY(s.rc());
    P2_TRY(launch(dOut, dScratch));
    return s.get(out.m, dOut.m, mWords);
}

}  // namespace multcolumn
