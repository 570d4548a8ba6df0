// A row's counter in a range table, gfx950, what range_mult.hip and mult_session.hip share: the range [lo, lo + size) as the kernels take it
// and the decode of one row of a side of f.  The table is implicit: the counter of a value v is (v - lo) mod p|r, and the value is in range
// when that difference, a FULL field element (64 bits, or 256), lies below size.  lo in either field is range_mult_plan.h's.
// Safety: idx is a counter's number only where decode() returned true, that is below size.
#pragma once
#include "common.h"
#include "tuple_side.cuh"
#include "range_mult_plan.h"

namespace rangedecode {

using namespace pil2gl;
using namespace tupleside;

// the range as the kernels take it: lo as a canonical element of the field (normal form over Fr), size
template <class F> struct Range;
template <> struct Range<GlField> { u64 lo; u32 size; };
template <> struct Range<FrField> { u32 lo[8]; u32 size; };

// row i of side f: is its value in the range, and then its counter.  The difference is a full field element: 64 bits, or 256
__device__ __forceinline__ bool decode(const Side<GlField> &f, u64 i, const Range<GlField> &rg, u32 &idx) {
    const u64 d = gl::sub(elem_of(f, i, 0), rg.lo);
    idx = (u32)d;
    return d < rg.size;
}
__device__ __forceinline__ bool decode(const Side<FrField> &f, u64 i, const Range<FrField> &rg, u32 &idx) {
    const FrField::Elem one = { { 1, 0, 0, 0, 0, 0, 0, 0 } };
    // any pattern times 1 over R: the normal form, canonical by FrField::mul's contract (below (2^256 + 2^256 r) / 2^256 before its subtraction)
    FrField::Elem v = FrField::mul(FrField::load(f.base, i * f.stride + f.cols[0]), one);
    bn::fr_sub(v.v, rg.lo);
    idx = v.v[0];
    return (v.v[1] | v.v[2] | v.v[3] | v.v[4] | v.v[5] | v.v[6] | v.v[7]) == 0 && v.v[0] < rg.size;
}

template <class F> inline Range<F> device_range(int64_t lo, u64 size);
template <> inline Range<GlField> device_range<GlField>(int64_t lo, u64 size) { return Range<GlField>{ rangemultplan::lo_mod_p(lo), (u32)size }; }
template <> inline Range<FrField> device_range<FrField>(int64_t lo, u64 size) {
    u64 w[4];
    rangemultplan::lo_mod_r(lo, w);
    Range<FrField> rg{};
    for (int i = 0; i < 4; i++) { rg.lo[2 * i] = (u32)w[i]; rg.lo[2 * i + 1] = (u32)(w[i] >> 32); }
    rg.size = (u32)size;
    return rg;
}

}  // namespace rangedecode
