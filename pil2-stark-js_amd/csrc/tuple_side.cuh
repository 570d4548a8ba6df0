// Device half of one side of a lookup or a permutation (tuple_check.hip, lookup_mult.hip), gfx950: the side as a kernel argument, whether
// it selects a row, a row's tuple as canonical elements, two tuples' equality and a tuple's home slot in the index table (index_table.cuh).
// The host half is tuple_side_plan.h.  same_tuple and home_of take any S that has an elem_of(S, i, j): a Side here; tuple_check.hip
// numbers the rows of both its sides as one index and gives an elem_of over that numbering.
#pragma once
#include "index_table.cuh"
#include "tuple_side_plan.h"

namespace tupleside {

using namespace indextable;

// one side as the kernels take it: the matrix and its k columns, the selector column of a matrix of its own (sel null: every row is selected)
template <class F> struct Side { const typename F::Mem *base, *sel; u64 stride, selStride, selCol; u32 cols[MAX_K]; };

// the side of an entry that has passed check_side(), its pointers the device's
template <class F> Side<F> device_side(const pil2gl_tuple_side &h, u32 k) {
    typedef typename F::Mem Mem;
    Side<F> s{ (const Mem *)h.base, (const Mem *)h.sel, h.stride, h.selStride, h.selCol, {} };
    for (u32 j = 0; j < k; j++) s.cols[j] = (u32)h.hostCols[j];
    return s;
}

template <class F> __device__ __forceinline__ bool selected(const Side<F> &S, u64 i) {
    return !S.sel || !is_zero(F::reduce(F::load(S.sel, i * S.selStride + S.selCol)));
}
// element j of the tuple of row i, canonical
template <class F> __device__ __forceinline__ typename F::Elem elem_of(const Side<F> &S, u64 i, u32 j) {
    return F::reduce(F::load(S.base, i * S.stride + S.cols[j]));
}
template <class SA, class SB> __device__ __forceinline__ bool same_tuple(const SA &A, u64 a, const SB &B, u64 b, u32 k) {
    for (u32 j = 0; j < k; j++)
        if (!same(elem_of(A, a, j), elem_of(B, b, j))) return false;
    return true;
}
template <class S> __device__ __forceinline__ u64 home_of(const S &A, u64 i, u32 k, u64 mask) {
    TupleHash x;
    for (u32 j = 0; j < k; j++) absorb(x, elem_of(A, i, j));
    return x.finish() & mask;
}

}  // namespace tupleside
