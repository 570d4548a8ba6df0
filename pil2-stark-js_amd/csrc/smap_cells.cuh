// Device half of what the units built on the resident sMap share (wtns_exec.hip, conn_pols.hip, conn_check.hip), gfx950: the report of the first cell whose
// index names no signal, the (row, column) walk of a grid-stride lane over a row-major table, and the element of either field as a kernel's
// template parameter.  The host half is smap_plan.h.
#pragma once
#include "common.h"
#include "gl_field.cuh"
#include "bn_elem.cuh"

namespace smapcells {

using namespace pil2gl;

constexpr u64 NO_BAD = ~0ull;                        // the bad cell of a table whose every index names a signal

// the wave's smallest bad cell, one atomic per wave that saw one, none without a cell to report to; every lane of the wave arrives here
__device__ __forceinline__ void report_bad(u64 best, unsigned long long *firstBad) {
    if (!firstBad) return;
    for (int o = 32; o > 0; o >>= 1) { const u64 other = __shfl_xor(best, o, 64); best = other < best ? other : best; }
    if ((threadIdx.x & 63) == 0 && best != NO_BAD) atomicMin(firstBad, (unsigned long long)best);
}

// (row r, column j) of a lane's cells in a table `cols` wide: its first cell by one division, the grid stride then as a precomputed
// (rows, columns) step
struct CellWalk {
    u64 r, j;
    const u64 cols, stepRows, stepCols;
    __device__ __forceinline__ CellWalk(u64 first, u64 stride, u64 cols) : r(first / cols), j(first % cols), cols(cols), stepRows(stride / cols), stepCols(stride % cols) {}
    __device__ __forceinline__ void next() {
        r += stepRows; j += stepCols;
        if (j >= cols) { j -= cols; r++; }
    }
};

// ---- the field of a kernel: Mem an element in memory, Elem in registers.  mul's first operand may be any bit pattern (its value mod the
// modulus counts), its second is canonical, and so is the result; add takes canonical operands; reduce makes any pattern canonical ----
struct GlField {
    typedef u64 Mem;
    typedef u64 Elem;
    static __device__ __forceinline__ Elem load(const Mem *p, u64 i) { return p[i]; }
    static __device__ __forceinline__ void store(Mem *p, u64 i, Elem x) { p[i] = x; }
    static __device__ __forceinline__ Elem reduce(Elem x) { return gl::canon(x); }
    static __device__ __forceinline__ Elem mul(Elem a, Elem b) { return gl::mul(a, b); }
    static __device__ __forceinline__ Elem add(Elem a, Elem b) { return gl::add(a, b); }
    static __device__ __forceinline__ Elem pow(Elem base, u64 e) { return gl::pow(base, e); }
};

// BN254 Fr: two 16-byte halves in memory, eight limbs in registers; mul and pow are Montgomery products
struct FrField {
    struct Mem { uint4 half[2]; };
    struct Elem { u32 v[8]; };
    static __device__ __forceinline__ Elem load(const Mem *p, u64 i) { Elem x; bn::ld_elem(p[i].half, x.v); return x; }
    static __device__ __forceinline__ void store(Mem *p, u64 i, const Elem &x) { bn::st_elem(p[i].half, x.v); }
    static __device__ __forceinline__ Elem reduce(Elem x) { bn::reduce256(x.v); return x; }
    static __device__ __forceinline__ Elem mul(const Elem &a, const Elem &b) { Elem x; bn::fr_mul(x.v, a.v, b.v); return x; }
    static __device__ __forceinline__ Elem add(Elem a, const Elem &b) { bn::fr_add(a.v, b.v); return a; }
    static __device__ __forceinline__ Elem pow(const Elem &base, u64 e) { Elem x; bn::fr_pow(x.v, base.v, e); return x; }
};

}  // namespace smapcells
