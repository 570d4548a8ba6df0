// A BN254 element between memory and registers, gfx950: 32 bytes travel as two 16-byte halves and are worked on as eight 32-bit limbs
// (bn_field.cuh, bn_fq.cuh).  The one copy of that move for every unit that takes elements from global memory; bn_ntt.hip's LDS tile
// accessors and bn_expr.hip's typed temporaries are indexed differently and stay where they are.
#pragma once
#include "bn_field.cuh"

namespace bn {

__device__ __forceinline__ void unpack(const uint4 &a, const uint4 &b, u32 x[8]) {
    x[0] = a.x; x[1] = a.y; x[2] = a.z; x[3] = a.w; x[4] = b.x; x[5] = b.y; x[6] = b.z; x[7] = b.w;
}
__device__ __forceinline__ void ld_elem(const uint4 *p, u32 x[8]) {
    const uint4 a = p[0], b = p[1];
    x[0] = a.x; x[1] = a.y; x[2] = a.z; x[3] = a.w; x[4] = b.x; x[5] = b.y; x[6] = b.z; x[7] = b.w;
}
__device__ __forceinline__ void st_elem(uint4 *p, const u32 x[8]) {
    p[0] = make_uint4(x[0], x[1], x[2], x[3]); p[1] = make_uint4(x[4], x[5], x[6], x[7]);
}
// any 256-bit pattern -> its value mod r: 2^256 < 6 r
__device__ __forceinline__ void reduce256(u32 x[8]) {
    u32 t[9];
#pragma unroll
    for (int i = 0; i < 8; i++) t[i] = x[i];
    t[8] = 0;
#pragma unroll
    for (int k = 0; k < 5; k++) cond_sub_r(t);
#pragma unroll
    for (int i = 0; i < 8; i++) x[i] = t[i];
}
// R^2 mod r: fr_mul by it takes a normal-form value to its Montgomery word
__device__ __forceinline__ void ld_r2(u32 r2[8]) {
#pragma unroll
    for (int i = 0; i < 8; i++) r2[i] = r2_limb(i);
}
// base^e by square and multiply, Montgomery in and out
__device__ __forceinline__ void fr_pow(u32 out[8], const u32 base[8], u64 e) {
    u32 b[8], one[8] = { 1, 0, 0, 0, 0, 0, 0, 0 }, r2[8];
#pragma unroll
    for (int i = 0; i < 8; i++) b[i] = base[i];
    ld_r2(r2);
    fr_mul(out, r2, one);                            // R^2 / R: one
    while (e) {
        if (e & 1) fr_mul(out, out, b);
        fr_mul(b, b, b);
        e >>= 1;
    }
}
// all eight 32-bit words decide
__device__ __forceinline__ bool is_zero(const u32 x[8]) { return (x[0] | x[1] | x[2] | x[3] | x[4] | x[5] | x[6] | x[7]) == 0; }
__device__ __forceinline__ bool is_zero(const uint4 &a, const uint4 &b) { return ((a.x | a.y | a.z | a.w) | (b.x | b.y | b.z | b.w)) == 0; }

}  // namespace bn
