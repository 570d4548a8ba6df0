// BN254 base field Fq for gfx950: eight 32-bit limbs, Montgomery form with R = 2^256 (the bytes ffjavascript's F1 keeps for G1 coordinates,
// so ptau section 2 / zkey.pTau is read as it is).  The product is the finely integrated product scanning of bn_field.cuh's fr_mul, built
// from the same column primitives (acc_column / acc_madn: one asm statement per column; acc_shift) with q's limbs and -q^-1 mod 2^32.
// Every function takes and returns canonical values (< q).  q < 2^254, so a sum of two elements and the unreduced Montgomery product
// (< 2q) fit eight limbs: the final subtractions work on eight limbs, in plain C++ (hipcc makes v_sub_co / v_addc_co chains of them).
#pragma once
#include "bn_field.cuh"
#include "bn_fq_consts.h"

namespace bn {

__device__ __forceinline__ u32 q_limb(int i) { constexpr bnq::Limbs Q = bnq::FQ_Q; return Q.v[i]; }
__device__ __forceinline__ u32 q_one_limb(int i) { constexpr bnq::Limbs R1 = bnq::FQ_R; return R1.v[i]; }

// t < 2q  ->  t mod q, in place
__device__ __forceinline__ void fq_cond_sub(u32 t[8]) {
    u32 d[8], borrow = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const u64 x = (u64)t[i] - q_limb(i) - borrow;
        d[i] = (u32)x;
        borrow = (u32)(x >> 63);
    }
#pragma unroll
    for (int i = 0; i < 8; i++) t[i] = borrow ? t[i] : d[i];
}

__device__ __forceinline__ void fq_add(u32 out[8], const u32 a[8], const u32 b[8]) {
    u32 t[8], carry = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const u64 s = (u64)a[i] + b[i] + carry;
        t[i] = (u32)s;
        carry = (u32)(s >> 32);
    }
    fq_cond_sub(t);
#pragma unroll
    for (int i = 0; i < 8; i++) out[i] = t[i];
}

// a - b: the borrow of the eight-limb difference becomes a mask and q AND the mask is added back
__device__ __forceinline__ void fq_sub(u32 out[8], const u32 a[8], const u32 b[8]) {
    u32 t[8], borrow = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const u64 d = (u64)a[i] - b[i] - borrow;
        t[i] = (u32)d;
        borrow = (u32)(d >> 63);
    }
    const u32 mask = 0u - borrow;
    u32 carry = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const u64 s = (u64)t[i] + (q_limb(i) & mask) + carry;
        out[i] = (u32)s;
        carry = (u32)(s >> 32);
    }
}

__device__ __forceinline__ bool fq_is_zero(const u32 a[8]) { return (a[0] | a[1] | a[2] | a[3] | a[4] | a[5] | a[6] | a[7]) == 0; }
__device__ __forceinline__ bool fq_eq(const u32 a[8], const u32 b[8]) {
    u32 x = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) x |= a[i] ^ b[i];
    return x == 0;
}

// -a  (0 stays 0: q - 0 would not be canonical)
__device__ __forceinline__ void fq_neg(u32 out[8], const u32 a[8]) {
    const u32 mask = fq_is_zero(a) ? 0u : ~0u;
    u32 borrow = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const u64 d = (u64)(q_limb(i) & mask) - a[i] - borrow;
        out[i] = (u32)d;
        borrow = (u32)(d >> 63);
    }
}

// out = a * b / 2^256 mod q   (a, b < q); out may be a or b
template <int I>
__device__ __forceinline__ void fq_mul_col(u64 &lo, u32 &hi, const u32 a[8], const u32 b[8], u32 m[8], const u32 ql[8], u32 t[8]) {
    acc_column<I, 8, false>(lo, hi, a, b);                   // a_j b_(I-j)
    acc_column<I, (I < 8 ? I : 8), false>(lo, hi, m, ql);    // m_j q_(I-j), j < I: only the m already known
    if constexpr (I < 8) { m[I] = (u32)lo * bnq::FQ_N0INV; acc_mad(lo, hi, m[I], ql[0]); }      // low word becomes 0
    else t[I - 8] = (u32)lo;
    acc_shift(lo, hi);
    if constexpr (I < 15) fq_mul_col<I + 1>(lo, hi, a, b, m, ql, t);
}
__device__ __forceinline__ void fq_mul(u32 out[8], const u32 a[8], const u32 b[8]) {
    u32 m[8], t[8], ql[8];
#pragma unroll
    for (int i = 0; i < 8; i++) ql[i] = q_limb(i);
    u64 lo = 0; u32 hi = 0;
    fq_mul_col<0>(lo, hi, a, b, m, ql, t);                   // (ab + mq) / 2^256 < 2q < 2^255: the ninth limb is zero
    fq_cond_sub(t);
#pragma unroll
    for (int i = 0; i < 8; i++) out[i] = t[i];
}
__device__ __forceinline__ void fq_sqr(u32 out[8], const u32 a[8]) { fq_mul(out, a, a); }
__device__ __forceinline__ void fq_dbl(u32 out[8], const u32 a[8]) { fq_add(out, a, a); }

// a^-1 = a^(q-2) (0 -> 0), Montgomery in and out: 254 squarings and a product per set bit; the exponent's bits come from q's constant limbs
__device__ __noinline__ void fq_inv(u32 out[8], const u32 a[8]) {
    u32 acc[8];
#pragma unroll
    for (int i = 0; i < 8; i++) acc[i] = q_one_limb(i);
    for (int bit = 253; bit >= 0; bit--) {
        fq_sqr(acc, acc);
        u32 w = 0;                                           // limb bit/32 of q - 2 (q's lowest limb ends in ...47: no borrow)
#pragma unroll
        for (int l = 0; l < 8; l++) if ((bit >> 5) == l) w = q_limb(l) - (l == 0 ? 2u : 0u);
        if ((w >> (bit & 31)) & 1) fq_mul(acc, acc, a);
    }
#pragma unroll
    for (int i = 0; i < 8; i++) out[i] = acc[i];
}

}  // namespace bn
