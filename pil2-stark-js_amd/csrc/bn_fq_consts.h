// BN254 base field Fq: the modulus (the one number typed in) and everything derived from it, computed at compile time.  Eight 32-bit limbs,
// least significant first; Montgomery form with R = 2^256.  No device keywords, no HIP header: the kernels (bn_fq.cuh) and the host-only
// units (bn_msm_plan.cpp, tests/bn_msm_dump.cpp) read the same values.
#pragma once
#include <stdint.h>

namespace bnq {

struct Limbs { uint32_t v[8]; };

// q = 21888242871839275222246405745257275088696311157297823662689037894645226208583
constexpr Limbs FQ_Q = { { 0xd87cfd47u, 0x3c208c16u, 0x6871ca8du, 0x97816a91u, 0x8181585du, 0xb85045b6u, 0xe131a029u, 0x30644e72u } };

constexpr bool fq_ge_q(const Limbs &a) {
    for (int i = 7; i >= 0; i--) if (a.v[i] != FQ_Q.v[i]) return a.v[i] > FQ_Q.v[i];
    return true;
}
// a + b mod q for a, b < q (a + b < 2^255: no carry out of the eighth limb)
constexpr Limbs fq_addmod(const Limbs &a, const Limbs &b) {
    Limbs s = { { 0, 0, 0, 0, 0, 0, 0, 0 } };
    uint64_t c = 0;
    for (int i = 0; i < 8; i++) { c += (uint64_t)a.v[i] + b.v[i]; s.v[i] = (uint32_t)c; c >>= 32; }
    if (fq_ge_q(s)) {
        uint64_t br = 0;
        for (int i = 0; i < 8; i++) { const uint64_t d = (uint64_t)s.v[i] - FQ_Q.v[i] - br; s.v[i] = (uint32_t)d; br = d >> 63; }
    }
    return s;
}
// 2^k mod q by k doublings of 1
constexpr Limbs fq_pow2(int k) {
    Limbs x = { { 1, 0, 0, 0, 0, 0, 0, 0 } };
    for (int i = 0; i < k; i++) x = fq_addmod(x, x);
    return x;
}
// -q^-1 mod 2^32 (Newton: each step doubles the correct low bits; q is odd, so x = 1 is right to one bit)
constexpr uint32_t fq_n0inv() {
    uint32_t x = 1;
    for (int i = 0; i < 5; i++) x *= 2u - FQ_Q.v[0] * x;
    return 0u - x;
}

constexpr Limbs FQ_R = fq_pow2(256);                 // 1 in Montgomery form
constexpr Limbs FQ_R2 = fq_pow2(512);                // the factor that takes a value into Montgomery form
constexpr Limbs FQ_3R = fq_addmod(fq_addmod(FQ_R, FQ_R), FQ_R);   // the curve's b = 3 in Montgomery form (y^2 = x^3 + 3)
constexpr uint32_t FQ_N0INV = fq_n0inv();

}  // namespace bnq
