// Signed-digit recoding of an MSM scalar, shared by the kernels of bn_msm.hip and the host (pil2gl_debug_bn128_msm_digits, the planner's
// tests): no HIP header, the function is __host__ __device__ only under hipcc.
//
// A scalar s < 2^254 is split into windows of c bits, least significant first.  Window w holds raw_w + carry_w in 0..2^c; a value above
// 2^(c-1) becomes value - 2^c with a carry into the next window, so every digit d_w lies in [-(2^(c-1) - 1), 2^(c-1)] and
// s = sum_w d_w 2^(c w).  |d_w| names one of 2^(c-1) buckets, the sign negates the point.  With nWindows * c >= 255 the last window's raw
// value is below 2^(c-1), so its digit is at most 2^(c-1) and no carry leaves it.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define BN_MSM_HD __host__ __device__ __forceinline__
#else
#define BN_MSM_HD inline
#endif

namespace bnm {

constexpr uint32_t MSM_MIN_C = 4, MSM_MAX_C = 16;
constexpr uint32_t MSM_SCALAR_BITS = 254;            // r < 2^254
constexpr uint32_t MSM_MAX_WINDOWS = (MSM_SCALAR_BITS + 1 + MSM_MIN_C - 1) / MSM_MIN_C;

// The next digit of the scalar in s (eight 32-bit limbs, consumed: s is shifted right by c bits), carry in and out.  2 <= c <= 16.
// Constant limb indices only: on the device the scalar stays in registers.
BN_MSM_HD int32_t msm_next_digit(uint32_t s[8], uint32_t &carry, uint32_t c) {
    const uint32_t v = (s[0] & ((1u << c) - 1)) + carry;
    for (int i = 0; i < 7; i++) s[i] = (s[i] >> c) | (s[i + 1] << (32 - c));
    s[7] >>= c;
    carry = v > (1u << (c - 1)) ? 1u : 0u;
    return (int32_t)v - (int32_t)(carry << c);
}

}  // namespace bnm
