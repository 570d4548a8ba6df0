// The packed polynomials of one G1 commit batch (pil2gl_bn128_g1_commit), shared by the kernels of bn_msm.hip, the host
// (pil2gl_debug_bn128_msm_batch_locate) and the stand-alone test program: no HIP header, the functions are __host__ __device__ only under
// hipcc.
//
// Polynomial k of K has n_k = m_k * rows_k coefficients; coefficient i sits in slot j = i mod m_k and row t = i div m_k of a row-major
// matrix of rowStride elements per row: it is 0 where slots[j] is MSM_EMPTY_SLOT, else the element first_k + t * rowStride + slots[j].
// This is fflonk's CPolynomial, f(X) = sum_j X^j p_j(X^m).  The batch's point lanes are the polynomials' coefficients one polynomial after
// the other: lane = sum_{k' < k} n_k' + i.  The struct travels to the kernels as a launch argument (1.3 KB).
#pragma once
#include <stdint.h>
#include "bn_msm_recode.h"

namespace bnm {

constexpr uint32_t MSM_MAX_POLYS = 16, MSM_MAX_SLOTS = 64, MSM_MAX_TOTAL_SLOTS = 256;
constexpr uint32_t MSM_EMPTY_SLOT = 0xFFFFFFFFu;

struct MsmBatch {
    uint64_t first[MSM_MAX_POLYS];                   // element offset of row 0, column 0
    uint32_t rows[MSM_MAX_POLYS], m[MSM_MAX_POLYS];  // m >= 1 for k < K; m * rows <= 2^28
    uint32_t slots[MSM_MAX_TOTAL_SLOTS];             // polynomial k's m_k slots follow those of k - 1
    uint32_t K, rowStride;
};

BN_MSM_HD uint32_t msm_batch_count(const MsmBatch &B, uint32_t k) { return B.rows[k] * B.m[k]; }

// lane -> (k, i); false for a lane at or past the batch's last point
BN_MSM_HD bool msm_batch_locate(const MsmBatch &B, uint64_t lane, uint32_t &k, uint32_t &i) {
    for (uint32_t p = 0; p < B.K && p < MSM_MAX_POLYS; p++) {
        const uint64_t n = msm_batch_count(B, p);
        if (lane < n) { k = p; i = (uint32_t)lane; return true; }
        lane -= n;
    }
    return false;
}

// (k, i) with i < n_k -> the element offset of the coefficient; false for an empty slot (the coefficient is 0)
BN_MSM_HD bool msm_batch_element(const MsmBatch &B, uint32_t k, uint32_t i, uint64_t &element) {
    uint32_t slot0 = 0;
    for (uint32_t p = 0; p < k; p++) slot0 += B.m[p];
    const uint32_t t = i / B.m[k], j = i - t * B.m[k];
    const uint32_t col = B.slots[(slot0 + j) & (MSM_MAX_TOTAL_SLOTS - 1)];
    if (col == MSM_EMPTY_SLOT) return false;
    element = B.first[k] + (uint64_t)t * B.rowStride + col;
    return true;
}

}  // namespace bnm
