// Plain constants of the BN254 Poseidon pipeline that the host parameter builder (bn_params.cpp) and the kernels (bn128.hip, bn_mfma.cuh)
// must agree on: they shape the tables the host writes and the order in which the kernels read them.  No device keywords, no HIP header.
#pragma once

namespace bnc {

// State elements kept in LDS (the rest in private memory: "Where the state lives" in bn128.hip): 10 = 20 KB per wave, two waves per SIMD.  With the
// batch in which the partial rounds fetch the others' operands (partial_rounds_mfma_impl::rows: a batch of four leaves the registers for the
// accumulators) it shapes the order of the tile stream the host writes (mfma_partial_tables).
constexpr int BN_LDS_ELEMS = 10;
constexpr int BN_HI_BATCH = 4;
constexpr int BN_SMALL_T = 4;                        // widths up to this run the permutation round by round with the state and the layer's tiles in registers (perm_small)
constexpr int N_ROUNDS_F = 8;
constexpr int N_ROUNDS_P[16] = { 56, 57, 56, 60, 60, 63, 64, 63, 60, 66, 60, 65, 70, 60, 64, 68 };   // poseidon.circom:8
constexpr int ACC_BIAS = 1 << 30;                    // 2.0f's bit pattern: an inline constant of the matrix instruction (its C operand), no register set-up per accumulator
// A dense layer reads its operand tiles MFMA_AHEAD tiles ahead of their use (dense_mfma_impl), past the end of its table after the last row: every
// tile table is followed by BN_SPARE_TILES zero tiles.  Twice the depth, 16: the committed table digests (tests/golden/bn_params_digests.json) pin it.
constexpr int MFMA_AHEAD = 8;
constexpr int BN_SPARE_TILES = 2 * MFMA_AHEAD;

// The Fr transforms (bn_ntt.hip; their planning and root tables: bn_params.cpp).  A sweep keeps a tile of 2^K rows x a group of columns in LDS,
// 32 bytes per element: 2048 elements = 64 KiB, two workgroups per CU.  K <= 10: the table of tile twiddles holds the 512 powers of w[10].
constexpr unsigned BN_NTT_MAX_BITS = 28;             // Fr.s: r - 1 = 2^28 * odd
constexpr unsigned BN_NTT_KMAX = 10;
constexpr unsigned BN_NTT_TILE_ELEMS = 2048;
constexpr unsigned BN_NTT_MAX_SWEEPS = (BN_NTT_MAX_BITS + BN_NTT_KMAX - 1) / BN_NTT_KMAX;

}  // namespace bnc
