// BN254 Poseidon parameters on the host: the 256-bit arithmetic, the published parameter generation (Grain LFSR), the sparse form of the
// partial rounds and the matrix-core operand tiles / row constants -- every byte the kernels of bn128.hip read, as a pure function of the
// width.  No HIP header: builds with plain g++ -std=c++17 as well as with hipcc (tests/bn_params_dump.cpp runs it under the sanitizers).
#pragma once
#include <stdint.h>
#include <string>
#include <vector>

namespace bnp {

struct U256 { uint64_t w[4]; };
U256 h_to_mont(const U256 &a);                       // a 2^256 mod r
U256 h_from_mont(const U256 &a);                     // a / 2^256 mod r
U256 bn_mont_mul(const U256 &a, const U256 &b);
const U256 &bn_mont_one();                           // 1 in Montgomery form
const U256 &bn_mont_neg_one();                       // r - 1 in Montgomery form
U256 bn_mont_pow(U256 base, uint64_t e);             // base^e, Montgomery form in and out
// four 64-bit words as the eight 32-bit limbs the kernels work on
inline void bn_limbs(const uint64_t w[4], uint32_t out[8]) { for (int i = 0; i < 4; i++) { out[2 * i] = (uint32_t)w[i]; out[2 * i + 1] = (uint32_t)(w[i] >> 32); } }

constexpr size_t BN_ABSENT = (size_t)-1;             // the offset of a region this width does not have

// The three tables of one state width t as the device holds them, and where each region starts:
//   elems   Montgomery form, 32 bytes per element; offsets in elements
//     C8[8][t]  constants of the 4+4 full rounds (the first of the second half also carries what the partial rounds pushed out)
//     M[t][t]   dense MDS (m00 = its first element);  S[RP] scalar constants;  V[RP][t-1], W[RP][t-1] sparse rows / columns
//     Cd[(8+RP)][t] the original constants (the dense statement of the chain kernel, perm_small's first round)
//   tiles   matrix-core operand tiles (bn_mfma.cuh), 1 KB each; offsets in tiles; every region is followed by BN_SPARE_TILES zero tiles
//     Mt / Dt   the dense layer and D = diag(1, Mhat^RP);  Pt the tile stream of the blocked partial rounds (mfma_partial_tables)
//     Mt0       the first layer for inputs S-boxed as plain integers;  St the two tile sets of the widths <= BN_SMALL_T (else absent)
//   consts  plain integers mod r, 32 bytes each; offsets in elements
//     MK[8][t] / DK / MK0 / SK the row constants of Mt / Dt / Mt0 / St (SK absent with St), KR / KU those of Pt's rows and columns,
//     C0p the first round's constants as plain integers
struct BnHostParams {
    int t = 0, rp = 0;
    std::vector<U256> elems, consts;
    std::vector<int8_t> tiles;
    size_t C8, M, S, V, W, Cd, m00;
    size_t Mt, Dt, Pt, Mt0, St;
    size_t MK, DK, KR, KU, MK0, C0p, SK;
    std::string error;                               // what went wrong when bn_build_params does not return 0
};

// t = 2..17.  No device, no globals.  Returns 0, or PIL2GL_EINVAL with out.error set.
int bn_build_params(int t, BnHostParams &out);

// ---- the Fr transforms (bn_ntt.hip) ----
// Roots of unity as ffjavascript's Fr.w[] has them: w[28] = 5^((r-1)/2^28) (5: the smallest quadratic non-residue), w[k] = w[k+1]^2;
// wi[k] = 1/w[k], ninv[k] = 1/2^k.  Montgomery form, computed on first use with the host arithmetic above (nothing typed in).
struct BnNttConsts { U256 w[29], wi[29], ninv[29]; };
const BnNttConsts &bn_ntt_consts();
// out[i] = g^i, i < n (Montgomery form in and out)
void bn_powers(const U256 &g, size_t n, U256 *out);
// The sweeps of a transform of 2^nBits rows: layers[i] butterfly layers in sweep i, as even as ceil(nBits / BN_NTT_KMAX) sweeps allow (the
// first ones take the odd layers).  A sweep of K layers holds 2^K rows x min(nPols, BN_NTT_TILE_ELEMS >> K) columns.  Returns the number of
// sweeps (0 for nBits = 0), -1 for nBits > BN_NTT_MAX_BITS.  layers: room for BN_NTT_MAX_SWEEPS.
int bn_ntt_plan(unsigned nBits, unsigned *layers);

// ---- the G1 multi-scalar multiplication (bn_msm.hip) ----
// How a batch of K MSMs over the same bases runs, polynomial k of counts[k] points (K = 1 is the single MSM; a batch without points plans
// as one point): windows of c bits (signed digits, bn_msm_recode.h), nWindows = ceil(255 / c) of them, bucketsPerWindow = 2^(c-1), one c
// for the batch: floor(log2 max_k counts[k]) - 3 within [4, 16], lowered while K * nWindows * bucketsPerWindow bucket points exceed
// BN_MSM_BUCKET_BUDGET = 9 * 2^19 (never for K = 1: 16 windows of 2^15 buckets are 2^19; only from 16 to 15, for K >= 10: sixteen
// polynomials fit at c = 15.  The budget is this large on purpose: the widths below 15 have a top window of few scalar bits -- c = 14
// keeps 2 of them -- so that a few buckets take a quarter of a polynomial's points each, one lane adding them one after the other).  The point lists of windowsPerPass windows of every
// polynomial are built and accumulated at a time: the largest power of two that keeps N * windowsPerPass list entries, N = sum_k
// counts[k], within clamp(8 N, 2^19, 2^30) and K * windowsPerPass * bucketsPerWindow histogram cells within BN_MSM_PASS_CELLS (what
// the one-workgroup scan is given; K = 1 never reaches it), at most nWindows.
// The working buffer, in bytes from its start (every region 16-byte aligned); window w of polynomial k is item w * K + k throughout:
//   offHist     K * windowsPerPass * bucketsPerWindow + 1 u32: the pass's histogram, then its exclusive scan (the last entry: the total)
//   offCursor   one u32 per bucket of the pass: where the scatter writes next
//   offEntries  N * windowsPerPass u32: point index within its polynomial | sign << 31, grouped by bucket
//   offBuckets  K * nWindows * bucketsPerWindow points of 128 bytes (X, Y, ZZ, ZZZ): every window's bucket sums
//   offLevelA / offLevelB   the reduction's levels (X then Y, K * nWindows * m1 resp. K * nWindows * m2 points each), used alternately
// scratchBytes <= 4 * clamp(8 N, 2^19, 2^30) + 96 MiB * min(K, 9) for every K <= 16 and N <= 2^28: the lists, then 2 MiB of histogram
// and cursors, and buckets and levels of at most min(K, 9) * 2^19 bucket points at 128 * (1 + 2/8 + 2/128) bytes and a little.
constexpr uint32_t BN_MSM_L1 = 8, BN_MSM_L = 16;     // buckets per lane in the reduction's first level / items per lane in the later ones
constexpr uint64_t BN_MSM_BUCKET_BUDGET = 9ull << 19, BN_MSM_PASS_CELLS = 1ull << 18;
struct BnMsmPlan {
    uint32_t c, nWindows, bucketsPerWindow, windowsPerPass, m1, m2;
    uint64_t offHist, offCursor, offEntries, offBuckets, offLevelA, offLevelB, scratchBytes;
};
BnMsmPlan bn_msm_batch_plan(uint32_t K, const uint64_t *counts);
inline BnMsmPlan bn_msm_plan(uint64_t n) { return bn_msm_batch_plan(1, &n); }

}  // namespace bnp
