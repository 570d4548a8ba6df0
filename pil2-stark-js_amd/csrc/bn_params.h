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

}  // namespace bnp
