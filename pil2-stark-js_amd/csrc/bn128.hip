// BN128 (BN254 scalar field) Poseidon linear hash and arity-ary Merkle tree, gfx950.
//
// Replaces src/helpers/hash/merklehash/merklehash_bn128_p.js:28-182 (merkelize, _getNNodes, getGroupProof), its worker
// merklehash_bn128_worker.js:13-144 (linearHash, merkelizeLevel) and the third-party kernels those call
// (circomlibjs@0.1.7 buildPoseidonWasm `poseidon`, wasmcurves@0.1.5 F1m `frm_toMontgomery`; neither is under the
// reference tree).  The permutation follows the in-tree statement circuits.bn128/custom/poseidon.circom:6-45
// (t = nInputs+1, RF = 8, RP = N_ROUNDS_P[t-2], x^5, dense round constants and MDS); its parameters are produced on the
// host (bn_params.cpp) by the published Poseidon parameter generation (Grain LFSR) and agree with every constant set the reference holds
// (tests/test_bn128_oracle.py pins the same generator; tests/test_gpu_bn128.py compares this one with it).
//
// One pipeline per width (bn_perm), one permutation per lane, the linear layers on the matrix cores (bn_mfma.cuh) and the S-box in radix
// 2^29 (bn_field29.cuh):
//   t = 2..4    perm_small: round by round as poseidon.circom states it, state and tiles in registers;
//   t = 5..16   the partial rounds in the sparse form (derivation: bn_params.cpp, next to derive_sparse(): 2t-1 products per round instead of t^2),
//               four to a block on the matrix cores (partial_rounds_mfma), the rp % 4 rounds left over on the vector ALU (partial_rounds);
//   t = 17      the same phases in ONE function body (the arity-16 trees).
// Between the layers the state is a lazy representative (< 2^255) in LDS as [element][limb][lane] for the lower elements and in private
// memory for the others ("Where the state lives" below); every round constant but the first rides on a layer's row constants.
// Few permutations (<= WAVE_PER_PERM_MAX) run the circuit's dense statement instead, a wave each (bn_sponge_chain_kernel).
// Nodes are stored as the reference stores them: 4 little-endian u64 words of the Montgomery form.
#include "common.h"
#include "bn_consts.h"
#include "bn_params.h"
#include "bn_field.cuh"
#include "bn_mfma.cuh"
#include "bn_field29.cuh"
#include <mutex>
#include <vector>
#include <string.h>
#include <algorithm>
#include <type_traits>

using namespace pil2gl;
using bn::u32;

namespace {

using namespace bnc;                               // BN_LDS_ELEMS, BN_HI_BATCH, BN_SMALL_T, the round numbers, MFMA_AHEAD: shared with the host parameter builder
constexpr int BN_BLOCK = 64;                         // lanes of a wave = permutations a wave carries
// Waves per workgroup.  Every wave works alone on its own 64 permutations and its own LDS slice; what the waves of a workgroup share is
// TIME: a barrier at the start of every matrix phase (dense layer, rows on y, column update) keeps them on the same operand tiles, so that
// of the workgroup's loads of a tile one goes to the L2 and the others hit the CU's L1.
constexpr int BN_WG_WAVES = 4;
constexpr int BN_THREADS = BN_BLOCK * BN_WG_WAVES;
// Up to this many permutations in one call run a wave each (bn_sponge_chain_kernel): a lane each would leave them at the latency of one wave
// working alone (~3 ms at t = 17); a wave each runs them in ~0.5 ms while the SIMDs outnumber them
constexpr long WAVE_PER_PERM_MAX = 2048;

// device tables of one state width t (their construction and layout: bn_params.h), three allocations: the elements in Montgomery form, 8 limbs each,
// the matrix-core operand tiles and the row constants
struct Params { int t = 0, rp = 0; u32 *base = nullptr, *C8, *M, *S, *V, *W, *Cd; u32 m00[8];
                const bnm::v4i *Mt = nullptr, *Dt = nullptr, *Pt = nullptr; const u32 *MK = nullptr, *DK = nullptr, *KR = nullptr, *KU = nullptr;
                const bnm::v4i *Mt0 = nullptr; const u32 *MK0 = nullptr, *C0p = nullptr;        // the first layer for inputs S-boxed as plain integers (plain_sbox_store)
                const bnm::v4i *St = nullptr; const u32 *SK = nullptr; };                         // widths <= BN_SMALL_T: the round-by-round form in registers (perm_small)
Params g_params[18];
std::mutex g_mu;

int get_params(int t, const Params **out) {
    if (t < 2 || t > 17) return fail(PIL2GL_EINVAL, "BN128 Poseidon takes 1..16 inputs (t=%d)", t);
    std::lock_guard<std::mutex> lk(g_mu);
    Params &P = g_params[t];
    if (!P.t) {
        bnp::BnHostParams H;
        if (const int rc = bnp::bn_build_params(t, H)) return fail(rc, "%s", H.error.c_str());
        const void *src[3] = { H.elems.data(), H.tiles.data(), H.consts.data() };
        const size_t bytes[3] = { H.elems.size() * 32, H.tiles.size(), H.consts.size() * 32 };
        void *d[3] = { nullptr, nullptr, nullptr };
        hipError_t e = hipSuccess;
        for (int k = 0; k < 3 && e == hipSuccess; k++) {
            e = hipMalloc(&d[k], bytes[k]);
            if (e == hipSuccess) e = hipMemcpy(d[k], src[k], bytes[k], hipMemcpyHostToDevice);
        }
        if (e != hipSuccess) {                       // P.t stays 0: a later call tries again
            for (int k = 0; k < 3; k++) if (d[k]) (void)hipFree(d[k]);
            return hip_fail(e, "BN128 parameter upload");
        }
        u32 *el = (u32 *)d[0];
        const int8_t *tl = (const int8_t *)d[1];
        const u32 *kc = (const u32 *)d[2];
        auto tile = [&](size_t o) { return (const bnm::v4i *)(tl + o * 1024); };
        P.base = el; P.C8 = el + H.C8 * 8; P.M = el + H.M * 8; P.S = el + H.S * 8; P.V = el + H.V * 8; P.W = el + H.W * 8; P.Cd = el + H.Cd * 8;
        memcpy(P.m00, H.elems[H.m00].w, 32);
        P.Mt = tile(H.Mt); P.Dt = tile(H.Dt); P.Pt = tile(H.Pt); P.Mt0 = tile(H.Mt0);
        P.MK = kc + H.MK * 8; P.DK = kc + H.DK * 8; P.KR = kc + H.KR * 8; P.KU = kc + H.KU * 8; P.MK0 = kc + H.MK0 * 8; P.C0p = kc + H.C0p * 8;
        if (H.St != bnp::BN_ABSENT) { P.St = tile(H.St); P.SK = kc + H.SK * 8; }
        P.rp = H.rp; P.t = t;
    }
    *out = &P;
    return PIL2GL_OK;
}

// ------------------------------------------------------------------------------------------ device side
struct PermArgs { const u32 *C8, *M, *S, *V, *W, *Cd; int t, rp; u32 m00[8];
                  const bnm::v4i *Mt, *Dt, *Pt; const u32 *MK, *DK, *KR, *KU;
                  const bnm::v4i *Mt0; const u32 *MK0, *C0p;
                  int plain;         // plain: elements 1..t-1 arrive S-boxed from the absorb (leaf kernel, width 17)
                  int nout1;         // nout1: the caller reads element 0 of the result only (sponges, tree nodes): the last layer computes ONE row
                  const bnm::v4i *St; const u32 *SK; };

// Where the state lives.  Elements [0, BN_LDS_ELEMS) in LDS as [element][limb][lane]; the elements above -- only the states
// wider than BN_LDS_ELEMS have any: t = 11..17 -- in the lane's own private (scratch) memory, which the hardware swizzles so
// that a wave's access to one word is one contiguous 256-byte piece.  10 elements = 20 KB of LDS per wave: EIGHT waves per CU
// (two per SIMD: all 160 KB) instead of the four that a 17-element state in LDS allows.  The private half is the kernel's costliest
// traffic (the per-XCD working set of 256 waves' private state plus the tile table passes the 4 MB L2: it travels through the fabric,
// and the card is power-limited): every phase touches it as few times as its registers allow, and never inside a loop that runs a
// tile ring (partial_rounds_mfma_impl).  The element index is static wherever that matters.
typedef u32 __attribute__((address_space(5))) *priv_u32;
typedef u32 __attribute__((address_space(3))) *lds_u32;
struct St { lds_u32 S; priv_u32 hi; int tmax, lane; };
__host__ __device__ constexpr int lds_words(int tmax) { return (tmax < BN_LDS_ELEMS ? tmax : BN_LDS_ELEMS) * 8 * BN_BLOCK; }   // one wave's slice
#define S_LDS(st, j, l) (st).S[(((j) * 8 + (l)) * BN_BLOCK) + (st).lane]

__device__ __forceinline__ void lds_load(const St st, int j, u32 x[8]) {
    if (j < BN_LDS_ELEMS) {
#pragma unroll
        for (int l = 0; l < 8; l++) x[l] = S_LDS(st, j, l);
    } else {
        priv_u32 hp = st.hi;
        asm volatile("" : "+v"(hp));                  // opaque: ONE address register and immediate offsets (hipcc would hoist an address per element into registers of its own)
#pragma unroll
        for (int l = 0; l < 8; l++) x[l] = hp[(j - BN_LDS_ELEMS) * 8 + l];
    }
}
__device__ __forceinline__ void lds_store(const St st, int j, const u32 x[8]) {
    if (j < BN_LDS_ELEMS) {
#pragma unroll
        for (int l = 0; l < 8; l++) S_LDS(st, j, l) = x[l];
    } else {
        priv_u32 hp = st.hi;
        asm volatile("" : "+v"(hp));
#pragma unroll
        for (int l = 0; l < 8; l++) hp[(j - BN_LDS_ELEMS) * 8 + l] = x[l];
    }
}
// An element kept in OPERAND form (the two v4i of bnm::b_prep: bytes signed, halves swapped between the wave's halves) in its usual slot: the y
// of the partial rounds live so from the layer before them to the layer after them -- every rows' pass and column update then LOADS its operand
// where it prepared it (twelve instructions per column and pass: 704 preparations per width-17 permutation become 160)
__device__ __forceinline__ void lds_load_b(const St st, int j, bnm::v4i &b0, bnm::v4i &b1) {
    u32 x[8];
    lds_load(st, j, x);
#pragma unroll
    for (int q = 0; q < 4; q++) { b0[q] = (int)x[q]; b1[q] = (int)x[4 + q]; }
}
__device__ __forceinline__ void lds_store_b(const St st, int j, const bnm::v4i &b0, const bnm::v4i &b1) {
    u32 x[8];
#pragma unroll
    for (int q = 0; q < 4; q++) { x[q] = (u32)b0[q]; x[4 + q] = (u32)b1[q]; }
    lds_store(st, j, x);
}
// wave-uniform address.  The tables live in global memory; saying so (the pointers reach the out-of-line helpers as generic ones)
// turns the flat loads into global loads, whose counter is separate from the LDS one and in order, so that a request for the
// next term can stay in flight across the current multiply
typedef const u32 __attribute__((address_space(1))) *gconst_u32;
__device__ __forceinline__ void load_const(const u32 *p, size_t idx, u32 c[8]) {
    gconst_u32 q = (gconst_u32)(p + idx * 8);
#pragma unroll
    for (int l = 0; l < 8; l++) c[l] = q[l];
}
__device__ __forceinline__ void pow5(u32 x[8]) {
    u32 x2[8], x4[8];
    bn::fr_mul(x2, x, x); bn::fr_mul(x4, x2, x2); bn::fr_mul(x, x4, x);
}
// the same on lazy representatives (a layer's output < 2^255, plus a round constant at most), in radix 2^29 (bn_field29.cuh: no carry
// instructions): x^5 in the state's form times 2^-20 -- the next layer's tiles carry 2^20 -- and any 256-bit value will do for the
// matrix operand that reads it
__device__ __forceinline__ void pow5_lazy(u32 x[8]) { bn29::pow5(x); }
// x + c for a lazy x < 2^255 and a constant c < r: < 0.69 * 2^256, left as it is (the S-box that follows takes it, pow5_lazy)
__device__ __forceinline__ void add_lazy(u32 x[8], const u32 c[8]) { bnm::add_chain8(x, c); }
// The S-box layer of a full round in the matrix-core pipeline: the round's constants arrive with the previous layer's rows
// (except the first round's, C != nullptr); lazy in, lazy out
// (element j + 1 is requested before element j is worked on: more than half of a wide state lives in private memory, whose L2 latency --
// a microsecond -- would otherwise be paid in full by every element; the same in the two loops of partial_rounds_mfma)
__device__ __forceinline__ void sbox_lazy_impl(const St st, int t, const u32 *C) {
    u32 xn[8];
    lds_load(st, 0, xn);
    for (int j = 0; j < t; j++) {
        u32 x[8];
#pragma unroll
        for (int l = 0; l < 8; l++) x[l] = xn[l];
        if (j + 1 < t) lds_load(st, j + 1, xn);
        if (C) {
            u32 c[8];
            load_const(C, (size_t)j, c);
            add_lazy(x, c);
        }
        pow5_lazy(x);
        lds_store(st, j, x);
    }
}
__device__ __noinline__ void sbox_lazy(const St st, int t, const u32 *C) { sbox_lazy_impl(st, t, C); }
__device__ __noinline__ void canon_state(const St st, int t) {
    for (int j = 0; j < t; j++) {
        u32 x[8];
        lds_load(st, j, x);
        bnm::canon(x);
        lds_store(st, j, x);
    }
}

// A dense layer on the matrix cores (bn_mfma.cuh): the N operand pairs are made once and stay in registers, a row is N pairs of
// MFMAs and one short finish; no 32x32 product of the state is left.  The operand tiles come from the L2 as ONE linear stream
// (row after row, tile after tile) read MFMA_AHEAD tiles ahead of their use -- a load per tile and lane, the oldest awaited
// alone -- so the table carries spare tiles after its last one (MFMA_AHEAD and BN_SPARE_TILES: bn_consts.h, the host writes them).
// with the S-box in the row loop the ring is shorter: the S-box needs some of its registers (4 / 6 / 8 tiles 27.15 / 26.9 / 26.9 ms)
constexpr int MFMA_AHEAD_SBOX = 6;
// SBOX: the NEXT round's S-box is applied to every finished row before it is stored (its constant came with the row): the separate S-box pass over
// the state -- a load and a store of every element, seven of them in private memory -- disappears for that round.
// STORE_B: the rows of elements 1.. are stored in operand form (the layer before the partial rounds); LOAD_B: the inputs are in that form (the layer after).
// nrows: the leading rows that are computed (the permutation's last layer when only element 0 of the result is read: one of N)
template <int N, bool SBOX = false, bool STORE_B = false, bool LOAD_B = false>
__device__ __forceinline__ void dense_mfma_impl(const St st, const bnm::v4i *tiles, const u32 *kc, int first, int nrows = N) {
    bnm::v4i B0[N], B1[N];
#pragma unroll
    for (int j = 0; j < N; j++) {
        if constexpr (LOAD_B) lds_load_b(st, first + j, B0[j], B1[j]);
        else {
            u32 x[8];
            lds_load(st, first + j, x);
            bnm::b_prep(x, B0[j], B1[j]);
        }
    }
    const bnm::Sh sh = bnm::sh_init();
    bnm::gtile tp = (bnm::gtile)tiles + st.lane;
    constexpr int AHEAD = SBOX ? MFMA_AHEAD_SBOX : MFMA_AHEAD;
    bnm::v4i q[AHEAD];
    __syncthreads();                                 // the workgroup's waves start the layer's tile stream together
#pragma unroll
    for (int k = 0; k < AHEAD; k++) q[k] = tp[(size_t)k * 64];
    for (int i = 0; i < nrows; i++) {
        u32 k[8], o[8];
        load_const(kc, (size_t)i, k);                // asked for ahead of the row's tiles: an in-order counter waits for everything older than what it wants
        bnm::v16i a0, a1;
#pragma unroll
        for (int j = 0; j < N; j++) {
            const bnm::v4i a = q[0];
#pragma unroll
            for (int k = 0; k + 1 < AHEAD; k++) q[k] = q[k + 1];
            q[AHEAD - 1] = tp[(size_t)(j + AHEAD) * 64];
            if (j == 0) bnm::mfma_first(a, B0[0], B1[0], a0, a1);
            else {
                a0 = bnm::mfma(a, B0[j], a0);
                a1 = bnm::mfma(a, B1[j], a1);
            }
        }
        tp += (size_t)N * 64;
        bnm::finish_row(a0, a1, k, o, sh);
        if constexpr (SBOX) pow5_lazy(o);
        if (STORE_B && first + i >= 1) { bnm::v4i ob0, ob1; bnm::b_prep(o, ob0, ob1); lds_store_b(st, first + i, ob0, ob1); }
        else lds_store(st, first + i, o);            // the old state is in B0 / B1: the new row can go straight to its place
    }
}
template <int N>
__device__ __noinline__ void dense_mfma_n(const St st, const bnm::v4i *tiles, const u32 *kc, int first, int nrows) { dense_mfma_impl<N>(st, tiles, kc, first, nrows < N ? nrows : N); }
// the widths 5..16 of bn_perm: the full rounds' layers (n = t) and the closing layer diag(1, Mh^RP) of the partial rounds (n = t - 1)
__device__ __forceinline__ void dense_mfma(const St st, const bnm::v4i *tiles, const u32 *kc, int n, int first, int nrows = 17) {
    switch (n) {
    case 4: dense_mfma_n<4>(st, tiles, kc, first, nrows); break;
    case 5: dense_mfma_n<5>(st, tiles, kc, first, nrows); break;
    case 6: dense_mfma_n<6>(st, tiles, kc, first, nrows); break;
    case 7: dense_mfma_n<7>(st, tiles, kc, first, nrows); break;
    case 8: dense_mfma_n<8>(st, tiles, kc, first, nrows); break;
    case 9: dense_mfma_n<9>(st, tiles, kc, first, nrows); break;
    case 10: dense_mfma_n<10>(st, tiles, kc, first, nrows); break;
    case 11: dense_mfma_n<11>(st, tiles, kc, first, nrows); break;
    case 12: dense_mfma_n<12>(st, tiles, kc, first, nrows); break;
    case 13: dense_mfma_n<13>(st, tiles, kc, first, nrows); break;
    case 14: dense_mfma_n<14>(st, tiles, kc, first, nrows); break;
    case 15: dense_mfma_n<15>(st, tiles, kc, first, nrows); break;
    default: dense_mfma_n<16>(st, tiles, kc, first, nrows); break;
    }
}

// partial rounds, sparse form, in place: element 0 stays in registers (the rp % 4 rounds the blocks leave over, on canonical values)
__device__ __noinline__ void partial_rounds(const St st, const PermArgs &A, int kFirst) {
    const int t = A.t;
    u32 x0[8], m00[8];
    lds_load(st, 0, x0);
#pragma unroll
    for (int l = 0; l < 8; l++) m00[l] = A.m00[l];
    const int n = t - 1;
    for (int k = kFirst; k < A.rp; k++) {
        u32 c[8];
        load_const(A.S, (size_t)k, c);
        bn::fr_add(x0, c);
        pow5(x0);
        u32 acc[17];
#pragma unroll
        for (int l = 0; l < 17; l++) acc[l] = 0;
        bn::mac17(acc, x0, m00);
        for (int j = 0; j < n; j++) {
            u32 y[8], vv[8], ww[8], p[8];
            lds_load(st, 1 + j, y);
            load_const(A.V, (size_t)k * n + j, vv);
            bn::mac17(acc, y, vv);                   // row 0:   m00*x0 + sum V_kj * y_j
            load_const(A.W, (size_t)k * n + j, ww);
            bn::fr_mul(p, x0, ww);                   // column:  y_j + W_kj * x0
            bn::fr_add(y, p);
            lds_store(st, 1 + j, y);
        }
        bn::redc17(x0, acc);
    }
    lds_store(st, 0, x0);
}

// The partial rounds on the matrix cores, four to a block, two blocks to a super-block (tables: mfma_partial_tables).  Per block: the four
// rows' parts on y (n x 4 pairs of MFMAs -- for a super-block's second block on the y of the super-block's START, plus 16 pairs on the first
// block's S-box outputs -- carried to ten words each), then the four rounds: S-box on the vector ALU, its output z_i made an operand, the
// cross terms of row i (<= 4 pairs) added to the row's stored part, one short finish = the next x0.  Per super-block, once: the n columns
// y_j + sum_k W z_k (1 + 8 pairs and one finish each -- the costliest phase, hence every eight rounds, not four).  No 32x32 product is left
// but the S-box's.  The tiles are ONE linear stream in consumption order, read PR_AHEAD tiles ahead.
constexpr int PR_AHEAD = 4;                          // (deeper read-ahead measured nothing; the registers go to the rows' accumulators and operand batches)
static_assert(BN_SPARE_TILES >= MFMA_AHEAD && BN_SPARE_TILES >= MFMA_AHEAD_SBOX && BN_SPARE_TILES >= PR_AHEAD, "the spare tiles after a table cover the deepest read-ahead");
struct TileStream {
    bnm::gtile p;
    bnm::v4i q[PR_AHEAD];
    __device__ __forceinline__ void start(const bnm::v4i *tiles, int lane) {
        p = (bnm::gtile)tiles + lane;
#pragma unroll
        for (int k = 0; k < PR_AHEAD; k++) q[k] = p[(size_t)k * 64];
    }
    // (the request for tile k + PR_AHEAD stays where tile k is taken: left to itself hipcc's scheduler, short of registers, sinks every request to
    // just before its use and the ring is one or two tiles deep)
    __device__ __forceinline__ bnm::v4i next() {
        const bnm::v4i a = q[0];
#pragma unroll
        for (int k = 0; k + 1 < PR_AHEAD; k++) q[k] = q[k + 1];
        __builtin_amdgcn_sched_barrier(0);
        q[PR_AHEAD - 1] = p[(size_t)PR_AHEAD * 64];
        __builtin_amdgcn_sched_barrier(0);
        p += 64;
        return a;
    }
};
// N = t - 1 columns.  Everything that indexes the state is unrolled, so that which columns live in LDS (elements below BN_LDS_ELEMS) and which in
// private memory is known statically, and NO private-memory access sits inside a loop that runs the tile ring: hipcc answers a mix of scratch and
// global accesses in flight -- or a branch around one -- with `s_waitcnt vmcnt(0)`, which drains the ring on every column and exposes the L2
// latency of every tile (round 5's form: 2 465 cycles per column of eight matrix instructions).  The upper columns are therefore fetched in ONE batch:
// before the rows' pass as matrix operands (kept for both half-passes), before / after the column update as words.  The rows on y are taken two at
// a time (two passes over the columns: four accumulators instead of eight leave the registers for the batch; the lower columns are read from LDS twice).
// BFORM: the y (elements 1..N) arrive, live and leave in operand form (lds_load_b): the fast path of the width-17 permutation.
template <int N, bool BFORM = false>
__device__ __forceinline__ void partial_rounds_mfma_impl(const St st, const bnm::v4i *Pt, const u32 *KR, const u32 *KU, int rp) {
    constexpr int NLO = N + 1 <= BN_LDS_ELEMS ? N : BN_LDS_ELEMS - 1;     // columns j whose element 1 + j lives in LDS
    constexpr int NHI = N - NLO, NHA = NHI ? NHI : 1;
    const int nb = rp / 4, nsb = (nb + 1) / 2;
    const bnm::Sh sh = bnm::sh_init();
    TileStream ts;
    __syncthreads();
    ts.start(Pt, st.lane);
    // x0 (S[0] came with the row of the layer before) stays in its LDS slot outside the rounds: the rows' pass and the columns need the registers
    // BFORM: the upper columns as the column update leaves them (operand form) stay in registers into the first rows' pass of the NEXT super-block
    // (the update's own operands are dead by then): that pass reads no private memory at all
    u32 yh[NHA][8];
    if constexpr (BFORM) {
#pragma unroll
        for (int q = 0; q < NHI; q++) lds_load(st, 1 + NLO + q, yh[q]);
    }
    for (int sb = 0; sb < nsb; sb++) {
        const int halves = nb - 2 * sb >= 2 ? 2 : 1;
        bnm::v4i zbA0[4], zbA1[4];                    // the first block's z operands, for the second block's rows and the column update
        bnm::v4i zb0[4], zb1[4];                      // the current block's: z_(i-3) .. z_i
#pragma unroll
        for (int s = 0; s < 4; s++) { zbA0[s] = bnm::v4i{ 0, 0, 0, 0 }; zbA1[s] = bnm::v4i{ 0, 0, 0, 0 }; }
        u32 pc[4][10];
        // the four rows' parts on y of one block; H = 1: the second block of a super-block (two instances: no branch inside the ring's straight line)
        auto rows = [&](auto Hc) {
            constexpr int H = decltype(Hc)::value;
            __syncthreads();
            // The upper columns as operands, in at most two batches of private-memory elements fetched just before their columns (all seven kept through a
            // pass do not fit beside the accumulators: hipcc spilled them, ~700 spill stores per wave).  The SECOND batch (columns SPL.., at most
            // BN_HI_BATCH of them) is still in its registers when the second pass begins: that pass takes it first, re-reads only the first batch,
            // and ends on the lower columns (mfma_partial_tables writes the tiles in this order).
            constexpr int HB2 = NHI < BN_HI_BATCH ? NHI : BN_HI_BATCH, SPL = NHI - HB2, HBA = HB2 ? HB2 : 1;
            static_assert(SPL <= HBA, "two batches of BN_HI_BATCH elements must cover the upper columns");
            bnm::v4i hb0[HBA], hb1[HBA];
            auto fetch = [&](int q0, int cnt) {
#pragma unroll
                for (int e = 0; e < HBA; e++)
                    if (e < cnt) {
                        if constexpr (BFORM) lds_load_b(st, 1 + NLO + q0 + e, hb0[e], hb1[e]);
                        else {
                            u32 y[8];
                            lds_load(st, 1 + NLO + q0 + e, y);
                            bnm::b_prep(y, hb0[e], hb1[e]);
                        }
                    }
            };
#pragma unroll
            for (int pass = 0; pass < 2; pass++) {
                bnm::v16i P0[2], P1[2];
                bool first = true;
                auto products = [&](const bnm::v4i &b0, const bnm::v4i &b1) {
#pragma unroll
                    for (int r = 0; r < 2; r++) {
                        const bnm::v4i a = ts.next();
                        if (first) bnm::mfma_first(a, b0, b1, P0[r], P1[r]);
                        else {
                            P0[r] = bnm::mfma(a, b0, P0[r]);
                            P1[r] = bnm::mfma(a, b1, P1[r]);
                        }
                    }
                    first = false;
                };
                auto lower = [&]() {
                    u32 yn[8];
                    if (NLO) lds_load(st, 1, yn);
#pragma unroll
                    for (int j = 0; j < NLO; j++) {
                        bnm::v4i b0, b1;
                        u32 y[8];
#pragma unroll
                        for (int l = 0; l < 8; l++) y[l] = yn[l];
                        if (j + 1 < NLO) lds_load(st, 2 + j, yn);         // the next column's words are on their way while this one's products run
                        if constexpr (BFORM) {
#pragma unroll
                            for (int q4 = 0; q4 < 4; q4++) { b0[q4] = (int)y[q4]; b1[q4] = (int)y[4 + q4]; }
                        } else bnm::b_prep(y, b0, b1);
                        products(b0, b1);
                    }
                };
                auto upper = [&](int q0, int cnt) {
#pragma unroll
                    for (int e = 0; e < HBA; e++)
                        if (e < cnt) products(hb0[e], hb1[e]);
                };
                auto carried = [&](int q0, int cnt) {                  // the upper columns the last column update left in registers
#pragma unroll
                    for (int q = 0; q < NHA; q++)
                        if (q >= q0 && q < q0 + cnt) {
                            bnm::v4i b0, b1;
#pragma unroll
                            for (int q4 = 0; q4 < 4; q4++) { b0[q4] = (int)yh[q][q4]; b1[q4] = (int)yh[q][4 + q4]; }
                            products(b0, b1);
                        }
                };
                constexpr bool CARRIED = BFORM && H == 0;
                if (pass == 0) {
                    lower();
                    if constexpr (CARRIED) carried(0, NHI);
                    else {
                        if (SPL) { fetch(0, SPL); upper(0, SPL); }
                        if (HB2) { fetch(SPL, HB2); upper(SPL, HB2); }
                    }
                } else {
                    if constexpr (CARRIED) { carried(SPL, HB2); carried(0, SPL); }
                    else {
                        if (HB2) upper(SPL, HB2);                      // (in registers since the first pass)
                        if (SPL) { fetch(0, SPL); upper(0, SPL); }
                    }
                    lower();
                }
                if constexpr (H == 1) {                               // the rows of the second block see the first block's z through cross terms of their own
#pragma unroll
                    for (int r = 0; r < 2; r++)
#pragma unroll
                        for (int s = 0; s < 4; s++) {
                            const bnm::v4i a = ts.next();
                            P0[r] = bnm::mfma(a, zbA0[s], P0[r]);
                            P1[r] = bnm::mfma(a, zbA1[s], P1[r]);
                        }
                }
#pragma unroll
                for (int r = 0; r < 2; r++) bnm::carry_pair(P0[r], P1[r], pc[2 * pass + r], sh);
            }
        };
        rows(std::integral_constant<int, 0>{});          // (outside the loop over the blocks: the carried columns must not be live around its back edge)
        for (int h = 0; h < halves; h++) {
            const int b = 2 * sb + h;
            if (h == 1) {
#pragma unroll
                for (int s = 0; s < 4; s++) { zbA0[s] = zb0[s]; zbA1[s] = zb1[s]; }
                rows(std::integral_constant<int, 1>{});
            }
            u32 x0[8];
            lds_load(st, 0, x0);
            // the four rounds, unrolled: round i's cross terms are i + 1 tiles (z_0 .. z_i of this block), its row's part pc[i] and its operand slot
            // are static -- no zero tiles multiplied, no operand or row shifted along
#pragma unroll
            for (int i = 0; i < 4; i++) {
                u32 k[8];
                load_const(KR, (size_t)(4 * b + i), k);               // (long before its use: the S-box hides it)
                pow5_lazy(x0);
                bnm::b_prep(x0, zb0[i], zb1[i]);
                bnm::v16i c0, c1;
#pragma unroll
                for (int s = 0; s <= i; s++) {
                    const bnm::v4i a = ts.next();
                    if (s == 0) bnm::mfma_first(a, zb0[0], zb1[0], c0, c1);
                    else {
                        c0 = bnm::mfma(a, zb0[s], c0);
                        c1 = bnm::mfma(a, zb1[s], c1);
                    }
                }
                u32 w[10];
                bnm::carry_pair(c0, c1, w, sh);
                bnm::add_pair(w, pc[i]);
                bnm::finish_words(w, k, x0);
            }
            lds_store(st, 0, x0);
        }
        // the columns, once per super-block: y_j + sum over its rounds of W z -- 1 + 8 tiles and one finish each (a last super-block of one block
        // has four zero tiles for the first block's operands, which are zero: ONE form of the column, mfma_partial_tables)
        auto column = [&](u32 y[8], int j) {
            u32 k[8];
            load_const(KU, (size_t)sb * N + j, k);                    // (asked for early: used after the products)
            bnm::v4i b0, b1;
            if constexpr (BFORM) {
#pragma unroll
                for (int q4 = 0; q4 < 4; q4++) { b0[q4] = (int)y[q4]; b1[q4] = (int)y[4 + q4]; }
            } else bnm::b_prep(y, b0, b1);
            bnm::v4i a = ts.next();
            bnm::v16i c0, c1;
            bnm::mfma_first(a, b0, b1, c0, c1);
#pragma unroll
            for (int s = 0; s < 4; s++) {
                a = ts.next();
                c0 = bnm::mfma(a, zbA0[s], c0);
                c1 = bnm::mfma(a, zbA1[s], c1);
            }
#pragma unroll
            for (int s = 0; s < 4; s++) {
                a = ts.next();
                c0 = bnm::mfma(a, zb0[s], c0);
                c1 = bnm::mfma(a, zb1[s], c1);
            }
            bnm::finish_row(c0, c1, k, y, sh);
            if constexpr (BFORM) {                                    // back to the form it is kept in
                bnm::v4i nb0, nb1;
                bnm::b_prep(y, nb0, nb1);
#pragma unroll
                for (int q4 = 0; q4 < 4; q4++) { y[q4] = (u32)nb0[q4]; y[4 + q4] = (u32)nb1[q4]; }
            }
        };
        if (halves == 1) {
#pragma unroll
            for (int s = 0; s < 4; s++) { zbA0[s] = bnm::v4i{ 0, 0, 0, 0 }; zbA1[s] = bnm::v4i{ 0, 0, 0, 0 }; }
        }
        __syncthreads();
        if (NLO) {                                                    // the lower columns: a loop (LDS takes a run-time index; the ring turns by three tiles per column)
            u32 yn[8];
            lds_load(st, 1, yn);
#pragma unroll 1
            for (int j = 0; j < NLO; j++) {
                u32 y[8];
#pragma unroll
                for (int l = 0; l < 8; l++) y[l] = yn[l];
                if (j + 1 < NLO) lds_load(st, 2 + j, yn);
                column(y, j);
                lds_store(st, 1 + j, y);
            }
        }
        {                                                             // the upper columns: one batch in, one batch out (and kept: see above)
#pragma unroll
            for (int q = 0; q < NHI; q++) lds_load(st, 1 + NLO + q, yh[q]);
#pragma unroll
            for (int q = 0; q < NHI; q++) column(yh[q], NLO + q);
#pragma unroll
            for (int q = 0; q < NHI; q++) lds_store(st, 1 + NLO + q, yh[q]);
        }
    }
}
template <int N>
__device__ __noinline__ void partial_rounds_mfma_n(const St st, const bnm::v4i *Pt, const u32 *KR, const u32 *KU, int rp) { partial_rounds_mfma_impl<N>(st, Pt, KR, KU, rp); }
// the widths 5..16 of bn_perm (N = t - 1)
__device__ __forceinline__ void partial_rounds_mfma(const St st, const PermArgs &A) {
    switch (A.t - 1) {
    case 4: partial_rounds_mfma_n<4>(st, A.Pt, A.KR, A.KU, A.rp); break;
    case 5: partial_rounds_mfma_n<5>(st, A.Pt, A.KR, A.KU, A.rp); break;
    case 6: partial_rounds_mfma_n<6>(st, A.Pt, A.KR, A.KU, A.rp); break;
    case 7: partial_rounds_mfma_n<7>(st, A.Pt, A.KR, A.KU, A.rp); break;
    case 8: partial_rounds_mfma_n<8>(st, A.Pt, A.KR, A.KU, A.rp); break;
    case 9: partial_rounds_mfma_n<9>(st, A.Pt, A.KR, A.KU, A.rp); break;
    case 10: partial_rounds_mfma_n<10>(st, A.Pt, A.KR, A.KU, A.rp); break;
    case 11: partial_rounds_mfma_n<11>(st, A.Pt, A.KR, A.KU, A.rp); break;
    case 12: partial_rounds_mfma_n<12>(st, A.Pt, A.KR, A.KU, A.rp); break;
    case 13: partial_rounds_mfma_n<13>(st, A.Pt, A.KR, A.KU, A.rp); break;
    case 14: partial_rounds_mfma_n<14>(st, A.Pt, A.KR, A.KU, A.rp); break;
    default: partial_rounds_mfma_n<15>(st, A.Pt, A.KR, A.KU, A.rp); break;
    }
}

// Widths up to BN_SMALL_T: the permutation round by round (poseidon.circom:22-44 as written) with the state, the layer's T x T tiles and the operands in
// REGISTERS: every round adds its constants (they arrive with the previous layer's rows), takes the S-box (all elements / element 0) and multiplies by the
// same matrix.  Two tile sets (which columns carry the S-box's 2^-20), swapped twice per permutation; nothing streams, nothing goes through LDS between
// the rounds.  The blocked pipeline is built for seventeen elements: at three its phases are a few matrix instructions each and the wave spends its time
// between them (a width-3 permutation took 1.08 M cycles per wave at an UNCAPPED 2.38 GHz, twice its S-boxes' issue time).
template <int T>
__device__ __noinline__ void perm_small(const St st, const PermArgs &A) {
    u32 x[T][8];
#pragma unroll
    for (int j = 0; j < T; j++) {
        u32 c[8];
        lds_load(st, j, x[j]);
        load_const(A.Cd, (size_t)j, c);
        add_lazy(x[j], c);
    }
    const bnm::Sh sh = bnm::sh_init();
    const int R = N_ROUNDS_F + A.rp;
    bnm::v4i tl[T * T];
    bnm::gtile tp = (bnm::gtile)A.St + st.lane;
#pragma unroll
    for (int q = 0; q < T * T; q++) tl[q] = tp[(size_t)q * 64];
#pragma unroll 1
    for (int r = 0; r < R; r++) {
        const bool full = r < N_ROUNDS_F / 2 || r >= N_ROUNDS_F / 2 + A.rp;
        if (r == N_ROUNDS_F / 2 || r == N_ROUNDS_F / 2 + A.rp) {          // the other tile set from here on
            const size_t off = (size_t)(r == N_ROUNDS_F / 2 ? T * T : 0) * 64;
#pragma unroll
            for (int q = 0; q < T * T; q++) tl[q] = tp[off + (size_t)q * 64];
        }
        u32 k[T][8];
#pragma unroll
        for (int i = 0; i < T; i++) load_const(A.SK, (size_t)r * T + i, k[i]);      // (asked for ahead of the S-boxes, which hide them)
        pow5_lazy(x[0]);
        if (full) {
#pragma unroll
            for (int j = 1; j < T; j++) pow5_lazy(x[j]);
        }
        bnm::v4i B0[T], B1[T];
#pragma unroll
        for (int j = 0; j < T; j++) bnm::b_prep(x[j], B0[j], B1[j]);
        const int rows = r == R - 1 && A.nout1 ? 1 : T;
#pragma unroll
        for (int i = 0; i < T; i++) {
            if (i < rows) {
                bnm::v16i a0, a1;
                bnm::mfma_first(tl[i * T], B0[0], B1[0], a0, a1);
#pragma unroll
                for (int j = 1; j < T; j++) { a0 = bnm::mfma(tl[i * T + j], B0[j], a0); a1 = bnm::mfma(tl[i * T + j], B1[j], a1); }
                bnm::finish_row(a0, a1, k[i], x[i], sh);
            }
        }
    }
#pragma unroll
    for (int j = 0; j < T; j++) lds_store(st, j, x[j]);
}

// the permutation of the t elements of the state, in place: one pipeline per width
__device__ __noinline__ void bn_perm(const St st, const PermArgs &A) {
    const int t = A.t;
    if (t <= BN_SMALL_T) {
        if (t == 2) perm_small<2>(st, A);
        else if (t == 3) perm_small<3>(st, A);
        else perm_small<4>(st, A);
        return;
    }
    if (t == 17) {
        // The width of the arity-16 trees (config 4) in ONE function body: every phase called out of line saves and restores the callee-saved
        // half of its 256 registers in private memory (92-112 words per lane and call, ~480 KB per wave and permutation -- a third of the
        // kernel's private-memory traffic, which the chip pays for in power: tools/power_probe.py).  One copy of each phase: the partial rounds
        // and the closing layer sit at the top of the fifth full round (rp = 68 = 17 blocks of four, nothing left over).
        // The S-boxes of rounds 1-3 and 5-7 ride on the rows of the layer before them, round 4's on the closing layer's rows (its element 0, which comes
        // out of the partial rounds, alone afterwards); only round 0's is a pass of its own.  Two copies of the wide layer (with / without the S-box).
        // A.plain (leaf kernel): elements 1..16 went through round 0's S-box where they were absorbed, as plain integers (plain_sbox_store): only element 0 is left,
        // and the first layer reads its own copy of the tiles
        if (A.plain) { u32 x[8], c[8]; lds_load(st, 0, x); load_const(A.C8, 0, c); add_lazy(x, c); pow5_lazy(x); lds_store(st, 0, x); }
        else sbox_lazy_impl(st, 17, A.C8);
        for (int r = 0; r < 8; r++) {                                         // (one copy of each form of the layer)
            const bnm::v4i *Mt = r == 0 && A.plain ? A.Mt0 : A.Mt;
            const u32 *MK = r == 0 && A.plain ? A.MK0 : A.MK + (size_t)r * 17 * 8;
            if (r == 3) dense_mfma_impl<17, false, true>(st, Mt, MK, 0);    // its rows 1..16: the partial rounds' y, in operand form
            else if (r == 7) dense_mfma_impl<17>(st, Mt, MK, 0, A.nout1 ? 1 : 17);
            else dense_mfma_impl<17, true>(st, Mt, MK, 0);
            if (r == 3) {
                partial_rounds_mfma_impl<16, true>(st, A.Pt, A.KR, A.KU, A.rp);
                dense_mfma_impl<16, true, false, true>(st, A.Dt, A.DK, 1);  // diag(1, Mh^RP) on the y as they are, then round 4's S-box on elements 1..16
                u32 x[8]; lds_load(st, 0, x); pow5_lazy(x); lds_store(st, 0, x);
            }
        }
        return;
    }
    // widths 5..16: between the layers the state is lazy (< 2^255), every constant but the first round's arrives with a layer's rows
    for (int r = 0; r < 4; r++) {
        sbox_lazy(st, t, r == 0 ? A.C8 : nullptr);
        dense_mfma(st, A.Mt, A.MK + (size_t)r * t * 8, t, 0);
    }
    partial_rounds_mfma(st, A);
    if (A.rp % 4) {                                  // the rounds left over, one by one on canonical values
        canon_state(st, t);
        partial_rounds(st, A, A.rp & ~3);
        u32 x[8], c[8];
        lds_load(st, 0, x);
        load_const(A.C8, (size_t)4 * t, c);
        bn::fr_add(x, c);
        lds_store(st, 0, x);
    }
    dense_mfma(st, A.Dt, A.DK, t - 1, 1);            // diag(1, Mh^RP)
    for (int r = 4; r < 8; r++) {
        sbox_lazy(st, t, nullptr);
        dense_mfma(st, A.Mt, A.MK + (size_t)r * t * 8, t, 0, r == 7 && A.nout1 ? 1 : 17);
    }
}

__device__ __forceinline__ void to_mont_store(const St st, int j, const u64 w[4]) {
    u32 x[8], r2[8], o[8];
#pragma unroll
    for (int k = 0; k < 4; k++) { x[2 * k] = (u32)w[k]; x[2 * k + 1] = (u32)(w[k] >> 32); }
#pragma unroll
    for (int l = 0; l < 8; l++) r2[l] = bn::r2_limb(l);
    bn::fr_mul(o, x, r2);                            // frm_toMontgomery: x * 2^256 mod r (x < 2^256)
    lds_store(st, j, o);
}
// the same input for a permutation with A.plain: round 0's S-box on the PLAIN integer x + c (c = the round constant as a plain integer; x < 2^192: no reduction,
// no conversion product); bn29::pow5's result is then 2^-1280 times what the state's form would give, which the first layer's own tiles take back
__device__ __forceinline__ void plain_sbox_store(const St st, int j, const u64 w[4], const u32 *C0p) {
    u32 x[8], c[8];
#pragma unroll
    for (int k = 0; k < 4; k++) { x[2 * k] = (u32)w[k]; x[2 * k + 1] = (u32)(w[k] >> 32); }
    load_const(C0p, (size_t)j, c);
    bnm::add_chain8(x, c);
    pow5_lazy(x);
    lds_store(st, j, x);
}
__device__ __forceinline__ void zero_store(const St st, int j) {
    const u32 z[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };
    lds_store(st, j, z);
}
__device__ __forceinline__ void digest_out(const St st, int j, u64 *o) {
    u32 x[8];
    lds_load(st, j, x);
    bnm::canon(x);                                   // the matrix-core pipeline leaves lazy representatives
#pragma unroll
    for (int k = 0; k < 4; k++) o[k] = (u64)x[2 * k] | ((u64)x[2 * k + 1] << 32);
}

// leaf digests (merklehash_bn128_worker.js:42-98): one row per lane
__global__ void __launch_bounds__(BN_THREADS) __attribute__((amdgpu_waves_per_eu(2))) bn_linear_hash_kernel(const u64 *__restrict__ in, u64 width, u64 height, int arity, int custom,
                                                                    PermArgs full, PermArgs last, u64 *__restrict__ out) {
    extern __shared__ u32 S[];
    const int lane = threadIdx.x % BN_BLOCK, wv = threadIdx.x / BN_BLOCK, tmax = arity + 1;
    u32 hi_arr[(17 - BN_LDS_ELEMS) * 8];
    const St st = { (lds_u32)S + wv * lds_words(tmax), (priv_u32)hi_arr, tmax, lane };
    const u64 row0 = ((u64)blockIdx.x * BN_WG_WAVES + wv) * BN_BLOCK + lane;
    const bool live = row0 < height;
    const u64 *v = in + (live ? row0 : height - 1) * width;
    if (width <= 4) {                                // :45-50: up to four words taken as one 256-bit integer
        u64 w[4] = { 0, 0, 0, 0 };
        for (u64 k = 0; k < width; k++) w[k] = v[k];
        to_mont_store(st, 0, w);
    } else {
        zero_store(st, 0);             // st = 0
        const u64 nEl = (width + 2) / 3;             // 3 Goldilocks words per field element (:54-67)
        u64 e = 0;
        while (e < nEl) {
            const u64 n = nEl - e < (u64)arity ? nEl - e : (u64)arity;
            const bool plain = full.plain && (n == (u64)arity || custom);      // the chunk goes to `full`, whose first S-box rides on the absorb
            for (u64 k = 0; k < n; k++) {
                u64 w[4] = { 0, 0, 0, 0 };
                for (int q = 0; q < 3; q++) { const u64 idx = 3 * (e + k) + q; if (idx < width) w[q] = v[idx]; }
                if (plain) plain_sbox_store(st, 1 + (int)k, w, full.C0p);
                else to_mont_store(st, 1 + (int)k, w);
            }
            if (n == (u64)arity) bn_perm(st, full);
            else if (custom) {                       // :87-93: zero-pad the last chunk to `arity` inputs
                const u64 z[4] = { 0, 0, 0, 0 };
                for (u64 k = n; k < (u64)arity; k++) { if (plain) plain_sbox_store(st, 1 + (int)k, z, full.C0p); else zero_store(st, 1 + (int)k); }
                bn_perm(st, full);
            } else bn_perm(st, last);      // :85-86: t = nLast + 1
            e += n;
        }
    }
    if (live) digest_out(st, 0, out + 4 * row0);
}

// parents (merklehash_bn128_worker.js:104-144): out[i] = Poseidon(0; in[arity*i .. arity*i+arity-1])[0]
__global__ void __launch_bounds__(BN_THREADS) __attribute__((amdgpu_waves_per_eu(2))) bn_merkle_level_kernel(const u64 *__restrict__ in, u64 nOps, int arity, PermArgs full, u64 *__restrict__ out) {
    extern __shared__ u32 S[];
    const int lane = threadIdx.x % BN_BLOCK, wv = threadIdx.x / BN_BLOCK, tmax = arity + 1;
    u32 hi_arr[(17 - BN_LDS_ELEMS) * 8];
    const St st = { (lds_u32)S + wv * lds_words(tmax), (priv_u32)hi_arr, tmax, lane };
    const u64 i0 = ((u64)blockIdx.x * BN_WG_WAVES + wv) * BN_BLOCK + lane;
    const bool live = i0 < nOps;
    const u64 *v = in + (live ? i0 : nOps - 1) * (u64)arity * 4;
    zero_store(st, 0);
    for (int k = 0; k < arity; k++) {                // children are already in Montgomery form
        u32 x[8];
#pragma unroll
        for (int q = 0; q < 4; q++) { const u64 w = v[4 * k + q]; x[2 * q] = (u32)w; x[2 * q + 1] = (u32)(w >> 32); }
        lds_store(st, 1 + k, x);
    }
    bn_perm(st, full);
    if (live) digest_out(st, 0, out + 4 * i0);
}

// circomlibjs poseidon(inputs, initState, nOut): normal-form words in and out (transcript, verification, tests)
__global__ void __launch_bounds__(BN_THREADS) __attribute__((amdgpu_waves_per_eu(2))) bn_poseidon_kernel(const u64 *__restrict__ in, const u64 *__restrict__ init, u64 count, int nIn, int nOut,
                                                                 PermArgs full, u64 *__restrict__ out) {
    extern __shared__ u32 S[];
    const int lane = threadIdx.x % BN_BLOCK, wv = threadIdx.x / BN_BLOCK, tmax = nIn + 1;
    u32 hi_arr[(17 - BN_LDS_ELEMS) * 8];
    const St st = { (lds_u32)S + wv * lds_words(tmax), (priv_u32)hi_arr, tmax, lane };
    const u64 i0 = ((u64)blockIdx.x * BN_WG_WAVES + wv) * BN_BLOCK + lane;
    const bool live = i0 < count;
    const u64 i = live ? i0 : count - 1;
    u64 w[4] = { 0, 0, 0, 0 };
    if (init) for (int q = 0; q < 4; q++) w[q] = init[4 * i + q];
    to_mont_store(st, 0, w);
    for (int k = 0; k < nIn; k++) {
        for (int q = 0; q < 4; q++) w[q] = in[(i * nIn + k) * 4 + q];
        to_mont_store(st, 1 + k, w);
    }
    bn_perm(st, full);
    if (!live) return;
    for (int k = 0; k < nOut; k++) {                 // out of Montgomery form: multiply by 1
        u32 x[8], one[8] = { 1, 0, 0, 0, 0, 0, 0, 0 }, o[8];
        lds_load(st, k, x);
        bn::fr_mul(o, x, one);
        for (int q = 0; q < 4; q++) out[(i * nOut + k) * 4 + q] = (u64)o[2 * q] | ((u64)o[2 * q + 1] << 32);
    }
}

// A chain of dependent permutations (transcript.bn128.js:56-66 absorbing a list: each full block of nIn elements is permuted
// with the previous output 0 as state element 0).  One permutation per lane leaves such a chain at one wave-alone
// permutation (~3 ms) per block; here the wave shares each permutation and runs the round function as poseidon.circom:22-44
// states it: lane (l, s), l < t, s < 3, holds state element l (the three copies stay equal); constants and S-boxes in
// parallel (element 0 alone in the partial rounds); of row l of the dense MDS product, lane (l, s) accumulates the terms
// j = s, s+3, ... unreduced in 17 limbs, the three partial sums are added through LDS and reduced once.  Normal-form words
// in and out.  Measured at t = 17: 3.1 ms per permutation for a call per block, 0.76 ms with one lane per row (issue-bound
// on its 17 multiply-accumulates per round; requesting operands a term ahead changes nothing), 0.49 ms with the row split.
constexpr int CHAIN_SUB = 3;
// One permutation of that form, a device function so that a kernel can run permutations of DIFFERENT widths one after the other (a Merkle
// path: the sponge's full chunks, its short last chunk, the levels): lane (l, sub) of the CHAIN_SUB*t active ones enters and leaves with
// state element l in x (Montgomery form); A supplies Cd, M and rp of width t.  sh: 17*8 words, part: CHAIN_SUB*17*17 words of the wave's LDS.
__device__ __forceinline__ void chain_perm(u32 (&x)[8], const PermArgs &A, int t, int l, int sub, bool act, lds_u32 sh, lds_u32 part) {
    const int nRounds = N_ROUNDS_F + A.rp;
    for (int r = 0; r < nRounds; r++) {
        u32 c[8];
        load_const(A.Cd, (size_t)r * t + l, c);
        bn::fr_add(x, c);
        const bool full = r < N_ROUNDS_F / 2 || r >= N_ROUNDS_F / 2 + A.rp;
        if (full || l == 0) pow5(x);
        if (act && sub == 0) {
#pragma unroll
            for (int i = 0; i < 8; i++) sh[l * 8 + i] = x[i];
        }
        __builtin_amdgcn_s_waitcnt(0xC07F);          // lgkmcnt(0): this wave's LDS writes have landed
        __builtin_amdgcn_wave_barrier();
        u32 acc[17];
#pragma unroll
        for (int i = 0; i < 17; i++) acc[i] = 0;
        for (int j = sub; j < t; j += CHAIN_SUB) {
            u32 y[8], m[8];
#pragma unroll
            for (int i = 0; i < 8; i++) y[i] = sh[j * 8 + i];
            load_const(A.M, (size_t)l * t + j, m);
            bn::mac17(acc, y, m);
        }
        if (act) {
#pragma unroll
            for (int i = 0; i < 17; i++) part[(sub * 17 + l) * 17 + i] = acc[i];
        }
        __builtin_amdgcn_s_waitcnt(0xC07F);
        __builtin_amdgcn_wave_barrier();
        // every copy adds the three partial sums (together at most t products: they fit the 17 limbs as one row did)
#pragma unroll
        for (int i = 0; i < 17; i++) acc[i] = part[l * 17 + i];
#pragma unroll
        for (int q = 1; q < CHAIN_SUB; q++) {
            u64 cy = 0;
#pragma unroll
            for (int i = 0; i < 17; i++) {
                const u64 v = (u64)acc[i] + part[(q * 17 + l) * 17 + i] + cy;
                acc[i] = (u32)v; cy = v >> 32;
            }
        }
        __builtin_amdgcn_wave_barrier();
        bn::redc17(x, acc);
    }
}

// One workgroup (one wave) per chain: chain g reads nBlocks*nIn elements at blocks + g*nBlocks*nIn*4, state element 0 from
// init + 4g (zero if init is null), and writes its first nOut outputs at out + g*nOut*4 -- with nBlocks = 1 this is a batch of
// independent permutations, the faster form while there are fewer of them than SIMDs to give a whole wave each.
__global__ void __launch_bounds__(64) bn_sponge_chain_kernel(const u64 *__restrict__ blocks, u64 nBlocks, int nIn, const u64 *__restrict__ init,
                                                            PermArgs A, int nOut, int mont, u64 *__restrict__ out) {
    __shared__ u32 sh[17 * 8];
    __shared__ u32 part[CHAIN_SUB * 17 * 17];
    const int t = nIn + 1, lane = threadIdx.x;
    blocks += (u64)blockIdx.x * nBlocks * nIn * 4;
    out += (u64)blockIdx.x * nOut * 4;
    const u64 zero4[4] = { 0, 0, 0, 0 };
    if (init) init += (u64)blockIdx.x * 4;
    const bool act = lane < CHAIN_SUB * t;
    const int sub = act ? lane / t : 0, l = act ? lane - sub * t : 0;
    u32 r2[8], x[8];
#pragma unroll
    for (int i = 0; i < 8; i++) r2[i] = bn::r2_limb(i);
    auto load_mont = [&](const u64 *w) {             // frm_toMontgomery; mont: the words are in Montgomery form already (tree nodes)
        u32 v[8];
#pragma unroll
        for (int q = 0; q < 4; q++) { v[2 * q] = (u32)w[q]; v[2 * q + 1] = (u32)(w[q] >> 32); }
        if (mont) {
#pragma unroll
            for (int i = 0; i < 8; i++) x[i] = v[i];
        } else bn::fr_mul(x, v, r2);
    };
    if (l == 0) load_mont(init ? init : zero4);
    for (u64 b = 0; b < nBlocks; b++) {
        if (l > 0) load_mont(blocks + (b * nIn + (l - 1)) * 4);
        chain_perm(x, A, t, l, sub, act, (lds_u32)sh, (lds_u32)part);
    }
    if (!act || sub != 0 || l >= nOut) return;
    u32 one[8] = { 1, 0, 0, 0, 0, 0, 0, 0 }, o[8];
    if (mont) {
#pragma unroll
        for (int i = 0; i < 8; i++) o[i] = x[i];
    } else bn::fr_mul(o, x, one);                    // out of Montgomery form
#pragma unroll
    for (int q = 0; q < 4; q++) out[l * 4 + q] = (u64)o[2 * q] | ((u64)o[2 * q + 1] << 32);
}

// MerkleHash.calculateRootFromGroupProof (merklehash_bn128_p.js:184-232, LinearHashBN.hash linearhash.bn128.js:13-59) for a batch of openings,
// the whole path of one opening in one wave: a verifier's batch is queries x trees, fewer chains than the chip has SIMDs, and every
// permutation of a path waits for the one before it -- the shape of the chain kernel above, with the width changing from step to step.
// Steps: the sponge over the row's elements (3 Goldilocks words packed per element; full chunks at t = arity+1 carrying output 0 as state
// element 0, a short last chunk at t = nLast+1 through `last`, or zero-padded when custom), then one permutation per level at t = arity+1
// over the level's siblings with the running value at position idx & (arity-1) (whatever the proof holds there is not read) and state 0.
// Between two steps the running value is lane 0's x (lane 0 is (l, sub) = (0, 0) at every width), read by every lane as a wave-uniform value.
// vals: nIdx x width words; sib: nIdx x levels x arity x 4 words, normal form (any value < 2^256: reduced by the conversion) or, sibMont,
// Montgomery words as tree.nodes holds them; roots: nIdx x 4 words, normal form.
__global__ void __launch_bounds__(64) bn_path_roots_kernel(const u64 *__restrict__ vals, const u64 *__restrict__ sib, const u64 *__restrict__ idxs,
                                                          u64 width, int levels, int arity, int abits, int custom, int sibMont,
                                                          PermArgs full, PermArgs last, u64 *__restrict__ roots) {
    __shared__ u32 sh[17 * 8];
    __shared__ u32 part[CHAIN_SUB * 17 * 17];
    const int lane = threadIdx.x;
    vals += (u64)blockIdx.x * width;
    sib += (u64)blockIdx.x * (u64)levels * arity * 4;
    u64 pos = idxs[blockIdx.x];
    u32 r2[8], x[8];
    const u32 one[8] = { 1, 0, 0, 0, 0, 0, 0, 0 };
#pragma unroll
    for (int i = 0; i < 8; i++) { r2[i] = bn::r2_limb(i); x[i] = 0; }
    const u64 nEl = (width + 2) / 3;
    auto load_elem = [&](u64 e) {                    // linearhash.bn128.js:27-38: x + y 2^64 + z 2^128 (< r: the % is the identity), to Montgomery form
        u32 v[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };
        for (int q = 0; q < 3; q++) { const u64 k = 3 * e + q; if (k < width) { const u64 w = vals[k]; v[2 * q] = (u32)w; v[2 * q + 1] = (u32)(w >> 32); } }
        bn::fr_mul(x, v, r2);
    };
    if (nEl == 1) load_elem(0);                      // :41: one element is its own hash (none: 0)
    const int nChunks = nEl < 2 ? 0 : (int)((nEl + (u64)arity - 1) / (u64)arity);
    for (int s = 0; s < nChunks + levels; s++) {
        u32 run[8];                                  // the value so far: the sponge's state element 0, a level's own child
#pragma unroll
        for (int i = 0; i < 8; i++) run[i] = (u32)__builtin_amdgcn_readlane((int)x[i], 0);
        const bool level = s >= nChunks;
        const u64 e0 = (u64)s * arity;
        const int n = level || nEl - e0 >= (u64)arity ? arity : (int)(nEl - e0);
        const bool shortLast = n < arity && !custom;
        const int t = shortLast ? n + 1 : arity + 1;
        const bool act = lane < CHAIN_SUB * t;
        const int sub = act ? lane / t : 0, l = act ? lane - sub * t : 0;
        const int cur = (int)(pos & (u64)(arity - 1));
#pragma unroll
        for (int i = 0; i < 8; i++) x[i] = 0;        // a level's state element 0; the zero padding of a custom last chunk
        if (!level) {
            if (l == 0) {
#pragma unroll
                for (int i = 0; i < 8; i++) x[i] = run[i];
            } else if (l - 1 < n) load_elem(e0 + (u64)(l - 1));
        } else if (l > 0) {
            if (l - 1 == cur) {
#pragma unroll
                for (int i = 0; i < 8; i++) x[i] = run[i];
            } else {
                const u64 *w = sib + ((u64)(s - nChunks) * arity + (u64)(l - 1)) * 4;
                u32 v[8], m[8];
#pragma unroll
                for (int q = 0; q < 4; q++) { v[2 * q] = (u32)w[q]; v[2 * q + 1] = (u32)(w[q] >> 32); }
                bn::fr_mul(m, v, r2);                // v 2^256 mod r, canonical for every v < 2^256 (merklehash_bn128_p.js:218: % R)
                if (sibMont) bn::fr_mul(x, m, one);  // v was the Montgomery word already: back to it, reduced
                else {
#pragma unroll
                    for (int i = 0; i < 8; i++) x[i] = m[i];
                }
            }
        }
        if (level) pos >>= abits;
        if (shortLast) chain_perm(x, last, t, l, sub, act, (lds_u32)sh, (lds_u32)part);
        else chain_perm(x, full, t, l, sub, act, (lds_u32)sh, (lds_u32)part);
    }
    if (lane != 0) return;
    u32 o[8];
    bn::fr_mul(o, x, one);                           // out of Montgomery form
#pragma unroll
    for (int q = 0; q < 4; q++) roots[(u64)blockIdx.x * 4 + q] = (u64)o[2 * q] | ((u64)o[2 * q + 1] << 32);
}

// Montgomery <-> normal form of n elements (frm_toMontgomery / F.toObject)
__global__ void bn_convert_kernel(const u64 *__restrict__ in, u64 n, int toMont, u64 *__restrict__ out) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    u32 x[8], k[8], o[8];
    for (int q = 0; q < 4; q++) { x[2 * q] = (u32)in[4 * i + q]; x[2 * q + 1] = (u32)(in[4 * i + q] >> 32); }
    for (int l = 0; l < 8; l++) k[l] = toMont ? bn::r2_limb(l) : (l == 0 ? 1u : 0u);
    bn::fr_mul(o, x, k);
    for (int q = 0; q < 4; q++) out[4 * i + q] = (u64)o[2 * q] | ((u64)o[2 * q + 1] << 32);
}

// A batch of openings (fri.js:83-105 opens every tree at every query): block q gathers row idxs[q] and, per level, the `arity` nodes of its group
// (Montgomery words as stored; nodes beyond the level's count read as zero, merklehash_bn128_p.js:165-170) into out[q] = [width values | levels x arity x 4 words]
struct BnLevels { u64 off[40], n[40]; u32 levels; };
__global__ void bn_group_proofs_kernel(const u64 *__restrict__ elems, const u64 *__restrict__ nodes, u64 width, int arity, int abits,
                                       const u64 *__restrict__ idxs, BnLevels L, u64 *__restrict__ out) {
    const u64 stride = width + (u64)L.levels * arity * 4;
    u64 *o = out + blockIdx.x * stride;
    const u64 idx = idxs[blockIdx.x];
    for (u64 c = threadIdx.x; c < width; c += blockDim.x) o[c] = elems[idx * width + c];
    u64 id = idx;
    for (u32 l = 0; l < L.levels; l++) {
        const u64 si = id ^ (id & (u64)(arity - 1));
        for (u32 k = threadIdx.x; k < (u32)arity * 4; k += blockDim.x)
            o[width + ((u64)l * arity) * 4 + k] = si + k / 4 < L.n[l] ? nodes[(L.off[l] + si) * 4 + k] : 0;
        id >>= abits;
    }
}

size_t lds_bytes(int tmax) { return (size_t)lds_words(tmax) * 4 * BN_WG_WAVES; }     // the elements above BN_LDS_ELEMS live in private memory

// plainInputs: the leaf kernel's absorb S-boxes elements 1..t-1 as plain integers (width 17 only); firstOnly: the caller reads element 0 alone
PermArgs perm_args(const Params *P, bool plainInputs = false, bool firstOnly = false) {
    PermArgs a;
    a.C8 = P->C8; a.M = P->M; a.S = P->S; a.V = P->V; a.W = P->W; a.Cd = P->Cd; a.t = P->t; a.rp = P->rp;
    a.Mt = P->Mt; a.Dt = P->Dt; a.Pt = P->Pt; a.MK = P->MK; a.DK = P->DK; a.KR = P->KR; a.KU = P->KU;
    memcpy(a.m00, P->m00, 32);
    a.Mt0 = P->Mt0; a.MK0 = P->MK0; a.C0p = P->C0p;
    a.St = P->St; a.SK = P->SK;
    a.plain = plainInputs && P->t == 17 ? 1 : 0;
    a.nout1 = firstOnly ? 1 : 0;
    return a;
}

template <typename K>
int set_lds_attr(K kernel, size_t bytes) {
    HIP_TRY(hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    return PIL2GL_OK;
}

int check_arity(uint32_t arity) {
    if (arity < 2 || arity > 16 || (arity & (arity - 1))) return fail(PIL2GL_EINVAL, "arity must be 2, 4, 8 or 16 (got %u)", arity);
    return PIL2GL_OK;
}

}  // namespace

extern "C" {

uint64_t pil2gl_bn128_merkle_num_nodes(uint64_t height, uint32_t arity) {      // merklehash_bn128_p.js:31-45, in nodes
    if (height == 0 || arity < 2) return 0;
    uint64_t n = height, nextN = (n - 1) / arity + 1, acc = nextN * arity;
    while (n > 1) {
        n = nextN;
        nextN = (n - 1) / arity + 1;
        acc += n > 1 ? nextN * arity : 1;
    }
    return acc;
}

int pil2gl_bn128_linear_hash_rows_dev(const uint64_t *in, uint64_t width, uint64_t height, uint32_t arity, int custom, uint64_t *out, void *stream) {
    P2_TRY(ensure_init());
    if (height == 0) return PIL2GL_OK;
    P2_TRY(check_arity(arity));
    if (!out || (!in && width)) return fail(PIL2GL_EINVAL, "null buffer");
    const Params *pf, *pl;
    P2_TRY(get_params((int)arity + 1, &pf));
    pl = pf;
    const uint64_t nEl = (width + 2) / 3, nLast = nEl % arity;
    if (width > 4 && !custom && nLast) P2_TRY(get_params((int)nLast + 1, &pl));
    const size_t lds = lds_bytes((int)arity + 1);
    const uint64_t blocks = (height + BN_THREADS - 1) / BN_THREADS;
    if (blocks > 0x7fffffffull) return fail(PIL2GL_EINVAL, "grid too large");
    P2_TRY(set_lds_attr(bn_linear_hash_kernel, lds));
    bn_linear_hash_kernel<<<(unsigned)blocks, BN_THREADS, lds, as_stream(stream)>>>(in, width, height, (int)arity, custom ? 1 : 0, perm_args(pf, true, true), perm_args(pl, false, true), out);
    KERNEL_CHECK();
    return PIL2GL_OK;
}

int pil2gl_bn128_merkelize_level_dev(const uint64_t *in, uint64_t nOps, uint32_t arity, uint64_t *out, void *stream) {
    P2_TRY(ensure_init());
    if (nOps == 0) return PIL2GL_OK;
    P2_TRY(check_arity(arity));
    if (!in || !out) return fail(PIL2GL_EINVAL, "null buffer");
    const Params *pf;
    P2_TRY(get_params((int)arity + 1, &pf));
    const size_t lds = lds_bytes((int)arity + 1);
    const uint64_t blocks = (nOps + BN_THREADS - 1) / BN_THREADS;
    if (blocks > 0x7fffffffull) return fail(PIL2GL_EINVAL, "grid too large");
    if ((long)nOps <= WAVE_PER_PERM_MAX) {           // the levels near the root: a wave per parent
        bn_sponge_chain_kernel<<<(unsigned)nOps, 64, 0, as_stream(stream)>>>(in, 1, (int)arity, nullptr, perm_args(pf), 1, 1, out);
        KERNEL_CHECK();
        return PIL2GL_OK;
    }
    P2_TRY(set_lds_attr(bn_merkle_level_kernel, lds));
    bn_merkle_level_kernel<<<(unsigned)blocks, BN_THREADS, lds, as_stream(stream)>>>(in, nOps, (int)arity, perm_args(pf, false, true), out);
    KERNEL_CHECK();
    return PIL2GL_OK;
}

int pil2gl_bn128_merkelize_dev(const uint64_t *elems, uint64_t width, uint64_t height, uint32_t arity, int custom, uint64_t *nodes, void *stream) {
    P2_TRY(ensure_init());
    if (height == 0) return fail(PIL2GL_EINVAL, "height must be > 0");
    P2_TRY(check_arity(arity));
    if (!nodes || (!elems && width)) return fail(PIL2GL_EINVAL, "null buffer");
    hipStream_t st = as_stream(stream);
    // merklehash_bn128_p.js:51: nodes is a fresh (zeroed) array; the zero padding of short levels relies on it
    HIP_TRY(hipMemsetAsync(nodes, 0, pil2gl_bn128_merkle_num_nodes(height, arity) * 32, st));
    P2_TRY(pil2gl_bn128_linear_hash_rows_dev(elems, width, height, arity, custom, nodes, stream));
    uint64_t pIn = 0, n = height, nextN = (n - 1) / arity + 1, pOut = pIn + nextN * arity * 4;   // :89-101, in u64 words
    while (n > 1) {
        P2_TRY(pil2gl_bn128_merkelize_level_dev(nodes + pIn, nextN, arity, nodes + pOut, stream));
        n = nextN;
        nextN = (n - 1) / arity + 1;
        pIn = pOut;
        pOut = pIn + nextN * arity * 4;
    }
    return PIL2GL_OK;
}

int pil2gl_bn128_poseidon_dev(const uint64_t *in, const uint64_t *init, uint64_t count, uint32_t nIn, uint32_t nOut, uint64_t *out, void *stream) {
    P2_TRY(ensure_init());
    if (count == 0) return PIL2GL_OK;
    if (nIn < 1 || nIn > 16) return fail(PIL2GL_EINVAL, "BN128 Poseidon takes 1..16 inputs (got %u)", nIn);
    if (nOut < 1 || nOut > nIn + 1) return fail(PIL2GL_EINVAL, "nOut must be 1..nInputs+1");
    if (!in || !out) return fail(PIL2GL_EINVAL, "null buffer");
    const Params *pf;
    P2_TRY(get_params((int)nIn + 1, &pf));
    const size_t lds = lds_bytes((int)nIn + 1);
    const unsigned pblocks = (unsigned)((count + BN_THREADS - 1) / BN_THREADS);
    if ((long)count <= WAVE_PER_PERM_MAX) {          // few permutations (a transcript squeeze, the levels of a handful of Merkle paths): a wave each
        bn_sponge_chain_kernel<<<(unsigned)count, 64, 0, as_stream(stream)>>>(in, 1, (int)nIn, init, perm_args(pf), (int)nOut, 0, out);
        KERNEL_CHECK();
        return PIL2GL_OK;
    }
    P2_TRY(set_lds_attr(bn_poseidon_kernel, lds));
    bn_poseidon_kernel<<<pblocks, BN_THREADS, lds, as_stream(stream)>>>(in, init, count, (int)nIn, (int)nOut, perm_args(pf), out);
    KERNEL_CHECK();
    return PIL2GL_OK;
}

int pil2gl_bn128_convert_dev(const uint64_t *in, uint64_t n, int toMontgomery, uint64_t *out, void *stream) {
    P2_TRY(ensure_init());
    if (n == 0) return PIL2GL_OK;
    if (!in || !out) return fail(PIL2GL_EINVAL, "null buffer");
    bn_convert_kernel<<<(unsigned)((n + 255) / 256), 256, 0, as_stream(stream)>>>(in, n, toMontgomery, out);
    KERNEL_CHECK();
    return PIL2GL_OK;
}

// getGroupProof (merklehash_bn128_p.js:142-182): row values + all `arity` nodes of idx's group at every level, normal form
int pil2gl_bn128_group_proof_dev(const uint64_t *elems, const uint64_t *nodes, uint64_t width, uint64_t height, uint32_t arity,
                                 uint64_t idx, uint64_t *hostVals, uint64_t *hostSiblings, uint32_t *nLevels) {
    P2_TRY(ensure_init());
    if (idx >= height) return fail(PIL2GL_EINVAL, "Out of range");               // :145
    P2_TRY(check_arity(arity));
    if (!nodes || !hostSiblings || !nLevels || (width && (!elems || !hostVals))) return fail(PIL2GL_EINVAL, "null buffer");
    if (width) HIP_TRY(hipMemcpy(hostVals, elems + idx * width, width * 8, hipMemcpyDeviceToHost));
    uint32_t nbits = 0; while ((1u << nbits) < arity) nbits++;
    uint64_t offset = 0, n = height, id = idx; uint32_t lv = 0;
    std::vector<uint64_t> mont;
    while (n > 1) {
        const uint64_t si = id ^ (id & (arity - 1));
        mont.resize((size_t)(lv + 1) * arity * 4);
        HIP_TRY(hipMemcpy(mont.data() + (size_t)lv * arity * 4, nodes + (offset + si) * 4, (size_t)arity * 32, hipMemcpyDeviceToHost));
        for (uint32_t i = 0; i < arity; i++) if (i >= n) memset(mont.data() + ((size_t)lv * arity + i) * 4, 0, 32);   // :165-170
        const uint64_t nextN = (n - 1) / arity + 1;
        offset += nextN * arity; n = nextN; id >>= nbits; lv++;
    }
    for (size_t k = 0; k < mont.size() / 4; k++) {
        bnp::U256 v = { { mont[4 * k], mont[4 * k + 1], mont[4 * k + 2], mont[4 * k + 3] } };
        v = bnp::h_from_mont(v);
        memcpy(hostSiblings + 4 * k, v.w, 32);
    }
    *nLevels = lv;
    return PIL2GL_OK;
}

// The same for a batch of rows in one launch and one copy each way (a proof opens 64 rows of every tree: one call per row is seven small
// synchronous copies per row and tree).  hostVals: nIdx x width; hostSiblings: nIdx x levels x arity x 4 words, normal form.
int pil2gl_bn128_group_proofs_dev(const uint64_t *elems, const uint64_t *nodes, uint64_t width, uint64_t height, uint32_t arity,
                                  const uint64_t *hostIdxs, uint32_t nIdx, uint64_t *hostVals, uint64_t *hostSiblings, uint32_t *nLevels) {
    P2_TRY(ensure_init());
    P2_TRY(check_arity(arity));
    if (!nIdx) return PIL2GL_OK;
    if (!nodes || !hostIdxs || !hostSiblings || !nLevels || (width && (!elems || !hostVals))) return fail(PIL2GL_EINVAL, "null buffer");
    for (uint32_t i = 0; i < nIdx; i++) if (hostIdxs[i] >= height) return fail(PIL2GL_EINVAL, "Out of range");       // merklehash_bn128_p.js:145
    uint32_t nbits = 0; while ((1u << nbits) < arity) nbits++;
    BnLevels L; L.levels = 0;
    uint64_t offset = 0, n = height;
    while (n > 1) {
        if (L.levels >= 40) return fail(PIL2GL_EINVAL, "too many levels");
        L.off[L.levels] = offset; L.n[L.levels] = n; L.levels++;
        const uint64_t nextN = (n - 1) / arity + 1;
        offset += nextN * arity; n = nextN;
    }
    const u64 stride = width + (u64)L.levels * arity * 4;
    u64 *d;
    P2_TRY(scratch(SCR_GROUP_PROOFS, (u64)nIdx * (stride + 1), &d));
    u64 *dIdx = d + (u64)nIdx * stride;
    HIP_TRY(hipMemcpy(dIdx, hostIdxs, (u64)nIdx * 8, hipMemcpyHostToDevice));
    bn_group_proofs_kernel<<<nIdx, 64>>>(elems, nodes, width, (int)arity, (int)nbits, dIdx, L, d);
    KERNEL_CHECK();
    std::vector<u64> h((size_t)nIdx * stride);
    HIP_TRY(hipMemcpy(h.data(), d, h.size() * 8, hipMemcpyDeviceToHost));
    const u64 per = (u64)L.levels * arity * 4;
    for (uint32_t q = 0; q < nIdx; q++) {
        if (width) memcpy(hostVals + (u64)q * width, h.data() + (u64)q * stride, width * 8);
        for (u64 k = 0; k < per / 4; k++) {
            const u64 *w = h.data() + (u64)q * stride + width + 4 * k;
            bnp::U256 v = { { w[0], w[1], w[2], w[3] } };
            v = bnp::h_from_mont(v);
            memcpy(hostSiblings + (u64)q * per + 4 * k, v.w, 32);
        }
    }
    *nLevels = L.levels;
    return PIL2GL_OK;
}

// calculateRootFromGroupProof (merklehash_bn128_p.js:184-232) for a batch of openings of one tree shape: one copy in, ONE launch (a wave per
// opening walks its whole path: bn_path_roots_kernel), one copy out
static uint64_t g_path_launches = 0;
uint64_t pil2gl_debug_bn128_path_launches(void) { return g_path_launches; }

int pil2gl_bn128_roots_from_group_proofs(const uint64_t *hostVals, const uint64_t *hostSiblings, uint64_t width, uint32_t levels, uint32_t arity, int custom,
                                         int siblingsMontgomery, const uint64_t *hostIdxs, uint32_t nIdx, uint64_t *hostRoots) {
    P2_TRY(ensure_init());
    P2_TRY(check_arity(arity));
    if (levels > 40) return fail(PIL2GL_EINVAL, "too many levels");
    if (!nIdx) return PIL2GL_OK;
    if (!hostIdxs || !hostRoots || (width && !hostVals) || (levels && !hostSiblings)) return fail(PIL2GL_EINVAL, "null buffer");
    uint32_t nbits = 0; while ((1u << nbits) < arity) nbits++;
    const Params *pf, *pl;
    P2_TRY(get_params((int)arity + 1, &pf));
    pl = pf;
    const uint64_t nEl = (width + 2) / 3, nLast = nEl % arity;
    if (nEl > 1 && !custom && nLast) P2_TRY(get_params((int)nLast + 1, &pl));
    const u64 nV = (u64)nIdx * width, nS = (u64)nIdx * levels * arity * 4, nO = (u64)nIdx * 4;
    Stage s(nV + nS + nIdx + nO);
    const u64 *dVals = s.put(hostVals, nV), *dSib = s.put(hostSiblings, nS), *dIdx = s.put(hostIdxs, nIdx);
    u64 *dRoots = s.take(nO);
    P2_TRY(s.rc());
    bn_path_roots_kernel<<<nIdx, 64>>>(dVals, dSib, dIdx, width, (int)levels, (int)arity, (int)nbits, custom ? 1 : 0, siblingsMontgomery ? 1 : 0,
                                       perm_args(pf), perm_args(pl), dRoots);
    g_path_launches++;
    KERNEL_CHECK();
    return s.get(hostRoots, dRoots, nO);
}

// ---- host-pointer forms ----
int pil2gl_bn128_poseidon(const uint64_t *in, const uint64_t *init, uint64_t count, uint32_t nIn, uint32_t nOut, uint64_t *out) {
    P2_TRY(ensure_init());
    if (count == 0) return PIL2GL_OK;
    if (!in || !out) return fail(PIL2GL_EINVAL, "null buffer");
    const u64 nI = count * nIn * 4, nS = init ? count * 4 : 0, nO = count * nOut * 4;
    Stage s(nI + nS + nO);
    const u64 *dIn = s.put(in, nI), *dInit = s.put(init, nS);
    u64 *dOut = s.take(nO);
    P2_TRY(s.rc());
    P2_TRY(pil2gl_bn128_poseidon_dev(dIn, dInit, count, nIn, nOut, dOut, nullptr));
    return s.get(out, dOut, nO);
}

// transcript.bn128.js:56-66 for a list: nBlocks full blocks of nIn elements absorbed one after the other; state element 0
// starts as hostInit and is then each permutation's output 0; hostOut = the nIn+1 outputs of the last permutation
int pil2gl_bn128_sponge_absorb(const uint64_t *hostBlocks, uint64_t nBlocks, uint32_t nIn, const uint64_t hostInit[4], uint64_t *hostOut) {
    P2_TRY(ensure_init());
    if (!hostBlocks || !hostInit || !hostOut) return fail(PIL2GL_EINVAL, "null buffer");
    if (nBlocks == 0) return fail(PIL2GL_EINVAL, "nothing to absorb");
    if (nIn < 1 || nIn > 16) return fail(PIL2GL_EINVAL, "BN128 Poseidon takes 1..16 inputs (got %u)", nIn);
    const Params *pf;
    P2_TRY(get_params((int)nIn + 1, &pf));
    const u64 nB = nBlocks * nIn * 4, nO = (u64)(nIn + 1) * 4;
    Stage s(nB + 4 + nO);
    const u64 *dBlocks = s.put(hostBlocks, nB), *dInit = s.put(hostInit, 4);
    u64 *dOut = s.take(nO);
    P2_TRY(s.rc());
    bn_sponge_chain_kernel<<<1, 64>>>(dBlocks, nBlocks, (int)nIn, dInit, perm_args(pf), (int)nIn + 1, 0, dOut);
    KERNEL_CHECK();
    return s.get(hostOut, dOut, nO);
}

int pil2gl_bn128_merkelize(const uint64_t *elems, uint64_t width, uint64_t height, uint32_t arity, int custom, uint64_t *nodes) {
    P2_TRY(ensure_init());
    if (height == 0) return fail(PIL2GL_EINVAL, "height must be > 0");
    P2_TRY(check_arity(arity));
    const u64 nE = width * height, nN = pil2gl_bn128_merkle_num_nodes(height, arity) * 4;
    Stage s(nE + nN);
    const u64 *dElems = s.put(elems, nE);
    u64 *dNodes = s.take(nN);
    P2_TRY(s.rc());
    P2_TRY(pil2gl_bn128_merkelize_dev(dElems, width, height, arity, custom, dNodes, nullptr));
    return s.get(nodes, dNodes, nN);
}

int pil2gl_bn128_linear_hash_rows(const uint64_t *in, uint64_t width, uint64_t height, uint32_t arity, int custom, uint64_t *out) {
    P2_TRY(ensure_init());
    if (height == 0) return PIL2GL_OK;
    const u64 nE = width * height, nO = height * 4;
    Stage s(nE + nO);
    const u64 *dIn = s.put(in, nE);
    u64 *dOut = s.take(nO);
    P2_TRY(s.rc());
    P2_TRY(pil2gl_bn128_linear_hash_rows_dev(dIn, width, height, arity, custom, dOut, nullptr));
    return s.get(out, dOut, nO);
}

int pil2gl_bn128_convert(const uint64_t *in, uint64_t n, int toMontgomery, uint64_t *out) {     // host-only arithmetic (a few values: roots, proofs)
    if (n && (!in || !out)) return fail(PIL2GL_EINVAL, "null buffer");
    for (uint64_t k = 0; k < n; k++) {
        bnp::U256 v = { { in[4 * k], in[4 * k + 1], in[4 * k + 2], in[4 * k + 3] } };
        v = toMontgomery ? bnp::h_to_mont(v) : bnp::h_from_mont(v);
        memcpy(out + 4 * k, v.w, 32);
    }
    return PIL2GL_OK;
}

}  // extern "C"
