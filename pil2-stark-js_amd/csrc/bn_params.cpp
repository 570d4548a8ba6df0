// BN254 Poseidon parameters on the host (interface and table layout: bn_params.h).
#include "bn_params.h"
#include "bn_consts.h"
#include "bn_msm_recode.h"
#include "../../include/pil2gl.h"
#include <string.h>
#include <algorithm>

namespace bnp {

using namespace bnc;
typedef uint64_t u64;

namespace {

// ------------------------------------------------------------------------------------------ host 256-bit arithmetic
const U256 HR = { { 0x43e1f593f0000001ull, 0x2833e84879b97091ull, 0xb85045b68181585dull, 0x30644e72e131a029ull } };
const U256 HR2 = { { 0x1bb8e645ae216da7ull, 0x53fe3ab1e35c59e3ull, 0x8c49833d53bb8085ull, 0x0216d0b17f4e44a5ull } };
const u64 HN0 = 0xc2e1f593efffffffull;
typedef unsigned __int128 u128;

bool h_ge(const U256 &a, const U256 &b) { for (int i = 3; i >= 0; i--) if (a.w[i] != b.w[i]) return a.w[i] > b.w[i]; return true; }
U256 h_sub(const U256 &a, const U256 &b) { U256 r; u64 br = 0; for (int i = 0; i < 4; i++) { u128 d = (u128)a.w[i] - b.w[i] - br; r.w[i] = (u64)d; br = (u64)(d >> 64) & 1; } return r; }
U256 h_addmod(const U256 &a, const U256 &b) {
    U256 r; u64 c = 0;
    for (int i = 0; i < 4; i++) { u128 s = (u128)a.w[i] + b.w[i] + c; r.w[i] = (u64)s; c = (u64)(s >> 64); }
    if (c || h_ge(r, HR)) r = h_sub(r, HR);
    return r;
}
U256 h_addraw(const U256 &a, const U256 &b) { U256 r; u64 c = 0; for (int i = 0; i < 4; i++) { u128 s = (u128)a.w[i] + b.w[i] + c; r.w[i] = (u64)s; c = (u64)(s >> 64); } return r; }
U256 h_mont(const U256 &a, const U256 &b) {           // a*b/2^256 mod r
    u64 t[6] = { 0, 0, 0, 0, 0, 0 };
    for (int i = 0; i < 4; i++) {
        u64 c = 0;
        for (int j = 0; j < 4; j++) { u128 x = (u128)a.w[j] * b.w[i] + t[j] + c; t[j] = (u64)x; c = (u64)(x >> 64); }
        u128 x = (u128)t[4] + c; t[4] = (u64)x; t[5] = (u64)(x >> 64);
        u64 m = t[0] * HN0;
        c = (u64)(((u128)m * HR.w[0] + t[0]) >> 64);
        for (int j = 1; j < 4; j++) { u128 y = (u128)m * HR.w[j] + t[j] + c; t[j - 1] = (u64)y; c = (u64)(y >> 64); }
        x = (u128)t[4] + c; t[3] = (u64)x; t[4] = t[5] + (u64)(x >> 64);
    }
    U256 r = { { t[0], t[1], t[2], t[3] } };
    if (t[4] || h_ge(r, HR)) r = h_sub(r, HR);
    return r;
}
U256 h_submod(const U256 &a, const U256 &b) { return h_ge(a, b) ? h_sub(a, b) : h_sub(h_addraw(a, HR), b); }   // a, b < r < 2^254
bool h_is_zero(const U256 &a) { return !(a.w[0] | a.w[1] | a.w[2] | a.w[3]); }

}  // namespace

U256 h_to_mont(const U256 &a) { return h_mont(a, HR2); }
U256 h_from_mont(const U256 &a) { U256 one = { { 1, 0, 0, 0 } }; return h_mont(a, one); }
U256 bn_mont_mul(const U256 &a, const U256 &b) { return h_mont(a, b); }
const U256 &bn_mont_one() { static const U256 v = h_to_mont(U256{ { 1, 0, 0, 0 } }); return v; }
const U256 &bn_mont_neg_one() { static const U256 v = h_submod(U256{ { 0, 0, 0, 0 } }, bn_mont_one()); return v; }
U256 bn_mont_pow(U256 base, uint64_t e) {
    U256 r = bn_mont_one();
    for (; e; e >>= 1) {
        if (e & 1) r = h_mont(r, base);
        base = h_mont(base, base);
    }
    return r;
}

namespace {

U256 h_inv_mont(const U256 &a) {                      // a^(r-2), Montgomery in and out
    U256 e = HR; e.w[0] -= 2;
    U256 acc = h_to_mont(U256{ { 1, 0, 0, 0 } });
    for (int i = 255; i >= 0; i--) {
        acc = h_mont(acc, acc);
        if ((e.w[i / 64] >> (i % 64)) & 1) acc = h_mont(acc, a);
    }
    return acc;
}

// ------------------------------------------------------------------------------------------ Poseidon parameters
// Grain LFSR parameter stream of the Poseidon paper's reference generator: 80-bit register initialised with
// field=1 (2 bits), sbox=0 (4), n=254 (12), t (12), RF (10), RP (10), thirty ones; 160 warm-up steps; output bits are
// self-shrunk (a 1 passes the next bit, a 0 drops it); field elements = 254 bits MSB first, rejected when >= r (round
// constants) or reduced mod r (the 2t Cauchy points); M[i][j] = 1/(x_i + y_j).
struct Grain {
    uint8_t b[80]; int p = 0;
    int step() { int nb = b[(p + 62) % 80] ^ b[(p + 51) % 80] ^ b[(p + 38) % 80] ^ b[(p + 23) % 80] ^ b[(p + 13) % 80] ^ b[p]; b[p] = (uint8_t)nb; p = (p + 1) % 80; return nb; }
    int next() { int nb = step(); while (!nb) { step(); nb = step(); } return step(); }
    U256 rnd() { U256 v = { { 0, 0, 0, 0 } }; for (int i = 0; i < 254; i++) { for (int k = 3; k > 0; k--) v.w[k] = (v.w[k] << 1) | (v.w[k - 1] >> 63); v.w[0] = (v.w[0] << 1) | (u64)next(); } return v; }
    Grain(int t, int rp) {
        int n = 0;
        auto put = [&](unsigned v, int w) { for (int i = w - 1; i >= 0; i--) b[n++] = (v >> i) & 1; };
        put(1, 2); put(0, 4); put(254, 12); put((unsigned)t, 12); put(N_ROUNDS_F, 10); put((unsigned)rp, 10);
        while (n < 80) b[n++] = 1;
        for (int i = 0; i < 160; i++) step();
    }
};

typedef std::vector<U256> Vec;
Vec mat_vec(const Vec &A, const Vec &x, int n) {        // A (n x n) * x
    Vec y((size_t)n);
    for (int i = 0; i < n; i++) { U256 a = { { 0, 0, 0, 0 } }; for (int j = 0; j < n; j++) a = h_addmod(a, h_mont(A[(size_t)i * n + j], x[j])); y[i] = a; }
    return y;
}
bool mat_inv(Vec &A, int n) {                            // Gauss-Jordan in place (Montgomery form); false: A is singular
    const U256 one = h_to_mont(U256{ { 1, 0, 0, 0 } });
    Vec I((size_t)n * n, U256{ { 0, 0, 0, 0 } });
    for (int i = 0; i < n; i++) I[(size_t)i * n + i] = one;
    for (int c = 0; c < n; c++) {
        int p = c;
        while (p < n && h_is_zero(A[(size_t)p * n + c])) p++;
        if (p == n) return false;
        if (p != c) for (int j = 0; j < n; j++) { std::swap(A[(size_t)p * n + j], A[(size_t)c * n + j]); std::swap(I[(size_t)p * n + j], I[(size_t)c * n + j]); }
        const U256 iv = h_inv_mont(A[(size_t)c * n + c]);
        for (int j = 0; j < n; j++) { A[(size_t)c * n + j] = h_mont(A[(size_t)c * n + j], iv); I[(size_t)c * n + j] = h_mont(I[(size_t)c * n + j], iv); }
        for (int r = 0; r < n; r++) {
            if (r == c || h_is_zero(A[(size_t)r * n + c])) continue;
            const U256 f = A[(size_t)r * n + c];
            for (int j = 0; j < n; j++) {
                A[(size_t)r * n + j] = h_submod(A[(size_t)r * n + j], h_mont(f, A[(size_t)c * n + j]));
                I[(size_t)r * n + j] = h_submod(I[(size_t)r * n + j], h_mont(f, I[(size_t)c * n + j]));
            }
        }
    }
    A = I;
    return true;
}

// Sparse form of the RP partial rounds.  Dense statement: x_{k+1} = M * sigma(x_k + c_k), sigma = x^5 on element 0 only.
//  (1) constants: with e_0 = c_0, s_k = e_k[0], e_{k+1} = c_{k+1} + M*(0, e_k[1:]), the sequence y_{k+1} = M*sigma'(y_k + s_k e0)
//      satisfies x_k + c_k = y_k + e_k; what is left, f = M*(0, e_{RP-1}[1:]), joins the next full round's constants.
//  (2) matrices: M = [[m00, v],[w, Mh]].  With D_k = diag(1, Mh^k), M*D_k = D_{k+1} * [[m00, v*Mh^k],[Mh^-(k+1) w, I]], and
//      D_k commutes with sigma', so y_k = D_k u_k with u_{k+1} = [[m00, V_k],[W_k, I]] * sigma'(u_k): 2t-1 products;
//      one dense multiplication by D_RP = diag(1, Mh^RP) closes the sequence.
bool derive_sparse(int t, int rp, const Vec &C, const Vec &M, Vec &C8, Vec &D, Vec &S, Vec &V, Vec &W) {
    const int n = t - 1;
    const U256 zero = { { 0, 0, 0, 0 } };
    Vec Mh((size_t)n * n), v((size_t)n), w((size_t)n);
    for (int i = 0; i < n; i++) { v[i] = M[(size_t)1 + i]; w[i] = M[(size_t)(i + 1) * t]; for (int j = 0; j < n; j++) Mh[(size_t)i * n + j] = M[(size_t)(i + 1) * t + 1 + j]; }
    Vec Mhi = Mh;
    if (!mat_inv(Mhi, n)) return false;
    S.resize((size_t)rp); V.resize((size_t)rp * n); W.resize((size_t)rp * n); C8.resize((size_t)8 * t);
    Vec e(C.begin() + (size_t)4 * t, C.begin() + (size_t)5 * t), f;
    for (int k = 0; k < rp; k++) {
        S[k] = e[0];
        Vec et = e; et[0] = zero;
        Vec Me = mat_vec(M, et, t);
        if (k + 1 < rp) for (int j = 0; j < t; j++) e[j] = h_addmod(C[(size_t)(5 + k) * t + j], Me[j]);
        else f = Me;
    }
    Vec vk = v, wk = mat_vec(Mhi, w, n);
    for (int k = 0; k < rp; k++) {
        for (int j = 0; j < n; j++) { V[(size_t)k * n + j] = vk[j]; W[(size_t)k * n + j] = wk[j]; }
        Vec nv((size_t)n);
        for (int j = 0; j < n; j++) { U256 a = zero; for (int i = 0; i < n; i++) a = h_addmod(a, h_mont(vk[i], Mh[(size_t)i * n + j])); nv[j] = a; }
        vk = nv;
        wk = mat_vec(Mhi, wk, n);
    }
    D.assign((size_t)n * n, zero);
    const U256 one = h_to_mont(U256{ { 1, 0, 0, 0 } });
    for (int i = 0; i < n; i++) D[(size_t)i * n + i] = one;
    for (int k = 0; k < rp; k++) {
        Vec nd((size_t)n * n);
        for (int i = 0; i < n; i++) for (int j = 0; j < n; j++) { U256 a = zero; for (int q = 0; q < n; q++) a = h_addmod(a, h_mont(Mh[(size_t)i * n + q], D[(size_t)q * n + j])); nd[(size_t)i * n + j] = a; }
        D = nd;
    }
    for (int r = 0; r < 4; r++) for (int j = 0; j < t; j++) {
        C8[(size_t)r * t + j] = C[(size_t)r * t + j];
        C8[(size_t)(4 + r) * t + j] = r == 0 ? h_addmod(C[(size_t)(4 + rp) * t + j], f[j]) : C[(size_t)(4 + rp + r) * t + j];
    }
    return true;
}

// Operand tiles and row constants for the matrix cores (layout and derivation: bn_mfma.cuh).
struct MfmaConsts {
    U256 P[32];                                      // 2^(8b+32) mod r, plain
    U256 off;                                        // sum_k ACC_BIAS 256^k mod r
    MfmaConsts() {
        U256 v = { { 1, 0, 0, 0 } };
        for (int e = 0; e < 32; e++) v = h_addmod(v, v);
        for (int b = 0; b < 32; b++) { P[b] = v; for (int e = 0; e < 8; e++) v = h_addmod(v, v); }
        off = U256{ { 0, 0, 0, 0 } };
        v = U256{ { (u64)ACC_BIAS, 0, 0, 0 } };
        for (int k = 0; k < 32; k++) { off = h_addmod(off, v); for (int e = 0; e < 8; e++) v = h_addmod(v, v); }
    }
};
// one tile (1 KB, lane order) of the coefficient a0 (Montgomery form); tot += the sum of its 32 constants.  sboxed: the operand this tile
// multiplies comes straight out of the S-box, i.e. (bn_field29.cuh) carries a factor 2^-20: the coefficient takes it back
void mfma_tile(const MfmaConsts &mc, const U256 &a0, int8_t *tile, U256 &tot, bool sboxed, const U256 *extra = nullptr) {
    U256 a = sboxed ? h_mont(a0, h_to_mont(U256{ { 1ull << 20, 0, 0, 0 } })) : a0;
    if (extra) a = h_mont(a, *extra);                // (a further factor in Montgomery form: the plain-input first layer)
    for (int b = 0; b < 32; b++) {
        const U256 c = h_mont(a, mc.P[b]);           // a 2^(8b+32) mod r as a plain integer
        tot = h_addmod(tot, c);
        int d[32], carry = 0;
        for (int k = 0; k < 32; k++) {
            int v = (int)((c.w[k / 8] >> (8 * (k % 8))) & 255) + carry;
            carry = v >= 128;
            d[k] = carry ? v - 256 : v;
        }                                             // c < 2^254: the top digit takes the last carry
        const int g = b / 16, sl = b % 16;
        for (int m = 0; m < 32; m++) {
            const int pos = 16 * ((m / 4) % 2) + 4 * (m / 8) + m % 4;
            tile[(size_t)(g * 32 + m) * 16 + sl] = (int8_t)d[pos];
        }
    }
}
// the row constant: (128 tot - nAcc sum_k ACC_BIAS 256^k) / 2^32 + fold mod r   (nAcc accumulations started at the bias make up the row)
U256 mfma_row_const(const MfmaConsts &mc, U256 tot, int nAcc, const U256 &fold) {
    const U256 inv32 = { { 0, 0, 0, 1ull << 32 } };  // 2^224: h_mont(a, 2^224) = a / 2^32
    for (int e = 0; e < 7; e++) tot = h_addmod(tot, tot);
    for (int e = 0; e < nAcc; e++) tot = h_submod(tot, mc.off);
    return h_addmod(h_mont(tot, inv32), fold);
}
// A: rows x cols entries in Montgomery form.  tiles: rows*cols KB; K: rows plain integers mod r (callers add what follows the layer).
// colFactor: columns >= 1 carry this further factor (Montgomery form)
void mfma_layer_tables(const Vec &A, int rows, int cols, std::vector<int8_t> &tiles, Vec &K, bool sboxed, const U256 *colFactor = nullptr) {
    const MfmaConsts mc;
    const U256 zero = { { 0, 0, 0, 0 } };
    tiles.assign((size_t)rows * cols * 1024, 0);
    K.resize((size_t)rows);
    for (int i = 0; i < rows; i++) {
        U256 tot = zero;
        for (int j = 0; j < cols; j++) mfma_tile(mc, A[(size_t)i * cols + j], tiles.data() + ((size_t)i * cols + j) * 1024, tot, sboxed, j >= 1 ? colFactor : nullptr);
        K[i] = mfma_row_const(mc, tot, 1, zero);
    }
}
// The partial rounds four to a block, blocks two to a SUPER-BLOCK (partial_rounds_mfma): the tile stream in the order the kernel consumes it and
// the row constants.  Block b (rounds k0 = 4b .. k0+3), z_i = the S-box output of round k0+i, y = elements 1..n at the start of b's SUPER-BLOCK:
//   x0 after round k0+i = m00 z_i + sum_j V[k0+i][j] y_j + sum_{i'<i} (V[k0+i] . W[k0+i']) z_i'  [+ for the second block of a super-block the same
//   cross terms with the four z of the first];   y_j after the super-block = y_j + sum over its rounds of W[k][j] z_k  (one column update per 8 rounds).
// Stream per block, in two passes (rows 0-1, then rows 2-3): n x 2 tiles V[k0+i][j] (j outer), second block: 2 x 4 tiles (V[k0+i] . W[k0-4+s]);  then the block's own
// cross terms, round i = 0..3: i + 1 tiles (z_0 .. z_i of the block; the last is m00).  Per super-block after its blocks: n x (1 + 8) tiles (1, W[k][j]; four zero tiles when
// the super-block has one block).
// KR[k]: round k's row constant with S[k+1] folded in while round k+1 is one of these; KU[sb][j]: the column constants.
void mfma_partial_tables(int t, int rp, const Vec &S, const Vec &V, const Vec &W, const U256 &m00, std::vector<int8_t> &tiles, Vec &KR, Vec &KU) {
    const MfmaConsts mc;
    const U256 zero = { { 0, 0, 0, 0 } }, one = h_to_mont(U256{ { 1, 0, 0, 0 } });
    const int n = t - 1, nb = rp / 4, nsb = (nb + 1) / 2;
    tiles.assign(((size_t)nb * (4 * n + 10) + (size_t)nsb * 9 * n + (size_t)(nb / 2) * 16) * 1024, 0);      // per block its rows and rounds, per super-block the columns (1 + 8 tiles each), 16 more for a second block's rows
    KR.assign((size_t)nb * 4, zero); KU.assign((size_t)nsb * n, zero);
    auto dot = [&](int ka, int kb) { U256 c = zero; for (int j = 0; j < n; j++) c = h_addmod(c, h_mont(V[(size_t)ka * n + j], W[(size_t)kb * n + j])); return c; };
    int8_t *tp = tiles.data();
    for (int sb = 0; sb < nsb; sb++) {
        const int halves = nb - 2 * sb >= 2 ? 2 : 1;
        for (int h = 0; h < halves; h++) {
            const int k0 = 4 * (2 * sb + h);
            U256 tot[4] = { zero, zero, zero, zero };
            // the kernel takes the rows two at a time (partial_rounds_mfma_impl::rows): the first pass walks the columns in order, the second starts with the last
            // batch of the columns that live in private memory (still in its registers), then the first batch, then the columns in LDS
            const int nlo = n + 1 <= BN_LDS_ELEMS ? n : BN_LDS_ELEMS - 1, nhi = n - nlo, hb2 = nhi < BN_HI_BATCH ? nhi : BN_HI_BATCH, spl = nhi - hb2;
            for (int pass = 0; pass < 2; pass++) {
                std::vector<int> order;
                if (pass == 0) for (int j = 0; j < n; j++) order.push_back(j);
                else {
                    for (int q = spl; q < nhi; q++) order.push_back(nlo + q);
                    for (int q = 0; q < spl; q++) order.push_back(nlo + q);
                    for (int j = 0; j < nlo; j++) order.push_back(j);
                }
                for (int j : order) for (int i = 2 * pass; i < 2 * pass + 2; i++, tp += 1024) mfma_tile(mc, V[(size_t)(k0 + i) * n + j], tp, tot[i], false);
                if (h == 1) for (int i = 2 * pass; i < 2 * pass + 2; i++) for (int s = 0; s < 4; s++, tp += 1024) mfma_tile(mc, dot(k0 + i, k0 - 4 + s), tp, tot[i], true);
            }
            for (int i = 0; i < 4; i++) {
                for (int ip = 0; ip <= i; ip++, tp += 1024)                                    // round i: its i + 1 cross terms, z_0 .. z_i of the block
                    mfma_tile(mc, ip < i ? dot(k0 + i, k0 + ip) : m00, tp, tot[i], true);      // a z: the S-box's output
                KR[(size_t)k0 + i] = mfma_row_const(mc, tot[i], 2, k0 + i + 1 < 4 * nb ? S[(size_t)k0 + i + 1] : zero);
            }
        }
        for (int j = 0; j < n; j++) {
            U256 tu = zero;
            mfma_tile(mc, one, tp, tu, false); tp += 1024;
            if (halves == 1) tp += 4 * 1024;       // (zero tiles where the kernel multiplies the absent first block's operands: one form of the column)
            for (int s = 0; s < 4 * halves; s++, tp += 1024) mfma_tile(mc, W[(size_t)(8 * sb + s) * n + j], tp, tu, true);
            KU[(size_t)sb * n + j] = mfma_row_const(mc, tu, 1, zero);
        }
    }
}


// The tables are packed by appending: a region goes where the blob ends and its offset comes back, counted in units of `unit` items;
// `spare` zero units follow it (the tiles a kernel's read-ahead touches past the end of a table)
template <typename T>
size_t append(std::vector<T> &blob, const std::vector<T> &region, size_t unit = 1, size_t spare = 0) {
    const size_t o = blob.size() / unit;
    blob.insert(blob.end(), region.begin(), region.end());
    blob.resize(blob.size() + spare * unit);
    return o;
}

}  // namespace

int bn_build_params(int t, BnHostParams &out) {
    out = BnHostParams();
    if (t < 2 || t > 17) { out.error = "BN128 Poseidon takes 1..16 inputs (t=" + std::to_string(t) + ")"; return PIL2GL_EINVAL; }
    const int rp = N_ROUNDS_P[t - 2], nC = (N_ROUNDS_F + rp) * t, n = t - 1;
    Grain g(t, rp);
    Vec C((size_t)nC), M((size_t)t * t), xy((size_t)2 * t);
    for (int i = 0; i < nC; i++) { U256 v = g.rnd(); while (h_ge(v, HR)) v = g.rnd(); C[i] = h_to_mont(v); }
    for (int i = 0; i < 2 * t; i++) { U256 v = g.rnd(); while (h_ge(v, HR)) v = h_sub(v, HR); xy[i] = h_to_mont(v); }
    for (int i = 0; i < t; i++) for (int j = 0; j < t; j++) M[(size_t)i * t + j] = h_inv_mont(h_addmod(xy[i], xy[t + j]));
    Vec C8, D, S, V, W;
    if (!derive_sparse(t, rp, C, M, C8, D, S, V, W)) { out.error = "singular MDS sub-matrix"; return PIL2GL_EINVAL; }
    out.C8 = append(out.elems, C8); out.M = out.m00 = append(out.elems, M); out.S = append(out.elems, S);
    out.V = append(out.elems, V); out.W = append(out.elems, W); out.Cd = append(out.elems, C);

    std::vector<int8_t> tm, td, tpr, tm0; Vec km0, km, kd, kr, ku, km0p, c0p;
    mfma_layer_tables(M, t, t, tm, km0, true);     // every dense layer follows an S-box layer
    // The first layer once more for inputs that went through the S-box as PLAIN integers (leaf kernel: v + c instead of (v + c) 2^256 mod r,
    // no conversion product): bn29::pow5 then returns the state form's value times 2^-1280 (five missing factors 2^256), which columns 1..t-1 of
    // this copy take back.  c0p: the first round's constants as plain integers.
    {
        U256 f = { { 1, 0, 0, 0 } };
        for (int e = 0; e < 1280; e++) f = h_addmod(f, f);
        const U256 fm = h_to_mont(f);
        mfma_layer_tables(M, t, t, tm0, km0p, true, &fm);
        c0p.resize((size_t)t);
        for (int i = 0; i < t; i++) c0p[i] = h_mont(C8[i], U256{ { 1, 0, 0, 0 } });
    }
    mfma_layer_tables(D, n, n, td, kd, false);    // the closing layer reads the columns the blocks left
    mfma_partial_tables(t, rp, S, V, W, M[0], tpr, kr, ku);
    // What follows a layer is added by its row constants (the values in between are lazy representatives, no other addition
    // is left): the next full round's constants C8; after the fourth full round S[0] on element 0; after the closing layer
    // C8[4] on elements 1..n -- element 0 gets C8[4][0] from the last partial round's row when that round is one of the
    // blocked ones (rp % 4 == 0), from the vector code otherwise.  MK: one set per dense layer of the permutation, 8 x t.
    km.resize((size_t)8 * t);
    for (int inst = 0; inst < 8; inst++) for (int i = 0; i < t; i++) {
        U256 f = { { 0, 0, 0, 0 } };
        if (inst == 3) { if (i == 0) f = S[0]; }
        else if (inst < 7) f = C8[(size_t)(inst + 1) * t + i];
        km[(size_t)inst * t + i] = h_addmod(km0[i], f);
    }
    for (int i = 0; i < t; i++) km0p[i] = h_addmod(km0p[i], C8[(size_t)t + i]);
    for (int i = 0; i < n; i++) kd[i] = h_addmod(kd[i], C8[(size_t)4 * t + 1 + i]);
    if (rp % 4 == 0 && rp >= 4) kr[(size_t)rp - 1] = h_addmod(kr[(size_t)rp - 1], C8[(size_t)4 * t]);
    // Small widths (t <= BN_SMALL_T): poseidon.circom:22-44 as written, every round one t x t layer of the SAME matrix -- two tile sets (after a full
    // round every column comes out of the S-box, after a partial round only column 0) that stay in registers, and one row constant per round and row
    // (the layer's own + the next round's constants).  No tile stream, no sparse blocks: a width-3 permutation is a chain of 65 short rounds whose
    // latency, not its work, was the cost (perm_small).
    std::vector<int8_t> ts; Vec sk;
    if (t <= BN_SMALL_T) {
        const MfmaConsts mc;
        const U256 zero = { { 0, 0, 0, 0 } };
        const int R = N_ROUNDS_F + rp;
        ts.assign((size_t)2 * t * t * 1024, 0);
        Vec kset[2]; kset[0].resize((size_t)t); kset[1].resize((size_t)t);
        for (int set = 0; set < 2; set++)
            for (int i = 0; i < t; i++) {
                U256 tot = zero;
                for (int j = 0; j < t; j++) mfma_tile(mc, M[(size_t)i * t + j], ts.data() + ((size_t)(set * t + i) * t + j) * 1024, tot, set == 0 || j == 0);
                kset[set][i] = mfma_row_const(mc, tot, 1, zero);
            }
        sk.resize((size_t)R * t);
        for (int r = 0; r < R; r++) {
            const bool full = r < N_ROUNDS_F / 2 || r >= N_ROUNDS_F / 2 + rp;
            for (int i = 0; i < t; i++) sk[(size_t)r * t + i] = h_addmod(kset[full ? 0 : 1][i], r + 1 < R ? C[(size_t)(r + 1) * t + i] : zero);
        }
    }
    auto tiles = [&](const std::vector<int8_t> &x) { return append(out.tiles, x, 1024, BN_SPARE_TILES); };
    out.Mt = tiles(tm); out.Dt = tiles(td); out.Pt = tiles(tpr); out.Mt0 = tiles(tm0); out.St = tiles(ts);
    out.MK = append(out.consts, km); out.DK = append(out.consts, kd); out.KR = append(out.consts, kr); out.KU = append(out.consts, ku);
    out.MK0 = append(out.consts, km0p); out.C0p = append(out.consts, c0p); out.SK = append(out.consts, sk);
    if (ts.empty()) out.St = out.SK = BN_ABSENT;     // (the tile table still ends with the spare tiles of the absent region)
    out.t = t; out.rp = rp;
    return PIL2GL_OK;
}

// ------------------------------------------------------------------------------------------ the Fr transforms
void bn_powers(const U256 &g, size_t n, U256 *out) {
    U256 acc = bn_mont_one();
    for (size_t i = 0; i < n; i++) { out[i] = acc; acc = h_mont(acc, g); }
}

const BnNttConsts &bn_ntt_consts() {
    static const BnNttConsts K = [] {
        BnNttConsts c;
        U256 e = HR; e.w[0] -= 1;                    // (r - 1) >> 28
        for (int i = 0; i < 4; i++) e.w[i] = (e.w[i] >> BN_NTT_MAX_BITS) | (i < 3 ? e.w[i + 1] << (64 - BN_NTT_MAX_BITS) : 0);
        const U256 one = h_to_mont(U256{ { 1, 0, 0, 0 } }), five = h_to_mont(U256{ { 5, 0, 0, 0 } });
        U256 acc = one;
        for (int i = 255; i >= 0; i--) {
            acc = h_mont(acc, acc);
            if ((e.w[i / 64] >> (i % 64)) & 1) acc = h_mont(acc, five);
        }
        c.w[BN_NTT_MAX_BITS] = acc;
        for (int k = (int)BN_NTT_MAX_BITS - 1; k >= 0; k--) c.w[k] = h_mont(c.w[k + 1], c.w[k + 1]);
        U256 p2 = one;
        for (unsigned k = 0; k <= BN_NTT_MAX_BITS; k++) { c.wi[k] = h_inv_mont(c.w[k]); c.ninv[k] = h_inv_mont(p2); p2 = h_addmod(p2, p2); }
        return c;
    }();
    return K;
}

int bn_ntt_plan(unsigned nBits, unsigned *layers) {
    if (nBits > BN_NTT_MAX_BITS) return -1;
    const unsigned S = (nBits + BN_NTT_KMAX - 1) / BN_NTT_KMAX;
    for (unsigned i = 0; i < S; i++) layers[i] = nBits / S + (i < nBits % S ? 1 : 0);
    return (int)S;
}

// ------------------------------------------------------------------------------------------ the G1 MSM
BnMsmPlan bn_msm_batch_plan(uint32_t K, const uint64_t *counts) {
    uint64_t N = 0, nMax = 1;
    for (uint32_t k = 0; k < K; k++) { N += counts[k]; nMax = std::max(nMax, counts[k]); }
    if (N == 0) N = 1;
    if (K == 0) K = 1;
    BnMsmPlan p;
    uint32_t lg = 0;
    while ((nMax >> lg) > 1) lg++;
    p.c = lg < bnm::MSM_MIN_C + 3 ? bnm::MSM_MIN_C : (lg - 3 > bnm::MSM_MAX_C ? bnm::MSM_MAX_C : lg - 3);
    auto windows = [](uint32_t c) { return (bnm::MSM_SCALAR_BITS + 1 + c - 1) / c; };
    while (p.c > bnm::MSM_MIN_C && (uint64_t)K * windows(p.c) << (p.c - 1) > BN_MSM_BUCKET_BUDGET) p.c--;
    p.nWindows = windows(p.c);
    p.bucketsPerWindow = 1u << (p.c - 1);
    const uint64_t lo = 1ull << 19, hi = 1ull << 30;
    const uint64_t room = std::min(std::max(8 * N, lo), hi) / N;         // entries / N >= 1 for N <= 2^30
    auto cells = [&](uint32_t g) { return (uint64_t)K * std::min(g, p.nWindows) * p.bucketsPerWindow; };
    uint32_t g = 1;
    while (2ull * g <= room && 2 * g <= bnm::MSM_MAX_WINDOWS && cells(2 * g) <= BN_MSM_PASS_CELLS) g *= 2;
    p.windowsPerPass = std::min(g, p.nWindows);
    p.m1 = (p.bucketsPerWindow + BN_MSM_L1 - 1) / BN_MSM_L1;
    p.m2 = (p.m1 + BN_MSM_L - 1) / BN_MSM_L;
    auto up16 = [](uint64_t x) { return (x + 15) & ~15ull; };
    const uint64_t nbPass = cells(p.windowsPerPass), items = (uint64_t)K * p.nWindows;
    p.offHist = 0;
    p.offCursor = up16((nbPass + 1) * 4);
    p.offEntries = p.offCursor + up16(nbPass * 4);
    p.offBuckets = p.offEntries + up16(N * p.windowsPerPass * 4);
    p.offLevelA = p.offBuckets + items * p.bucketsPerWindow * 128;
    p.offLevelB = p.offLevelA + 2 * items * p.m1 * 128;
    p.scratchBytes = p.offLevelB + 2 * items * p.m2 * 128;
    return p;
}

}  // namespace bnp
