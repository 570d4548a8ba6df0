// Multi-column Goldilocks NTT / iNTT / LDE on a row-major rows x C matrix (gfx950).
//
// Replaces src/helpers/fft/fft_p.js:178-302 (interpolate / fft / ifft) of the reference, whose
// result is, per column, F.fft / F.ifft / extendPol (test/fft_p.test.js:47-229).
//
// Design (not the reference's block/transposition scheme):
//  * A transform of 2^n rows is cut into passes of k index bits (8, or 7 for matrices whose rows are
//    shorter than 128 bytes; at most 10).  One workgroup owns a tile of 2^k rows (stride 2^lo rows)
//    x S column slots in LDS, runs the k stages there as register steps of up to four stages (16-row
//    sub-transforms in Z/(2^96+1), see below), and applies the inter-pass twiddle w_(2^(lo+k))^(b*j)
//    from a per-tile LDS table that is shared by all columns of the tile.  All passes are in place.
//    Workgroups are numbered so that the column chunks of one row block run on one XCD (one L2); in the 16-slot pass kernels a
//    workgroup takes a run of consecutive chunks of its row tile and builds the tables once (walk_at).
//  * Forward/inverse transforms run decimation-in-frequency (natural in -> bit-reversed out);
//    the last pass scatters rows to their bit-reversed index so the caller sees natural order.
//  * interpolate (LDE) never reorders anything: iNTT as DIF leaves coefficient m at row
//    bitrev(m); the "mid" kernel finishes the iNTT on a contiguous tile, multiplies coefficient m
//    by (7*w_E^j)^m / N for each of the 2^b cosets j and immediately runs the first k stages of a
//    decimation-in-time NTT (bit-reversed in -> natural out), writing coset j's tile to rows
//    (pos << b) + j of dst.  dst is then just an N x (C*2^b) matrix on which the remaining DIT
//    passes run in place.  Extended row i = 8k+j is coset point 7*w_E^(8k+j): natural order.
//  * Rows are contiguous in memory, so a tile row is one contiguous segment of Wc*8 bytes
//    (or several adjacent rows when C is small): every global access is a coalesced segment.
//  * The host side plans first and launches second: plan_ntt / plan_lde turn (rows, columns, cosets) into a short list of launches
//    (kernel instance, tile geometry, grid, LDS) without touching a device, ntt_launch / lde_launch run the list, and
//    pil2gl_debug_plan_transform shows it to the tests.  Three environment switches, read once per call, are test hooks that reach
//    pass sizes and kernel families the default plan does not: PIL2GL_NTT_KMAX, PIL2GL_NTT_GENERIC, PIL2GL_LDE_WIDEFWD.
#include "common.h"
#include "gl_field.cuh"
#include "gl_fermat.cuh"
#include <stdlib.h>
#include <algorithm>

#ifndef NTT_MUL
#define NTT_MUL(a, b) mul_lazy_x(a, b)   // the twiddle products of the tile kernels: the 16-instruction exact carry-out form (A/B: -DNTT_MUL=mul_lazy, 22 compiler instructions: 208.5 vs 201.5 ms per config-3 interpolate)
#endif
using namespace gl;

namespace {

__device__ __forceinline__ u64 pow256(const u64 *__restrict__ T, u32 e) {
    u64 r = T[e & 255];
    r = mul_lazy(r, T[256 + ((e >> 8) & 255)]);
    r = mul_lazy(r, T[512 + ((e >> 16) & 255)]);
    return mul(r, T[768 + (e >> 24)]);
}
// w_(2^logM)^e for the root whose pow256 table is T (1 <= logM <= 32, e < 2^logM)
__device__ __forceinline__ u64 root_pow(const u64 *__restrict__ T, u32 logM, u32 e) { return pow256(T, e << (32 - logM)); }

// k stages on tile[2^k][S] (column x).  The stages are grouped into register steps of c <= 4 stages: a lane takes the
// 2^c rows of one sub-transform into registers, runs it in Z/(2^96+1) where its twiddles are constant shifts
// (gl_fermat.cuh), reduces once, multiplies by the twiddle that joins it to the next group and writes it back: one LDS
// round trip and one modular multiplication per element per c stages.  TW[j] = w_(2^k)^j for all j < 2^k.
__host__ __device__ constexpr u32 next_chunk(u32 rem) { return rem <= 4 ? rem : (rem == 5 || rem == 6 || rem == 9) ? 3 : 4; }
__host__ __device__ constexpr u32 brev_c(u32 i, int c) { u32 r = 0; for (int b = 0; b < c; b++) r |= ((i >> b) & 1u) << (c - 1 - b); return r; }

// Gentleman-Sande group on blocks of 2^lm rows: natural in -> bit-reversed out (within the group's c index bits)
// PAD (fixed-geometry kernels: k = 8, C = 4): tile row t lives at row t + (t >> 4), one spare row per 16, so that the four
// sub-transforms a wave reads together (rows 256 words apart otherwise: the same LDS banks) start in different banks
template <int C, bool INV, bool PAD = false>
__device__ __forceinline__ void dif_step(u64 *tile, const u64 *TW, u32 k, u32 lm, u32 S, u32 x, u32 y, u32 by) {
    constexpr u32 R = 1u << C;
    const u32 ls = lm - C, nD = 1u << (k - C), st = PAD && ls == 4 ? (S << ls) + S : S << ls;
    const bool last = ls == 0;
    for (u32 d = y; d < nD; d += by) {
        const u32 np = d & ((1u << ls) - 1);
        u64 *col = tile + (size_t)(((d >> ls) << lm) + np + (PAD && ls == 0 ? d : 0)) * S + x;
        fermat::f128 v[R];
#pragma unroll
        for (u32 r = 0; r < R; r++) v[r] = fermat::from_gl(col[r * st]);
        fermat::dft_dif<C, INV>(v);
        const u32 e1 = np << (k - lm);                         // w_(2^lm)^np = TW[e1]
#pragma unroll
        for (u32 i = 0; i < R; i++) {
            const u32 q = brev_c(i, C);
            u64 o = fermat::to_gl_lazy(v[i]);
            if (!last && q) o = NTT_MUL(o, TW[e1 * q]);            // the tile stays lazy: whoever stores a FINAL result canonicalises it
            col[i * st] = o;
        }
    }
    __syncthreads();
}
// Cooley-Tukey group joining 2^C finished blocks of 2^lp rows: bit-reversed in -> natural out.  The inputs already carry
// this group's twiddles (applied when they were stored); the outputs get the next group's (cn = its stage count, 0: none).
template <int C, bool INV, bool PAD = false>
__device__ __forceinline__ void dit_step(u64 *tile, const u64 *TW, u32 k, u32 lp, u32 cn, u32 S, u32 x, u32 y, u32 by) {
    constexpr u32 R = 1u << C;
    const u32 lm = lp + C, nD = 1u << (k - C), st = PAD && lp == 4 ? (S << lp) + S : S << lp;
    for (u32 d = y; d < nD; d += by) {
        const u32 np = d & ((1u << lp) - 1), blk = d >> lp;
        u64 *col = tile + (size_t)((blk << lm) + np + (PAD && lp == 0 ? blk : 0)) * S + x;
        fermat::f128 v[R];
#pragma unroll
        for (u32 r = 0; r < R; r++) v[r] = fermat::from_gl(col[r * st]);
        fermat::dft_dit<C, INV>(v);
        if (cn) {
            const u32 rho = bitrev32(blk & ((1u << cn) - 1), cn), sh = k - lm - cn;
#pragma unroll
            for (u32 q = 0; q < R; q++) {
                // rho = 0 multiplies by TW[0] = 1: cheaper than a lane-dependent branch around every product
                col[q * st] = NTT_MUL(fermat::to_gl_lazy(v[q]), TW[(rho * (np + (q << lp))) << sh]);
            }
        } else {
#pragma unroll
            for (u32 q = 0; q < R; q++) col[q * st] = fermat::to_gl_lazy(v[q]);     // lazy, see dif_step
        }
    }
    __syncthreads();
}
template <bool INV>
__device__ __forceinline__ void dif_stages(u64 *tile, const u64 *TW, u32 k, u32 S, u32 x, u32 y, u32 by) {
    for (u32 lm = k; lm > 0;) {
        const u32 c = next_chunk(lm);
        switch (c) {
        case 4: dif_step<4, INV>(tile, TW, k, lm, S, x, y, by); break;
        case 3: dif_step<3, INV>(tile, TW, k, lm, S, x, y, by); break;
        case 2: dif_step<2, INV>(tile, TW, k, lm, S, x, y, by); break;
        default: dif_step<1, INV>(tile, TW, k, lm, S, x, y, by); break;
        }
        lm -= c;
    }
}
template <bool INV>
__device__ __forceinline__ void dit_stages(u64 *tile, const u64 *TW, u32 k, u32 S, u32 x, u32 y, u32 by) {
    for (u32 lp = 0; lp < k;) {
        const u32 c = next_chunk(k - lp), cn = next_chunk(k - lp - c);
        switch (c) {
        case 4: dit_step<4, INV>(tile, TW, k, lp, cn, S, x, y, by); break;
        case 3: dit_step<3, INV>(tile, TW, k, lp, cn, S, x, y, by); break;
        case 2: dit_step<2, INV>(tile, TW, k, lp, cn, S, x, y, by); break;
        default: dit_step<1, INV>(tile, TW, k, lp, cn, S, x, y, by); break;
        }
        lp += c;
    }
}

// Workgroups are dealt round-robin over the 8 XCDs (blocks b and b+8 share one, each XCD has its own L2).  Tiles that are
// neighbours in memory -- the column chunks of the same rows, whose row segments share cache lines when the row length is
// not a multiple of 128 bytes -- are consecutive logical indices; this maps consecutive logical indices to one XCD, so the
// second half of a straddled line is found (reads) or completed (writes) in the same L2.
__host__ __device__ constexpr u32 xcd_local_block(u32 b, u32 grid) {
    const u32 per = grid >> 3;
    return b < (per << 3) ? (b & 7) * per + (b >> 3) : b;
}

// The chunk walk: which tile of the launch workgroup `block` (of `grid`) works on in its step `step`.  A launch is nHi x nGroupTiles row
// tiles x nColChunks column chunks; a workgroup owns ONE row tile (hi, gt) and a run of up to W consecutive chunks of it, a last shorter
// run taking what W leaves over, so that whatever depends on the row tile alone -- the twiddle and scale tables -- is built once per W
// chunks.  The runs of a row tile are consecutive logical indices: one XCD.  -> false where the workgroup has no such step (step 0
// always exists).  W = 1 is one tile per workgroup, the chunk index varying fastest.  The kernels and the host's account of a launch
// (pil2gl_debug_transform_walk) both go through this one function.
__host__ __device__ constexpr bool walk_at(u32 block, u32 grid, u32 step, u32 W, u32 nColChunks, u32 nGroupTiles, u32 &hi, u32 &gt, u32 &cc) {
    const u32 b = xcd_local_block(block, grid), runs = (nColChunks + W - 1) / W, rowTile = b / runs;
    hi = rowTile / nGroupTiles;
    gt = rowTile - hi * nGroupTiles;
    cc = (b - rowTile * runs) * W + step;
    return step < W && cc < nColChunks;
}
// its workgroups: ceil(nColChunks / W) runs per row tile
__host__ __device__ constexpr u64 walk_grid(u64 rowTiles, u32 W, u32 nColChunks) { return rowTiles * ((nColChunks + W - 1) / W); }

// Two adjacent column slots of one tile row.  The 16-slot fixed-geometry kernels move a tile between HBM and LDS in these: lane
// tid owns slots 2*px, 2*px+1 (px = tid & 7) of the eight tile rows r + 32*i (r = tid >> 3), so a 128-byte row piece is 8 lanes x 16
// bytes, a row's inter-pass twiddle is read once for two elements, and everything that tells the eight rows apart is a constant:
// an immediate offset in LDS (34 padded rows), a workgroup-uniform 64-bit step in HBM.  A matrix row of an odd column count starts on
// 8 bytes, so the HBM side claims no more; the ragged last lane of such a row (one valid column) moves 8 bytes.
struct Pair { u64 a, b; };
typedef Pair __attribute__((aligned(16))) PairL;       // in LDS: tile rows are 128 bytes
constexpr u32 PAIR_ROWS = 8, PAIR_LDS_STEP = 34 * 8;     // rows per lane; pairs between them in a padded tile (32 rows + 2 spare)
__host__ __device__ constexpr u32 brev3(u32 i) { return ((i & 1) << 2) | (i & 2) | ((i >> 2) & 1); }

constexpr unsigned PASS_THREADS = 256, MID_THREADS = 512;      // workgroup budgets of ntt_pass_kernel / lde_mid_kernel: the planner sizes tiles by them

struct PassParams {
    const u64 *src; u64 *dst;
    const u64 *tw;                  // pow256 table of the transform's 2^32-th root (forward or inverse)
    const u64 *twK;                 // twK[j] = w_1024^j of the same direction (tile twiddles: w_(2^k)^j = twK[j << (10-k)])
    u64 C;                          // matrix columns
    u64 tStride, gStride, hiStride; // words between tile rows / slot groups / tiles along the outer index
    u64 scale;                      // 0: none; else every output is multiplied by it (1/N of an inverse transform)
    u32 k, logM, hasTw, dit;
    u32 Wc, nbT;                    // tile slots S = nbT*Wc : nbT adjacent groups x Wc columns
    u32 nColChunks, nGroupTiles;
    u32 walk;                       // column chunks a workgroup walks (walk_at's W; 1 outside the 16-slot instances)
    u32 n, scatter;                 // scatter: store row bitrev_n(g*2^k + t) (lo = 0 pass of a natural-order transform)
    u32 canonOut;                   // 1: this pass writes a transform's result (canonical values); 0: the next pass takes any representative
};

// KC = 0: any geometry; KC = 8: the geometry of the wide matrices (8 stages, SC = 15 or 16 column slots x 16 sub-transform lanes,
// one slot group), with every stride, LDS offset and twiddle index a compile-time constant.  16 slots: rows of 128 bytes and more, cut
// into 16-column chunks with a ragged last one (100 columns: 16 x 6 + 4).  15 slots: a 15-column matrix, whose rows are under 128
// bytes and take 7-stage passes, so no default plan reaches SC = 15 (enumerated over 2^0..2^30 rows x 1..200 columns, tests/golden/
// transform_plans.txt.gz); PIL2GL_NTT_KMAX=9 or 10 does, e.g. fft of 2^8 x 15 (one pass) and interpolate of 2^16 x 15 (DIT pass).
// The 16-slot fixed-geometry pass (8 stages, 16 column slots x 16 sub-transform lanes, one slot group: g = gt): the workgroup builds the
// tables of its row tile once and walks its column chunks (walk_at): load, tile write, stages, store, next chunk.  The tile moves in
// slot pairs (see Pair).  Only the first chunk's loads overlap anything of the workgroup's own (the tables): issuing chunk c+1's before
// chunk c's store costs 33 registers (147 / 153 / 156 against 114 / 121 / 124: a wave per SIMD), and the three other workgroups of
// the CU cover the latency.
template <bool INV, bool DIT>
__device__ __forceinline__ void pass_walk16(const PassParams &P, u64 *lds) {
    constexpr u32 K = 256, S = 16;
    const u32 x = threadIdx.x, y = threadIdx.y, tid = y * S + x;
    u64 *tile = lds, *TW = tile + S * (K + K / 16), *TWO = TW + K;
    u32 hi, gt, cc;
    walk_at(blockIdx.x, gridDim.x, 0, P.walk, P.nColChunks, P.nGroupTiles, hi, gt, cc);
    const u32 px = tid & 7, r = tid >> 3;
    // the lane's first row at slot pair px of chunk 0, in and out; a chunk is 16 words further, the lane's eight rows are rs / os apart
    const u64 in0 = (u64)hi * P.hiStride + (u64)gt * P.gStride + (u64)r * P.tStride + 2 * px, rs = P.tStride * 32;
    // row i of this lane goes to out0 + ord(i) * os, ord = i, or its 3-bit reversal where the pass scatters (tile row bits 5..7 are
    // the lowest three of the reversed index above the tile's own: bitrev_n(g*2^8 + r + 32 i) = bitrev_n(g*2^8 + r) + (brev3(i) << (n - 8)))
    u64 out0 = in0, os = rs;
    if (P.scatter) { out0 = (u64)bitrev32(gt * K + r, P.n) * P.C + 2 * px; os = P.C << (P.n - 8); }

    Pair vin2[PAIR_ROWS];
    // all eight loads of a chunk are in flight together; the ragged last lane of an odd-width row has one column, lanes beyond it none
    auto load = [&](u32 chunk) {
        const u64 c0 = (u64)chunk * 16 + 2 * px;
        // (the offset is made opaque: left alone the compiler works out the eight row addresses of every chunk once, ahead of the
        // loop, and keeps them in registers through the stages; this way it redoes the eight additions per chunk)
        u64 off = in0 + (u64)chunk * 16;
        asm volatile("" : "+v"(off));
        const u64 *sp = P.src + off;
#pragma unroll
        for (u32 i = 0; i < PAIR_ROWS; i++) vin2[i] = {0, 0};
        if (c0 + 1 < P.C) {
#pragma unroll
            for (u32 i = 0; i < PAIR_ROWS; i++) vin2[i] = *reinterpret_cast<const Pair *>(sp + i * rs);
        } else if (c0 < P.C) {
#pragma unroll
            for (u32 i = 0; i < PAIR_ROWS; i++) vin2[i].a = sp[i * rs];
        }
    };
    load(cc);                                       // the first chunk's latency overlaps the tables
    TW[tid] = P.twK[tid << 2];
    if (P.hasTw) {
        u64 v = root_pow(P.tw, P.logM, gt * bitrev32(tid, 8));
        if (P.scale) v = mul(v, P.scale);
        TWO[tid] = v;
    }
    __syncthreads();
    PairL *trow = reinterpret_cast<PairL *>(tile) + (r + (r >> 4)) * 8 + px;       // tile row r + 32*i: PAIR_LDS_STEP * i further
    for (u32 step = 0;;) {
        // (a lane reads back and rewrites only its own pairs of the tile, so no barrier stands between one chunk's store and the next
        // chunk's tile write; the stages end in one)
        if (DIT && P.hasTw) {
#pragma unroll
            for (u32 i = 0; i < PAIR_ROWS; i++) {
                const u64 w = TWO[r + 32 * i];
                PairL o; o.a = NTT_MUL(vin2[i].a, w); o.b = NTT_MUL(vin2[i].b, w);
                trow[i * PAIR_LDS_STEP] = o;
            }
        } else {
#pragma unroll
            for (u32 i = 0; i < PAIR_ROWS; i++) { PairL o; o.a = vin2[i].a; o.b = vin2[i].b; trow[i * PAIR_LDS_STEP] = o; }
        }
        __syncthreads();
        if (DIT) { dit_step<4, INV, true>(tile, TW, 8, 0, 4, S, x, y, 16); dit_step<4, INV, true>(tile, TW, 8, 4, 0, S, x, y, 16); }
        else { dif_step<4, INV, true>(tile, TW, 8, 8, S, x, y, 16); dif_step<4, INV, true>(tile, TW, 8, 4, S, x, y, 16); }

        const u64 c0 = (u64)cc * 16 + 2 * px;
        const bool v1 = c0 < P.C, v2 = c0 + 1 < P.C;
        u64 outOff = out0 + (u64)cc * 16;            // (opaque for the same reason)
        asm volatile("" : "+v"(outOff));
        u64 *dp = P.dst + outOff;
        u32 h2, g2, ccNext;
        const bool more = walk_at(blockIdx.x, gridDim.x, ++step, P.walk, P.nColChunks, P.nGroupTiles, h2, g2, ccNext);
        // what a value takes on its way out is the same for the whole launch: one loop per case, nothing decided per element
        auto put = [&](auto xf) {
            if (v2) {
#pragma unroll
                for (u32 i = 0; i < PAIR_ROWS; i++) {
                    Pair v; { const PairL l = trow[i * PAIR_LDS_STEP]; v.a = l.a; v.b = l.b; }
                    xf(v, i);
                    *reinterpret_cast<Pair *>(dp + (P.scatter ? brev3(i) : i) * os) = v;
                }
            } else if (v1) {
#pragma unroll
                for (u32 i = 0; i < PAIR_ROWS; i++) {
                    Pair v; v.a = reinterpret_cast<const u64 *>(trow + i * PAIR_LDS_STEP)[0]; v.b = 0;
                    xf(v, i);
                    dp[(P.scatter ? brev3(i) : i) * os] = v.a;
                }
            }
        };
        if (P.hasTw && !DIT) {
            if (P.canonOut) put([&](Pair &v, u32 i) { const u64 w = TWO[r + 32 * i]; v.a = mul(v.a, w); v.b = mul(v.b, w); });
            else put([&](Pair &v, u32 i) { const u64 w = TWO[r + 32 * i]; v.a = NTT_MUL(v.a, w); v.b = NTT_MUL(v.b, w); });
        } else if (!P.hasTw && P.scale) put([&](Pair &v, u32) { v.a = mul(v.a, P.scale); v.b = mul(v.b, P.scale); });
        else if (P.canonOut) put([&](Pair &v, u32) { v.a = canon(v.a); v.b = canon(v.b); });
        else put([&](Pair &, u32) {});
        if (!more) break;
        cc = ccNext;
        load(cc);
    }
}

template <bool INV, bool DIT, int KC, int SC = 16>
__global__ void __launch_bounds__(PASS_THREADS) ntt_pass_kernel(PassParams P) {
    extern __shared__ u64 lds[];
    if constexpr (KC == 8 && SC == 16) { pass_walk16<INV, DIT>(P, lds); return; }
    const u32 k = KC ? KC : P.k, K = 1u << k, S = KC ? SC : blockDim.x, by = KC ? 16 : blockDim.y;
    const u32 x = threadIdx.x, y = threadIdx.y, tid = y * S + x, nth = S * by;
    constexpr bool PAD = KC != 0;                   // one spare tile row per 16 (see dif_step)
    const u32 tileRows = PAD ? K + (K >> 4) : K;
    u64 *tile = lds, *TW = tile + (size_t)S * tileRows, *TWO = TW + K;
#define TROW(t_) (PAD ? (t_) + ((t_) >> 4) : (t_))

    u32 hi, gt, cc;                                 // one tile per workgroup
    walk_at(blockIdx.x, gridDim.x, 0, 1, P.nColChunks, P.nGroupTiles, hi, gt, cc);
    const u32 gi = KC ? 0 : x / P.Wc, ci = x - gi * P.Wc;
    const u64 c = (u64)cc * P.Wc + ci;
    const bool valid = c < P.C;
    // slot groups: adjacent blocks; in the scattering pass blocks nGroupTiles apart, whose bit-reversed rows are adjacent
    const u64 g = P.scatter ? (u64)gi * P.nGroupTiles + gt : (u64)gt * P.nbT + gi;
    const u64 base = (u64)hi * P.hiStride + g * P.gStride + c;

    // the first LOADB rows of this lane are requested before the tables are built, so that their latency overlaps it;
    // all loads of a batch are in flight together (one load per iteration would serialise the HBM latency)
    constexpr u32 LOADB = 16;
    u64 vin[LOADB];
#pragma unroll
    for (u32 i = 0; i < LOADB; i++) { const u32 t = y + i * by; vin[i] = (valid && t < K) ? P.src[base + (u64)t * P.tStride] : 0; }
    for (u32 j = tid; j < K; j += nth) TW[j] = P.twK[j << (10 - k)];
    if (P.hasTw) {
        for (u32 idx = tid; idx < (KC ? 1 : P.nbT) * K; idx += nth) {
            u32 b = gt * (KC ? 1 : P.nbT) + (idx >> k);
            u64 v = root_pow(P.tw, P.logM, b * bitrev32(idx & (K - 1), k));
            if (P.scale) v = mul(v, P.scale);
            TWO[idx] = v;
        }
    }
    __syncthreads();
    for (u32 t0 = y;;) {
#pragma unroll
        for (u32 i = 0; i < LOADB; i++) {
            const u32 t = t0 + i * by;
            if (t < K) {
                u64 v = vin[i];
                if (DIT && P.hasTw) v = NTT_MUL(v, TWO[gi * K + t]);
                tile[TROW(t) * S + x] = v;
            }
        }
        t0 += LOADB * by;
        if (t0 >= K) break;
#pragma unroll
        for (u32 i = 0; i < LOADB; i++) { const u32 t = t0 + i * by; vin[i] = (valid && t < K) ? P.src[base + (u64)t * P.tStride] : 0; }
    }
    __syncthreads();
    if constexpr (KC == 8) {
        if (DIT) { dit_step<4, INV, true>(tile, TW, 8, 0, 4, SC, x, y, 16); dit_step<4, INV, true>(tile, TW, 8, 4, 0, SC, x, y, 16); }
        else { dif_step<4, INV, true>(tile, TW, 8, 8, SC, x, y, 16); dif_step<4, INV, true>(tile, TW, 8, 4, SC, x, y, 16); }
    } else {
        if (DIT) dit_stages<INV>(tile, TW, k, S, x, y, by); else dif_stages<INV>(tile, TW, k, S, x, y, by);
    }
    if (!valid) return;
    for (u32 t = y; t < K; t += by) {
        u64 v = tile[TROW(t) * S + x];
        if (P.hasTw && !DIT) v = P.canonOut ? mul(v, TWO[gi * K + t]) : NTT_MUL(v, TWO[gi * K + t]);
        else if (!P.hasTw && P.scale) v = mul(v, P.scale);
        else if (P.canonOut) v = canon(v);
        u64 addr = P.scatter ? (u64)bitrev32((u32)(g * K + t), P.n) * P.C + c : base + (u64)t * P.tStride;
        P.dst[addr] = v;
    }
#undef TROW
}

struct LdeParams {
    const u64 *src; u64 *dst;
    const u64 *twi, *twf, *pow7;    // pow256 tables: inverse root, forward root, coset shift 7
    const u64 *twKi, *twKf;         // w_1024^-j, w_1024^j (tile twiddles)
    u64 C, ninv;
    u32 n, k, extBits;
    u32 canonOut;                   // 1: no pass follows (n <= k): the stored values are the result
    u32 cosetBegin, cosetCount;     // this call produces cosets [cosetBegin, cosetBegin+cosetCount) of the 2^extBits (multi-GPU: one slice per rank)
    u32 coefIn;                     // 1: src already holds COEFFICIENTS, coefficient m at row bitrev_n(m) (what the inverse passes + the stages below leave): no inverse stages here
    u32 Wc, G, nColChunks;
    u32 nTiles;                     // row tiles of the launch
};

// Finishes the iNTT on bits [0,k), scales by the coset factors and starts the forward NTT (see header).
// SC = 0: any geometry; SC > 0: 8 stages, SC column slots x 16 sub-transform lanes, one slot group (EPT = 16) -- the geometry
// of the wide matrices, with compile-time strides: 16 slots for 16 columns and more, 15 for a 15-column matrix of more than 2^8 rows
// (the mid kernel takes 8 stages there even though the passes around it take 7)
template <int EPT, int SC>
__global__ void __launch_bounds__(MID_THREADS) lde_mid_kernel(LdeParams P) {
    extern __shared__ u64 lds[];
    const u32 k = SC ? 8 : P.k, K = 1u << k, S = SC ? SC : blockDim.x, by = SC ? 16 : blockDim.y;
    const u32 x = threadIdx.x, y = threadIdx.y, tid = y * S + x, nth = S * by;
    constexpr bool PAD = SC != 0;                   // one spare tile row per 16 (see dif_step)
    const u32 tileRows = PAD ? K + (K >> 4) : K, rowStep = PAD ? by + 1 : by;      // rows y + i*by -> y + i*(by+1) when padded (by = 16)
    u64 *tile = lds, *TWi = tile + (size_t)S * tileRows, *TWf = TWi + K, *Sc = TWf + K, *Uc = Sc + (size_t)P.G * K;

    u32 hi, gt, cc;                                 // one tile per workgroup (hi = 0: the row blocks of the mid kernel are one run of tiles)
    walk_at(blockIdx.x, gridDim.x, 0, 1, P.nColChunks, P.nTiles, hi, gt, cc);
    const u32 gi = SC ? 0 : x / P.Wc, ci = x - gi * P.Wc;
    const u64 c = (u64)cc * P.Wc + ci;
    const bool valid = c < P.C;
    const u64 g = (u64)gt * (SC ? 1 : P.G) + gi;    // index of this slot's 2^k-row block
    const u64 base = g * K * P.C + c;

    // 16 slots: pairs of slots (see Pair), the lane's eight pairs of coefficients in registers over the cosets
    constexpr bool WIDE = SC == 16;
    const u32 px = tid & 7, r = tid >> 3;
    const u64 c0 = (u64)cc * 16 + 2 * px;
    const bool v1 = c0 < P.C, v2 = c0 + 1 < P.C;
    Pair coef2[PAIR_ROWS];
    PairL *trow = reinterpret_cast<PairL *>(tile) + (r + (r >> 4)) * 8 + px;       // tile row r + 32*i: PAIR_LDS_STEP * i further

    u64 coef[EPT];                                  // EPT >= K / by rows per lane (2, 4, 8 or 16): all loads in flight while the tables are built
    if constexpr (WIDE) {
#pragma unroll
        for (u32 i = 0; i < PAIR_ROWS; i++) coef2[i] = {0, 0};
        const u64 *sp = P.src + (g * K + r) * P.C + c0;
        const u64 rs = P.C * 32;
        if (v2) {
#pragma unroll
            for (u32 i = 0; i < PAIR_ROWS; i++) coef2[i] = *reinterpret_cast<const Pair *>(sp + i * rs);
        } else if (v1) {
#pragma unroll
            for (u32 i = 0; i < PAIR_ROWS; i++) coef2[i].a = sp[i * rs];
        }
    } else {
#pragma unroll
        for (int i = 0; i < EPT; i++) { const u32 t = y + i * by; coef[i] = (valid && t < K) ? P.src[base + (u64)t * P.C] : 0; }
    }
    for (u32 j = tid; j < K; j += nth) { TWi[j] = P.twKi[j << (10 - k)]; TWf[j] = P.twKf[j << (10 - k)]; }
    for (u32 idx = tid; idx < P.G * K; idx += nth) {
        u32 pos = (gt * P.G + (idx >> k)) * K + (idx & (K - 1));
        u32 m = bitrev32(pos, P.n);                 // this row holds coefficient m of the column polynomial
        Uc[idx] = root_pow(P.twf, P.n + P.extBits, m);   // w_E^m : step from coset j to j+1
        u64 s0 = P.pow7 ? mul(P.ninv, pow256(P.pow7, m)) : P.ninv;    // shift^m / N  (coset j = 0; shift 7, or 1 when pow7 is null)
        if (P.cosetBegin) s0 = mul(s0, root_pow(P.twf, P.n + P.extBits, m * P.cosetBegin));   // (w_E^m)^cosetBegin, m*cb < 2^(n+b)
        Sc[idx] = s0;
    }
    if (!P.coefIn) {                                // (uniform for the launch)
        if constexpr (WIDE) {
#pragma unroll
            for (u32 i = 0; i < PAIR_ROWS; i++) { PairL o; o.a = coef2[i].a; o.b = coef2[i].b; trow[i * PAIR_LDS_STEP] = o; }
        } else {
#pragma unroll
            for (int i = 0; i < EPT; i++) { const u32 t = y + i * by; if (t < K) tile[(y + i * rowStep) * S + x] = coef[i]; }
        }
        __syncthreads();
        if constexpr (SC != 0) { dif_step<4, true, true>(tile, TWi, 8, 8, SC, x, y, 16); dif_step<4, true, true>(tile, TWi, 8, 4, SC, x, y, 16); }
        else dif_stages<true>(tile, TWi, k, S, x, y, by);
        if constexpr (WIDE) {
#pragma unroll
            for (u32 i = 0; i < PAIR_ROWS; i++) { const PairL l = trow[i * PAIR_LDS_STEP]; coef2[i].a = l.a; coef2[i].b = l.b; }
        } else {
#pragma unroll
            for (int i = 0; i < EPT; i++) { u32 t = y + i * by; coef[i] = t < K ? tile[(y + i * rowStep) * S + x] : 0; }
        }
    }
    __syncthreads();
    const u32 nCosets = P.cosetCount;
    for (u32 j = 0; j < nCosets; j++) {
        if constexpr (WIDE) {
            // (the offsets are made opaque for the reason given below; the eight rows are then a uniform step apart)
            u64 dstOff = ((g * K + r) * P.cosetCount + j) * P.C + c0;
            u32 pairOff = (r + (r >> 4)) * 8 + px, scOff = r;
            asm volatile("" : "+v"(dstOff), "+v"(pairOff), "+v"(scOff));
            const u64 dstStep = (u64)32 * P.cosetCount * P.C;
            PairL *tp = reinterpret_cast<PairL *>(tile) + pairOff;
#pragma unroll
            for (u32 i = 0; i < PAIR_ROWS; i++) {
                const u64 sc = Sc[scOff + 32 * i];
                PairL o; o.a = NTT_MUL(coef2[i].a, sc); o.b = NTT_MUL(coef2[i].b, sc);
                tp[i * PAIR_LDS_STEP] = o;
            }
            __syncthreads();
            dit_step<4, false, true>(tile, TWf, 8, 0, 4, SC, x, y, 16); dit_step<4, false, true>(tile, TWf, 8, 4, 0, SC, x, y, 16);
            asm volatile("" : "+v"(dstOff), "+v"(pairOff));
            tp = reinterpret_cast<PairL *>(tile) + pairOff;
            u64 *dp = P.dst + dstOff;
            if (v2) {
                if (P.canonOut) {
#pragma unroll
                    for (u32 i = 0; i < PAIR_ROWS; i++) { const PairL l = tp[i * PAIR_LDS_STEP]; Pair v; v.a = canon(l.a); v.b = canon(l.b); *reinterpret_cast<Pair *>(dp + i * dstStep) = v; }
                } else {
#pragma unroll
                    for (u32 i = 0; i < PAIR_ROWS; i++) { const PairL l = tp[i * PAIR_LDS_STEP]; Pair v; v.a = l.a; v.b = l.b; *reinterpret_cast<Pair *>(dp + i * dstStep) = v; }
                }
            } else if (v1) {
#pragma unroll
                for (u32 i = 0; i < PAIR_ROWS; i++) { const u64 v = reinterpret_cast<const u64 *>(tp + i * PAIR_LDS_STEP)[0]; dp[i * dstStep] = P.canonOut ? canon(v) : v; }
            }
        } else {
        // the per-row offsets do not depend on j: left alone the compiler computes them all once and keeps ~4 registers per
        // row alive across the loop; the opaque copies make it redo the few additions in every coset instead
        u64 dstOff = ((g * K + y) * P.cosetCount + j) * P.C + c;
        u32 tileOff = y * S + x, scOff = gi * K + y;
        asm volatile("" : "+v"(dstOff), "+v"(tileOff), "+v"(scOff));
        const u64 dstStep = (u64)by * P.cosetCount * P.C;
#pragma unroll
        for (int i = 0; i < EPT; i++) { u32 t = y + i * by; if (t < K) tile[tileOff + i * rowStep * S] = NTT_MUL(coef[i], Sc[scOff + i * by]); }
        __syncthreads();
        if constexpr (SC != 0) { dit_step<4, false, true>(tile, TWf, 8, 0, 4, SC, x, y, 16); dit_step<4, false, true>(tile, TWf, 8, 4, 0, SC, x, y, 16); }
        else dit_stages<false>(tile, TWf, k, S, x, y, by);
        asm volatile("" : "+v"(dstOff), "+v"(tileOff));
        if (valid) {
#pragma unroll
            for (int i = 0; i < EPT; i++) {
                u32 t = y + i * by;
                if (t < K) { const u64 v = tile[tileOff + i * rowStep * S]; P.dst[dstOff + i * dstStep] = P.canonOut ? canon(v) : v; }
            }
        }
        }
        for (u32 idx = tid; idx < P.G * K; idx += nth) Sc[idx] = mul(Sc[idx], Uc[idx]);
        __syncthreads();
    }
}

__global__ void copy_rows_kernel(const u64 *src, u64 *dst, u64 nWords) {
    u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < nWords) dst[i] = src[i];
}
__global__ void broadcast_row_kernel(const u64 *src, u64 *dst, u64 C, u64 rows) {
    u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < rows * C) dst[i] = src[i % C];
}

// ---------------------------------------------------------------- host-side planning
// plan_ntt / plan_lde decide every launch of a transform as plain values, without touching a device; ntt_launch / lde_launch
// run what they planned.  pil2gl_debug_plan_transform shows the same plan to the tests.
using namespace pil2gl;

constexpr u32 TILE_WORDS = 4096;       // u64 words of a tile in LDS (32 KiB), beside its twiddle / scale tables

// test hooks: reach pass sizes and kernel families the default plan does not.  Read once per call, here only.
struct PlanOptions {
    u32 kmax;           // PIL2GL_NTT_KMAX: stages per pass (1..10) instead of the 8 / 7 of pick_kmax; 0 = not set
    bool generic;       // PIL2GL_NTT_GENERIC=1: the any-geometry instances where the fixed-geometry ones would run
    bool wideFwd;       // PIL2GL_LDE_WIDEFWD=0: the forward passes of a narrow interpolate keep the narrow matrix's 7 stages
};
PlanOptions plan_options() {
    PlanOptions o = {0, false, true};
    if (const char *s = getenv("PIL2GL_NTT_KMAX")) o.kmax = std::min<u32>(10, std::max<u32>(1, (u32)atoi(s)));
    if (const char *s = getenv("PIL2GL_NTT_GENERIC")) o.generic = atoi(s) != 0;
    if (const char *s = getenv("PIL2GL_LDE_WIDEFWD")) o.wideFwd = atoi(s) != 0;
    return o;
}

u32 pow2floor(u64 v) { u32 r = 1; while ((u64)r * 2 <= v) r *= 2; return r; }

struct Geom { u32 Wc, nbT, nColChunks, S, by; };
// tile slots for 2^k rows: at most maxElems u64 in LDS, S*by = up to nThreads threads
Geom make_geom(u32 k, u64 C, u64 totalGroups, u32 maxElems, u32 nThreads) {
    Geom g;
    u32 smax = std::min<u32>(256, std::max<u32>(1, maxElems >> k));
    if (C <= smax) {
        g.Wc = (u32)C;
        g.nbT = (u32)std::min<u64>(pow2floor(smax / C), totalGroups);
        g.nColChunks = 1;
    } else {
        u32 chunks = (u32)((C + smax - 1) / smax);
        g.Wc = (u32)((C + chunks - 1) / chunks);
        // 8-stage tiles have fixed-geometry kernels: chunks of 16 with a ragged last chunk beat evenly cut chunks on the any-geometry
        // kernels (81 columns: 16 x 5 + 1 instead of 14 x 5 + 11: -11 %), and 16 beats 15 where both give the same number of chunks
        // (100 columns, 16 x 6 + 4 against 15 x 6 + 10: 194.7 against 198.1 ms per config-3 interpolate; profiles/r05_lde_chunks_15_16.txt)
        if (k == 8 && smax == 16) g.Wc = 16;
        g.nbT = 1;
        g.nColChunks = (u32)((C + g.Wc - 1) / g.Wc);
    }
    g.S = g.Wc * g.nbT;
    u32 nSub = 1u << (k - next_chunk(k));          // sub-transforms per column in the widest register step
    g.by = std::max<u32>(1, std::min<u32>(nThreads / g.S, nSub));
    return g;
}

// The fixed-geometry rule: a tile of 8 stages, 15 or 16 slots x 16 sub-transform lanes, one slot group runs the instances whose
// strides are compile-time constants.  -> the slot count, or 0 for the any-geometry instances.
// One slot group (nbT == 1) makes S == Wc, so the chunk width needs no test of its own; and an 8-stage tile has 16 sub-transforms per
// column, so by = min(threads / S, 16) is 16 at 15 or 16 slots under either thread budget (256 / 16 = 16, 512 / 16 = 32): the pass
// kernels, the mid kernel and the planners' probes all get the same answer from the same geometry.  With 4096-word tiles that is
// 16 slots for 16 columns and more (chunks of 16) and 15 slots for 15 columns; narrower matrices pack several slot groups.
u32 fixed_slots(u32 k, const Geom &g, const PlanOptions &o) {
    return !o.generic && k == 8 && g.nbT == 1 && g.by == 16 && (g.S == 15 || g.S == 16) ? g.S : 0;
}
// would an 8-stage tile of a 2^n x C matrix (n > 8) run a fixed-geometry instance?
bool fixed_at_8(u32 n, u64 C, const PlanOptions &o) { return fixed_slots(8, make_geom(8, C, 1ull << (n - 8), TILE_WORDS, PASS_THREADS), o) != 0; }

// stages per pass: a tile row is S*8 contiguous bytes and S <= 256 / 2^(k-4), so 8 stages keep 128-byte segments for
// wide matrices; narrow ones (rows under 128 bytes) take 7 so that adjacent rows fill the segment
u32 pick_kmax(u64 C, const PlanOptions &o) { return o.kmax ? o.kmax : C * 8 >= 128 ? 8 : 7; }

enum LaunchKind : u32 { PASS_INV_DIF = 0, PASS_FWD_DIF = 1, PASS_DIT = 2, MID = 3 };
// one kernel launch of a transform
struct Launch {
    u32 kind;
    u32 lo, k;              // the launch works on index bits [lo, lo+k)
    Geom g;
    u32 fixedSlots;         // 0: any-geometry instance; 15 / 16: the fixed-geometry instance of that many slots
    u32 ept;                // mid: the rows-per-lane instance (lde_mid_kernel<EPT, ..>); passes: 0
    u32 ldsBytes, blocks;   // blocks: the tiles of the launch, row tiles x column chunks
    u32 groupTiles;         // row tiles per outer index (passes above bit 0: 2^lo / slot groups; else all of them)
    u32 walk, grid;         // a workgroup walks up to `walk` column chunks of its row tile (walk_at): `grid` workgroups take the `blocks` tiles
    u32 scatter, canonOut;  // passes: PassParams of the same names; mid: canonOut = no pass follows
};
constexpr int MAX_LAUNCHES = 64;           // 2 x 30 one-stage passes and the mid kernel at most
struct Plan { Launch l[MAX_LAUNCHES]; int n = 0; };

constexpr size_t MAX_LDS_BYTES = 160 * 1024;
int check_launch(const Launch &L, u64 blocks) {
    if (blocks > 0x7fffffffull) return fail(PIL2GL_EINVAL, "grid too large");
    if (L.ldsBytes > MAX_LDS_BYTES) return fail(PIL2GL_EINVAL, "tile needs %u bytes of LDS (>160 KiB)", L.ldsBytes);
    return PIL2GL_OK;
}

// How many column chunks a workgroup of the launch walks.  The 16-slot fixed-geometry instances build their per-row-tile tables once per
// workgroup, so the longer the run the less of that work is repeated; but the chip wants several workgroups per CU slot, so a launch
// that has 4 x 256 tiles keeps at least that many workgroups: with R = ceil(1024 / rowTiles) runs wanted per row tile, W =
// floor(nColChunks / R) leaves at least R (2^24 rows: R = 1, a workgroup takes its whole row of chunks, 7 of 100 columns and 50 of 800).
// Where that comes to one chunk, two are taken if the grid still holds 1024 or never could (a launch that cannot fill the chip is a few
// microseconds either way).  The mid kernel and every other instance keep one tile per workgroup (the mid kernel's tables serve eight
// cosets already, and walking costs it 18 registers: 182, a wave per SIMD).
constexpr u32 WALK_MIN_GRID = 4 * 256;
void plan_walk(Launch &L, u64 rowTiles) {
    const u32 nc = L.g.nColChunks;
    L.walk = 1;
    if (L.fixedSlots == 16 && L.kind != MID) {
        const u64 R = (WALK_MIN_GRID + rowTiles - 1) / rowTiles;
        if (R <= nc) L.walk = (u32)(nc / R);
        if (L.walk == 1 && nc >= 2 && (rowTiles * nc < WALK_MIN_GRID || walk_grid(rowTiles, 2, nc) >= WALK_MIN_GRID)) L.walk = 2;
    }
    L.grid = (u32)walk_grid(rowTiles, L.walk, nc);
}

// One pass over index bits [lo, lo+k) of a 2^n x C matrix.
int plan_pass(Plan &p, u32 kind, u64 C, u32 n, u32 lo, u32 k, bool scatter, bool canonOut, const PlanOptions &o) {
    Launch &L = p.l[p.n++];
    L.kind = kind; L.lo = lo; L.k = k; L.ept = 0; L.scatter = scatter; L.canonOut = canonOut;
    const u64 totalGroups = lo > 0 ? 1ull << lo : 1ull << (n - k), nHi = lo > 0 ? 1ull << (n - lo - k) : 1, K = 1ull << k;
    L.g = make_geom(k, C, totalGroups, TILE_WORDS, PASS_THREADS);
    L.fixedSlots = fixed_slots(k, L.g, o);
    // tile (one spare row per 16 in the fixed geometry) + tile twiddles + the inter-pass twiddles of every slot group
    L.ldsBytes = (u32)(8 * ((size_t)L.g.S * (L.fixedSlots ? K + K / 16 : K) + K + (lo > 0 ? (size_t)L.g.nbT * K : 0)));
    const u64 blocks = nHi * (totalGroups / L.g.nbT) * L.g.nColChunks;
    L.blocks = (u32)blocks;
    L.groupTiles = (u32)(totalGroups / L.g.nbT);
    plan_walk(L, nHi * L.groupTiles);
    return check_launch(L, blocks);
}

// split `bits` into ceil(bits/kmax) nearly equal passes
int split_bits(u32 bits, u32 kmax, u32 *ks) {
    if (bits == 0) return 0;
    u32 np = (bits + kmax - 1) / kmax, base = bits / np, extra = bits % np;
    for (u32 i = 0; i < np; i++) ks[i] = base + (i < extra ? 1 : 0);
    return (int)np;
}

// fft / ifft of a 2^n x C matrix: decimation in frequency from the top bits down; the last pass scatters to natural order.
// Where the 8-bit pass has its fixed-geometry kernel as many passes as possible take 8 bits and ONE takes the remainder, if that is at
// least 4 bits: 2^20 x 100 in 8,8,4 instead of 7,7,6 -17 %, 2^22 in 8,8,6 instead of 8,7,7 -5 %; a remainder of 1..3 bits (a whole sweep
// for almost no arithmetic) stays balanced: 2^26 in 8,8,8,2 loses 8 % (profiles/r05_lde_mid8_planner.txt)
int plan_ntt(u32 n, u64 C, bool inverse, const PlanOptions &o, Plan &p) {
    p.n = 0;
    if (C == 0 || n == 0) return PIL2GL_OK;         // (n = 0: a copy)
    const u32 kmax = pick_kmax(C, o), r = n & 7;
    u32 ks[32];
    int np = 0;
    if (kmax == 8 && n > 16 && (r == 0 || r >= 4) && fixed_at_8(n, C, o)) {
        for (u32 i = 0; i < n / 8; i++) ks[np++] = 8;
        if (r) ks[np++] = r;
    } else np = split_bits(n, kmax, ks);
    u32 lo = n;
    for (int i = 0; i < np; i++) {
        lo -= ks[i];
        P2_TRY(plan_pass(p, inverse ? PASS_INV_DIF : PASS_FWD_DIF, C, n, lo, ks[i], i == np - 1, i == np - 1, o));
    }
    return PIL2GL_OK;
}

// interpolate / extend of a 2^n x C matrix onto cosetCount of the 2^extBits cosets (0: all of them); coefIn: the input holds
// coefficients already (row bitrev(m) = coefficient m), so no inverse stage runs.
//  1. iNTT, decimation in frequency, bits [kf, n) from the top down
//  2. mid kernel: the last kf iNTT stages + coset scaling + the first kf NTT stages
//  3. the remaining forward stages, decimation in time, bits [kf, n) from the bottom up, on dst viewed as N x (C * cosets)
int plan_lde(u32 n, u64 C, u32 extBits, u32 cosetCount, bool coefIn, const PlanOptions &o, Plan &p) {
    p.n = 0;
    if (C == 0 || n == 0) return PIL2GL_OK;         // (n = 0: a broadcast)
    if (cosetCount == 0) cosetCount = 1u << extBits;
    // a narrow matrix (rows under 128 bytes) whose extension is wide takes 8-stage passes on that side
    const u32 kmax = pick_kmax(C, o), kmaxF = o.wideFwd ? std::max(kmax, pick_kmax(C * cosetCount, o)) : kmax;
    const u32 nfp = (n + kmaxF - 1) / kmaxF;
    u32 kf = (n + nfp - 1) / nfp;       // bits done by the mid kernel (both directions)
    // The balanced split gives the mid kernel 6 or 7 bits whenever n is not 8 * passes (n = 17..21, 25..29): its fixed-geometry form
    // (coefficients in registers over the cosets) is worth more than balance -- 8-17 % of an interpolate at 2^17..2^28 rows x 16 / 32 /
    // 64 / 100 columns, full extensions and single cosets alike (profiles/r05_lde_mid8_planner.txt); widths whose tiles are not 15 or
    // 16 slots keep the balanced split (20 columns lose 2-4 % with 8)
    if (kf < 8 && n > 8 && kmaxF == 8 && fixed_at_8(n, C, o)) kf = 8;
    u32 ks[32];
    if (!coefIn) {
        const int np = split_bits(n - kf, kmax, ks);
        u32 lo = n;
        for (int i = 0; i < np; i++) { lo -= ks[i]; P2_TRY(plan_pass(p, PASS_INV_DIF, C, n, lo, ks[i], false, false, o)); }
    }
    {
        Launch &L = p.l[p.n++];
        L.kind = MID; L.lo = 0; L.k = kf; L.scatter = 0; L.canonOut = n > kf ? 0 : 1;
        const u64 totalGroups = 1ull << (n - kf), K = 1ull << kf;
        // LDS = tile (S*K, one spare row per 16 in the fixed geometry) + two tile twiddle tables (K) + coset scale tables (2*G*K); narrow
        // matrices (small C => many slot groups per tile) are dominated by the scale tables: halve the tile until it fits 96 KiB
        for (u32 words = TILE_WORDS;; words /= 2) {
            L.g = make_geom(kf, C, totalGroups, words, MID_THREADS);
            L.fixedSlots = fixed_slots(kf, L.g, o);
            L.ldsBytes = (u32)(8 * ((size_t)L.g.S * (L.fixedSlots ? K + K / 16 : K) + 2 * K + 2 * (size_t)L.g.nbT * K));
            if (L.ldsBytes <= 96 * 1024 || L.g.nbT == 1) break;
        }
        // rows per lane: K / by = 2^(stages of the widest register step) = 2, 4, 8 or 16 -- by always reaches the sub-transform count,
        // as 512 threads cover it at every tile the LDS holds
        const u32 need = (u32)((K + L.g.by - 1) / L.g.by);
        L.ept = L.fixedSlots ? 16 : need <= 2 ? 2 : need <= 4 ? 4 : need <= 8 ? 8 : 16;
        if (need > 16) return fail(PIL2GL_EINVAL, "lde tile too tall for the thread block (need %u rows per thread)", need);
        const u64 blocks = (totalGroups / L.g.nbT) * L.g.nColChunks;
        L.blocks = (u32)blocks;
        L.groupTiles = (u32)(totalGroups / L.g.nbT);
        plan_walk(L, L.groupTiles);
        P2_TRY(check_launch(L, blocks));
    }
    const int np = split_bits(n - kf, kmaxF, ks);
    u32 lo = kf;
    for (int i = 0; i < np; i++) { P2_TRY(plan_pass(p, PASS_DIT, C * cosetCount, n, lo, ks[i], false, i == np - 1, o)); lo += ks[i]; }
    return PIL2GL_OK;
}

// ---------------------------------------------------------------- launching a plan
int set_lds(const void *fn, size_t bytes) {
    if (bytes > 48 * 1024) HIP_TRY(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    return PIL2GL_OK;
}

// a planned pass on a 2^n x C matrix; scale: 0, or the factor every output takes (1/N of an inverse transform)
int launch_pass(const Launch &L, const u64 *src, u64 *dst, u64 C, u32 n, u64 scale, hipStream_t st) {
    const bool inverse = L.kind == PASS_INV_DIF;
    const u32 lo = L.lo, k = L.k;
    PassParams P;
    P.src = src; P.dst = dst; P.canonOut = L.canonOut;
    P.tw = inverse ? tables().powWi : tables().powW;
    P.twK = inverse ? tables().tw1024i : tables().tw1024;
    P.C = C; P.scale = scale; P.k = k; P.logM = lo + k; P.hasTw = lo > 0; P.dit = L.kind == PASS_DIT; P.n = n; P.scatter = L.scatter;
    if (lo > 0) { P.tStride = (C << lo); P.gStride = C; P.hiStride = (C << (lo + k)); }
    else { P.tStride = C; P.gStride = (C << k); P.hiStride = 0; }
    P.Wc = L.g.Wc; P.nbT = L.g.nbT; P.nColChunks = L.g.nColChunks; P.nGroupTiles = L.groupTiles; P.walk = L.walk;
    const dim3 grid(L.grid), block(L.g.S, L.g.by);
#define PASS_CASE(INV_, DIT_)                                                                             \
    switch (L.fixedSlots) {                                                                               \
    case 16: P2_TRY(set_lds((const void *)ntt_pass_kernel<INV_, DIT_, 8, 16>, L.ldsBytes));                \
             hipLaunchKernelGGL((ntt_pass_kernel<INV_, DIT_, 8, 16>), grid, block, L.ldsBytes, st, P); break; \
    case 15: P2_TRY(set_lds((const void *)ntt_pass_kernel<INV_, DIT_, 8, 15>, L.ldsBytes));                \
             hipLaunchKernelGGL((ntt_pass_kernel<INV_, DIT_, 8, 15>), grid, block, L.ldsBytes, st, P); break; \
    default: P2_TRY(set_lds((const void *)ntt_pass_kernel<INV_, DIT_, 0>, L.ldsBytes));                    \
             hipLaunchKernelGGL((ntt_pass_kernel<INV_, DIT_, 0>), grid, block, L.ldsBytes, st, P); }
    switch (L.kind) {
    case PASS_DIT: PASS_CASE(false, true) break;
    case PASS_INV_DIF: PASS_CASE(true, false) break;
    default: PASS_CASE(false, false)
    }
#undef PASS_CASE
    KERNEL_CHECK();
    return PIL2GL_OK;
}

int launch_mid(const Launch &L, LdeParams &P, hipStream_t st) {
    P.k = L.k; P.canonOut = L.canonOut; P.Wc = L.g.Wc; P.G = L.g.nbT; P.nColChunks = L.g.nColChunks;
    P.nTiles = L.groupTiles;
    const dim3 grid(L.grid), block(L.g.S, L.g.by);
#define LDE_CASE(E_)                                                                              \
    if (!L.fixedSlots && L.ept == E_) {                                                           \
        P2_TRY(set_lds((const void *)lde_mid_kernel<E_, 0>, L.ldsBytes));                          \
        hipLaunchKernelGGL((lde_mid_kernel<E_, 0>), grid, block, L.ldsBytes, st, P);               \
    } else
#define LDE_FIXED(S_)                                                                             \
    if (L.fixedSlots == S_) {                                                                     \
        P2_TRY(set_lds((const void *)lde_mid_kernel<16, S_>, L.ldsBytes));                         \
        hipLaunchKernelGGL((lde_mid_kernel<16, S_>), grid, block, L.ldsBytes, st, P);              \
    } else
    LDE_FIXED(15) LDE_FIXED(16)
    LDE_CASE(2) LDE_CASE(4) LDE_CASE(8) LDE_CASE(16)
    { return fail(PIL2GL_EINVAL, "no lde_mid_kernel instance of %u rows per lane", L.ept); }
#undef LDE_CASE
#undef LDE_FIXED
    KERNEL_CHECK();
    return PIL2GL_OK;
}

}  // namespace

namespace pil2gl {

int ntt_launch(const u64 *src, u64 C, u32 n, u64 *dst, bool inverse, hipStream_t st) {
    if (C == 0) return PIL2GL_OK;
    if (n == 0) {
        if (src != dst) HIP_TRY(hipMemcpyAsync(dst, src, C * 8, hipMemcpyDeviceToDevice, st));
        return PIL2GL_OK;
    }
    Plan p;
    P2_TRY(plan_ntt(n, C, inverse, plan_options(), p));
    const u64 N = 1ull << n, scale = inverse ? h_inv(N % 0xFFFFFFFF00000001ull) : 0;
    u64 *tmp = nullptr;                             // src -> tmp, in place there, -> dst
    if (p.n > 1) P2_TRY(scratch(SCR_NTT_TMP, N * C, &tmp));
    for (int i = 0; i < p.n; i++) P2_TRY(launch_pass(p.l[i], i == 0 ? src : tmp, i == p.n - 1 ? dst : tmp, C, n, i == 0 ? scale : 0, st));
    return PIL2GL_OK;
}

int lde_launch(const u64 *src, u64 C, u32 n, u64 *dst, u32 nExt, hipStream_t st, u32 cosetBegin, u32 cosetCount, u64 *work, bool unitShift, bool coefIn) {
    if (C == 0) return PIL2GL_OK;
    const u32 eb = nExt - n;
    if (cosetCount == 0) { cosetBegin = 0; cosetCount = 1u << eb; }
    if (n == 0) {                       // constant polynomial: every coset point evaluates to it
        broadcast_row_kernel<<<(unsigned)(((u64)cosetCount * C + 255) / 256), 256, 0, st>>>(src, dst, C, cosetCount);
        KERNEL_CHECK();
        return PIL2GL_OK;
    }
    Plan p;
    P2_TRY(plan_lde(n, C, eb, cosetCount, coefIn, plan_options(), p));
    const u64 N = 1ull << n;
    const u64 *coef = src;              // what the mid kernel reads
    u64 *tmp = work;                    // the inverse passes: src -> tmp, then in place (the caller's workspace may be src itself)
    if (p.l[0].kind == PASS_INV_DIF && !tmp) P2_TRY(scratch(SCR_NTT_TMP, N * C, &tmp));
    for (int i = 0; i < p.n; i++) {
        const Launch &L = p.l[i];
        if (L.kind == PASS_INV_DIF) { P2_TRY(launch_pass(L, coef, tmp, C, n, 0, st)); coef = tmp; }
        else if (L.kind == PASS_DIT) P2_TRY(launch_pass(L, dst, dst, C * cosetCount, n, 0, st));
        else {
            LdeParams P;
            P.src = coef; P.dst = dst; P.twi = tables().powWi; P.twf = tables().powW; P.twKi = tables().tw1024i; P.twKf = tables().tw1024; P.pow7 = unitShift ? nullptr : tables().pow7;
            P.C = C; P.ninv = coefIn ? 1 : h_inv(N % 0xFFFFFFFF00000001ull); P.n = n; P.extBits = eb; P.coefIn = coefIn ? 1 : 0;
            P.cosetBegin = cosetBegin; P.cosetCount = cosetCount;
            P2_TRY(launch_mid(L, P, st));
        }
    }
    return PIL2GL_OK;
}

}  // namespace pil2gl

using namespace pil2gl;

static int check_ntt_args(const void *src, const void *dst, uint32_t nBits, uint32_t nBitsExt) {
    if (!src || !dst) return fail(PIL2GL_EINVAL, "null buffer");
    // the reference's transforms take any nBits <= 32 (f3g.js:40, fft.js:39-50); here row indices, twiddle exponents and grid sizes are
    // 32-bit quantities that have been checked to 2^30 rows (four passes of 8/8/7/7 stages; 2^30 x 1 column is 8.6 GB each way)
    if (nBits > PIL2GL_MAX_NTT_BITS || nBitsExt > PIL2GL_MAX_NTT_BITS) return fail(PIL2GL_EINVAL, "domain of 2^%u rows is not supported (max 2^%d)", nBits > nBitsExt ? nBits : nBitsExt, PIL2GL_MAX_NTT_BITS);
    if (nBitsExt < nBits) return fail(PIL2GL_EINVAL, "nBitsExt (%u) < nBits (%u)", nBitsExt, nBits);
    return PIL2GL_OK;
}

// a coset slice only ever indexes 2^nBits * cosetCount local rows: the full extension may be larger than one device holds
// ---- the reference's worker-level operators (fft_worker.js:6-67), for a caller that keeps fft_p.js's own block loop ----------------
// The product path never runs these (pil2gl_fft / _interpolate replace the whole loop: bit reversal, blocks and transposes); they
// exist so that `pool.exec("fft_block", ...)` / `("interpolatePrepareBlock", ...)` have a device twin with the same arguments.
// One launch per stage, twiddles straight from the pow256 table.
//
// _fft_block (fft_worker.js:21-60) on a buffer of 2^blockBits rows that sits at row start_pos of an n-row transform: the recursion
// first cuts the block into pieces of 2^layers rows (:30-34), then runs a decimation-in-time transform of `layers` stages on each
// piece (:35-38); stage l = 1..layers pairs rows 2^(l-1) apart inside sub-blocks of 2^l rows and is the recursion level whose
// (s, blockBits, layers) are (s - layers + l, l, l).  Its twiddle for pair i of the sub-block at absolute row sp (:40-58):
//   w = w0 * F.w[l]^i,   w0 = F.w[s - layers + l]^p  if s > layers, else 1,   width = 2^(s - layers), height = n / width,
//   p = (sp % height) * width + floor(sp / height)
// (s > layers and width are the same at every level: s and the level's block size fall together.)
namespace {
__global__ void fft_block_stage_kernel(u64 *__restrict__ buf, u64 startPos, u64 nPols, u32 nBits, u32 s, u32 layers, u32 l, u64 nPairs,
                                       const u64 *__restrict__ powW) {
    const u64 idx = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= nPairs * nPols) return;
    const u64 g = idx / nPols, c = idx - g * nPols;
    const u64 half = 1ull << (l - 1), i = g & (half - 1), rel = (g >> (l - 1)) << l;
    u64 w = root_pow(powW, l, (u32)i);
    if (s > layers) {
        const u32 sl = s - layers + l, wBits = s - layers;               // sl <= s <= 32
        const u64 sp = startPos + rel, hBits = nBits - wBits;             // height = 2^hBits rows
        const u64 pe = ((sp & ((1ull << hBits) - 1)) << wBits) + (sp >> hBits);
        w = mul(w, root_pow(powW, sl, (u32)(pe & ((1ull << sl) - 1))));   // the root has order 2^sl
    }
    u64 *a = buf + (rel + i) * nPols + c, *b = buf + (rel + half + i) * nPols + c;
    const u64 u = canon(*a), t = mul(w, *b);
    *a = add(u, t);
    *b = sub(u, t);
}
// interpolatePrepareBlock (fft_worker.js:6-19): row i of the block times start * inc^i
__global__ void interpolate_prepare_block_kernel(u64 *__restrict__ buf, u64 width, u64 height, u64 start, u64 inc) {
    const u64 idx = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= width * height) return;
    buf[idx] = mul(buf[idx], mul(start, pow(inc, idx / width)));
}
}  // namespace

static int check_coset_args(const void *src, const void *dst, uint32_t nBits, uint32_t nBitsExt, uint32_t cosetBegin, uint32_t cosetCount) {
    if (!src || !dst) return fail(PIL2GL_EINVAL, "null buffer");
    if (nBitsExt < nBits) return fail(PIL2GL_EINVAL, "nBitsExt (%u) < nBits (%u)", nBitsExt, nBits);
    if (nBits > PIL2GL_MAX_NTT_BITS || nBitsExt > 31) return fail(PIL2GL_EINVAL, "domain of 2^%u rows (extended 2^%u) is not supported", nBits, nBitsExt);
    if (cosetCount == 0 || (uint64_t)cosetBegin + cosetCount > (1ull << (nBitsExt - nBits))) return fail(PIL2GL_EINVAL, "coset range [%u,%u) outside 2^%u", cosetBegin, cosetBegin + cosetCount, nBitsExt - nBits);
    if (((uint64_t)cosetCount << nBits) > (1ull << PIL2GL_MAX_NTT_BITS)) return fail(PIL2GL_EINVAL, "slice of %u cosets x 2^%u rows exceeds 2^%d local rows", cosetCount, nBits, PIL2GL_MAX_NTT_BITS);
    return PIL2GL_OK;
}

extern "C" {

// test hooks (host only, no device): the launches ntt_launch / lde_launch make for this call, under the environment's test hooks, and how
// those launches walk their column chunks
namespace {
int plan_for_debug(uint32_t op, uint32_t nBits, uint64_t nPols, uint32_t nBitsExt, uint32_t cosetCount, Plan &p) {
    if (op > PIL2GL_PLAN_EXTEND_COEFS) return fail(PIL2GL_EINVAL, "unknown transform %u", op);
    if (nBits > PIL2GL_MAX_NTT_BITS || nBitsExt < nBits || nBitsExt - nBits > 31) return fail(PIL2GL_EINVAL, "nBits %u, nBitsExt %u", nBits, nBitsExt);
    if (op <= PIL2GL_PLAN_IFFT) return plan_ntt(nBits, nPols, op == PIL2GL_PLAN_IFFT, plan_options(), p);
    return plan_lde(nBits, nPols, nBitsExt - nBits, cosetCount, op == PIL2GL_PLAN_EXTEND_COEFS, plan_options(), p);
}
struct WalkShape { u32 grid, walk, rowTiles, nGroupTiles, nColChunks; };
// what launch_pass / launch_mid hand walk_at for this launch
WalkShape walk_shape(const Launch &L) {
    return {L.grid, L.walk, L.blocks / L.g.nColChunks, L.groupTiles, L.g.nColChunks};
}
}  // namespace

int pil2gl_debug_plan_transform(uint32_t op, uint32_t nBits, uint64_t nPols, uint32_t nBitsExt, uint32_t cosetCount,
                                uint32_t *out, uint32_t maxLaunches, uint32_t *nLaunches) {
    if (!nLaunches || (!out && maxLaunches)) return fail(PIL2GL_EINVAL, "null argument");
    Plan p;
    P2_TRY(plan_for_debug(op, nBits, nPols, nBitsExt, cosetCount, p));
    *nLaunches = (uint32_t)p.n;
    if ((uint32_t)p.n > maxLaunches) return fail(PIL2GL_EINVAL, "%d launches, room for %u", p.n, maxLaunches);
    for (int i = 0; i < p.n; i++) {
        const Launch &L = p.l[i];
        const uint32_t r[PIL2GL_PLAN_LAUNCH_WORDS] = {L.kind, L.lo, L.k, L.g.Wc, L.g.nbT, L.g.nColChunks, L.g.S, L.g.by, L.fixedSlots, L.ept,
                                                      L.ldsBytes, L.blocks, L.scatter, L.canonOut};
        for (int j = 0; j < PIL2GL_PLAN_LAUNCH_WORDS; j++) out[i * PIL2GL_PLAN_LAUNCH_WORDS + j] = r[j];
    }
    return PIL2GL_OK;
}

int pil2gl_debug_plan_transform_grid(uint32_t op, uint32_t nBits, uint64_t nPols, uint32_t nBitsExt, uint32_t cosetCount,
                                     uint32_t *out, uint32_t maxLaunches, uint32_t *nLaunches) {
    if (!nLaunches || (!out && maxLaunches)) return fail(PIL2GL_EINVAL, "null argument");
    Plan p;
    P2_TRY(plan_for_debug(op, nBits, nPols, nBitsExt, cosetCount, p));
    *nLaunches = (uint32_t)p.n;
    if ((uint32_t)p.n > maxLaunches) return fail(PIL2GL_EINVAL, "%d launches, room for %u", p.n, maxLaunches);
    for (int i = 0; i < p.n; i++) {
        const WalkShape w = walk_shape(p.l[i]);
        const uint32_t r[PIL2GL_PLAN_GRID_WORDS] = {w.grid, w.walk, w.rowTiles, w.nGroupTiles, w.nColChunks};
        for (int j = 0; j < PIL2GL_PLAN_GRID_WORDS; j++) out[i * PIL2GL_PLAN_GRID_WORDS + j] = r[j];
    }
    return PIL2GL_OK;
}

int pil2gl_debug_transform_walk(uint32_t op, uint32_t nBits, uint64_t nPols, uint32_t nBitsExt, uint32_t cosetCount, uint32_t launch,
                                uint32_t firstBlock, uint32_t count, uint32_t *out) {
    if (!out) return fail(PIL2GL_EINVAL, "null argument");
    Plan p;
    P2_TRY(plan_for_debug(op, nBits, nPols, nBitsExt, cosetCount, p));
    if (launch >= (uint32_t)p.n) return fail(PIL2GL_EINVAL, "launch %u of %d", launch, p.n);
    const WalkShape w = walk_shape(p.l[launch]);
    if ((uint64_t)firstBlock + count > w.grid) return fail(PIL2GL_EINVAL, "workgroups [%u, +%u) of %u", firstBlock, count, w.grid);
    for (uint32_t b = 0; b < count; b++)
        for (uint32_t s = 0; s < w.walk; s++) {
            uint32_t *o = out + ((size_t)b * w.walk + s) * 3;
            if (!walk_at(firstBlock + b, w.grid, s, w.walk, w.nColChunks, w.nGroupTiles, o[0], o[1], o[2])) o[0] = o[1] = o[2] = 0xffffffffu;
        }
    return PIL2GL_OK;
}

int pil2gl_debug_transform_walk_cover(uint32_t op, uint32_t nBits, uint64_t nPols, uint32_t nBitsExt, uint32_t cosetCount, uint32_t launch,
                                      uint64_t *counts) {
    if (!counts) return fail(PIL2GL_EINVAL, "null argument");
    Plan p;
    P2_TRY(plan_for_debug(op, nBits, nPols, nBitsExt, cosetCount, p));
    if (launch >= (uint32_t)p.n) return fail(PIL2GL_EINVAL, "launch %u of %d", launch, p.n);
    const Launch &L = p.l[launch];
    const WalkShape w = walk_shape(L);
    uint64_t *seen = (uint64_t *)calloc(((size_t)L.blocks + 63) / 64, 8);
    if (!seen) return fail(PIL2GL_EINVAL, "out of memory");
    uint64_t once = 0, extra = 0;
    for (uint32_t b = 0; b < w.grid; b++) {
        uint32_t hi, gt, cc;
        for (uint32_t s = 0; walk_at(b, w.grid, s, w.walk, w.nColChunks, w.nGroupTiles, hi, gt, cc); s++) {
            const uint64_t rowTile = (uint64_t)hi * w.nGroupTiles + gt, cell = rowTile * w.nColChunks + cc;
            if (gt >= w.nGroupTiles || rowTile >= w.rowTiles || (seen[cell >> 6] >> (cell & 63) & 1)) { extra++; continue; }
            seen[cell >> 6] |= 1ull << (cell & 63);
            once++;
        }
    }
    free(seen);
    counts[0] = once; counts[1] = L.blocks - once; counts[2] = extra;
    return PIL2GL_OK;
}

int pil2gl_interpolate_dev(const uint64_t *src, uint64_t nPols, uint32_t nBits, uint64_t *dst, uint32_t nBitsExt, void *stream) {
    P2_TRY(ensure_init());
    P2_TRY(check_ntt_args(src, dst, nBits, nBitsExt));
    return lde_launch(src, nPols, nBits, dst, nBitsExt, as_stream(stream), 0, 0, nullptr, false);
}
int pil2gl_interpolate_cosets_dev(const uint64_t *src, uint64_t nPols, uint32_t nBits, uint64_t *dst, uint32_t nBitsExt,
                                  uint32_t cosetBegin, uint32_t cosetCount, void *stream) {
    P2_TRY(ensure_init());
    P2_TRY(check_coset_args(src, dst, nBits, nBitsExt, cosetBegin, cosetCount));
    return lde_launch(src, nPols, nBits, dst, nBitsExt, as_stream(stream), cosetBegin, cosetCount, nullptr, false);
}
// the same slice of the PLAIN extension (evaluations on w_E^j <w_N>, no coset shift): rows (pos << b) + j of fft_E applied to
// the zero-padded coefficients of the columns -- how computeQStark extends its split quotient (stark_gen_helpers.js:192)
int pil2gl_extend_cosets_unshifted_dev(const uint64_t *src, uint64_t nPols, uint32_t nBits, uint64_t *dst, uint32_t nBitsExt,
                                       uint32_t cosetBegin, uint32_t cosetCount, void *stream) {
    P2_TRY(ensure_init());
    P2_TRY(check_coset_args(src, dst, nBits, nBitsExt, cosetBegin, cosetCount));
    return lde_launch(src, nPols, nBits, dst, nBitsExt, as_stream(stream), cosetBegin, cosetCount, nullptr, true);
}
// The evaluations, on the UNSHIFTED domain of 2^nBitsExt points in natural order, of polynomials handed over as COEFFICIENTS:
// coefBrev is a 2^nBits x nPols matrix whose row bitrev(m) holds coefficient m (the order the inverse passes leave, and the one
// pil2gl_compute_q_split_brev_dev writes) -- fft of the zero-padded coefficient matrix (stark_gen_helpers.js:192) without the
// 2^nBitsExt-row padded input and without its first nBitsExt - nBits stages.
int pil2gl_extend_coefs_brev_dev(const uint64_t *coefBrev, uint64_t nPols, uint32_t nBits, uint64_t *dst, uint32_t nBitsExt, void *stream) {
    P2_TRY(ensure_init());
    P2_TRY(check_ntt_args(coefBrev, dst, nBits, nBitsExt));
    return lde_launch(coefBrev, nPols, nBits, dst, nBitsExt, as_stream(stream), 0, 0, nullptr, true, true);
}
int pil2gl_extend_coefs_brev_cosets_dev(const uint64_t *coefBrev, uint64_t nPols, uint32_t nBits, uint64_t *dst, uint32_t nBitsExt,
                                        uint32_t cosetBegin, uint32_t cosetCount, void *stream) {
    P2_TRY(ensure_init());
    P2_TRY(check_coset_args(coefBrev, dst, nBits, nBitsExt, cosetBegin, cosetCount));
    return lde_launch(coefBrev, nPols, nBits, dst, nBitsExt, as_stream(stream), cosetBegin, cosetCount, nullptr, true, true);
}
int pil2gl_interpolate_cosets_ws_dev(const uint64_t *src, uint64_t nPols, uint32_t nBits, uint64_t *dst, uint32_t nBitsExt,
                                     uint32_t cosetBegin, uint32_t cosetCount, uint64_t *workspace, void *stream) {
    P2_TRY(ensure_init());
    P2_TRY(check_coset_args(src, dst, nBits, nBitsExt, cosetBegin, cosetCount));
    if (!workspace) return fail(PIL2GL_EINVAL, "null workspace");
    return lde_launch(src, nPols, nBits, dst, nBitsExt, as_stream(stream), cosetBegin, cosetCount, workspace, false);
}
int pil2gl_fft_dev(const uint64_t *src, uint64_t nPols, uint32_t nBits, uint64_t *dst, void *stream) {
    P2_TRY(ensure_init());
    P2_TRY(check_ntt_args(src, dst, nBits, nBits));
    return ntt_launch(src, nPols, nBits, dst, false, as_stream(stream));
}
int pil2gl_ifft_dev(const uint64_t *src, uint64_t nPols, uint32_t nBits, uint64_t *dst, void *stream) {
    P2_TRY(ensure_init());
    P2_TRY(check_ntt_args(src, dst, nBits, nBits));
    return ntt_launch(src, nPols, nBits, dst, true, as_stream(stream));
}

static int host_wrap(const uint64_t *src, uint64_t nPols, uint32_t nBits, uint64_t *dst, uint32_t nBitsOut, int mode) {
    P2_TRY(ensure_init());
    P2_TRY(check_ntt_args(src, dst, nBits, nBitsOut));
    uint64_t nIn = (nPols << nBits), nOut = (nPols << nBitsOut);
    if (nIn == 0) return PIL2GL_OK;
    // device copies: up to 1 GiB each they live in persistent slots (a caller looping over BigBuffers of one size -- the
    // reference's extendAndMerkelize does -- pays the allocations once); larger ones are allocated and freed per call
    const uint64_t keepWords = 1ull << 27;
    const bool keepIn = nIn <= keepWords, keepOut = nOut <= keepWords;
    uint64_t *dIn = nullptr, *dOut = nullptr;
    if (keepIn) P2_TRY(scratch(SCR_HOST_NTT_IN, nIn, &dIn)); else HIP_TRY(hipMalloc((void **)&dIn, nIn * 8));
    int rc = PIL2GL_OK;
    if (keepOut) rc = scratch(SCR_HOST_NTT_OUT, nOut, &dOut);
    else { hipError_t e = hipMalloc((void **)&dOut, nOut * 8); if (e != hipSuccess) rc = hip_fail(e, "hipMalloc(dst)"); }
    hipError_t e = hipSuccess;
    if (rc == PIL2GL_OK) { e = hipMemcpy(dIn, src, nIn * 8, hipMemcpyHostToDevice); if (e != hipSuccess) rc = hip_fail(e, "hipMemcpy H2D"); }
    if (rc == PIL2GL_OK) rc = mode == 0 ? lde_launch(dIn, nPols, nBits, dOut, nBitsOut, 0, 0, 0, nullptr, false) : ntt_launch(dIn, nPols, nBits, dOut, mode == 2, 0);
    if (rc == PIL2GL_OK) { e = hipMemcpy(dst, dOut, nOut * 8, hipMemcpyDeviceToHost); if (e != hipSuccess) rc = hip_fail(e, "hipMemcpy D2H"); }
    if (!keepIn) (void)hipFree(dIn);
    if (!keepOut && dOut) (void)hipFree(dOut);
    return rc;
}
int pil2gl_interpolate(const uint64_t *src, uint64_t nPols, uint32_t nBits, uint64_t *dst, uint32_t nBitsExt) { return host_wrap(src, nPols, nBits, dst, nBitsExt, 0); }
int pil2gl_fft(const uint64_t *src, uint64_t nPols, uint32_t nBits, uint64_t *dst) { return host_wrap(src, nPols, nBits, dst, nBits, 1); }
int pil2gl_ifft(const uint64_t *src, uint64_t nPols, uint32_t nBits, uint64_t *dst) { return host_wrap(src, nPols, nBits, dst, nBits, 2); }

// fft_block(buff, start_pos, nPols, nBits, s, blockBits, layers)  fft_worker.js:62-67: buf = the 2^blockBits x nPols block, in place
int pil2gl_fft_block_dev(uint64_t *buf, uint64_t start_pos, uint64_t nPols, uint32_t nBits, uint32_t s, uint32_t blockBits, uint32_t layers, void *stream) {
    P2_TRY(ensure_init());
    // (the reference checks nothing; what is refused here has no meaning there either: F.w has 33 entries, :30-38 never end for
    // layers > blockBits, and n / width is not an integer for s - layers > nBits)
    if (nBits > 32 || s > 32 || blockBits > 32) return fail(PIL2GL_EINVAL, "fft_block: nBits %u, s %u, blockBits %u", nBits, s, blockBits);
    if (layers > blockBits) return fail(PIL2GL_EINVAL, "fft_block: %u layers in a block of 2^%u rows", layers, blockBits);
    if (s > layers && s - layers > nBits) return fail(PIL2GL_EINVAL, "fft_block: stage %u with %u layers in a transform of 2^%u rows", s, layers, nBits);
    if (layers == 0 || nPols == 0) return PIL2GL_OK;                      // (:30-34 cut the block down to single rows: nothing to pair)
    if (!buf) return fail(PIL2GL_EINVAL, "null buffer");
    const u64 nPairs = 1ull << (blockBits - 1);
    if (nPols > (1ull << 40) / nPairs) return fail(PIL2GL_EINVAL, "fft_block: block too large");
    const u64 blocks = (nPairs * nPols + 255) / 256;
    if (blocks > 0x7fffffffull) return fail(PIL2GL_EINVAL, "fft_block: grid too large");
    hipStream_t st = as_stream(stream);
    for (u32 l = 1; l <= layers; l++) {
        fft_block_stage_kernel<<<(unsigned)blocks, 256, 0, st>>>(buf, start_pos, nPols, nBits, s, layers, l, nPairs, tables().powW);
        KERNEL_CHECK();
    }
    return PIL2GL_OK;
}
// interpolatePrepareBlock(buff, width, start, inc, st_i, st_n)  fft_worker.js:6-19: buf = height x width, in place
int pil2gl_interpolate_prepare_block_dev(uint64_t *buf, uint64_t width, uint64_t height, uint64_t start, uint64_t inc, void *stream) {
    P2_TRY(ensure_init());
    if (width == 0 || height == 0) return PIL2GL_OK;
    if (!buf) return fail(PIL2GL_EINVAL, "null buffer");
    if (height > (1ull << 40) / width) return fail(PIL2GL_EINVAL, "interpolatePrepareBlock: block too large");
    const u64 blocks = (width * height + 255) / 256;
    if (blocks > 0x7fffffffull) return fail(PIL2GL_EINVAL, "interpolatePrepareBlock: grid too large");
    interpolate_prepare_block_kernel<<<(unsigned)blocks, 256, 0, as_stream(stream)>>>(buf, width, height, start % P, inc % P);
    KERNEL_CHECK();
    return PIL2GL_OK;
}

}  // extern "C"
