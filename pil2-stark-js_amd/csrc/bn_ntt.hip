// Multi-column NTT over the BN254 scalar field Fr, gfx950: the device twin of src/helpers/fft/fft_p.bn128.js:178-285 (fft, ifft,
// interpolate) and of the worker loop it drives (fft_worker.bn128.js:6-67).  Elements are 32 bytes, Montgomery form (bn_field.cuh), the
// matrix is row-major: element (row j, polynomial i) at byte (j*nPols + i)*32.  Inputs are canonical (< r); so are the outputs.
//
// A transform of N = 2^n rows is S = ceil(n / 10) SWEEPS over global memory (bnp::bn_ntt_plan).  Sweep s works on the sub-transforms of
// 2^m rows that the sweeps before it left (m = n minus their layers) and takes the K most significant of their m index bits: a workgroup
// loads the tile of 2^K rows q * 2^(m-K) + n2 (q = 0..2^K-1) of one sub-transform, for a group of neighbouring columns, into LDS, runs K
// decimation-in-frequency layers there (a' = a + b, b' = (a - b) w_{2^(t+1)}^j for the layer of distance 2^t; the distance-1 layer has no
// product) and, unless it is the last sweep, multiplies row q by the seam twiddle w_{2^m}^(n2 brev_K(q)) -- once per element, not once per
// butterfly -- before it writes the tile back to the rows it came from.  After the last sweep row p of the working buffer holds the
// output of index brev_n(p): the last sweep stores its rows there, so the bit reversal is that sweep's store pattern and no pass of its
// own.  ifft is the same with the inverse roots, and n^-1 rides on the last sweep's stores.
//
// Buffers: one sweep reads src and writes dst (a workgroup reads its whole tile before it writes, and no other workgroup touches those
// rows and columns: dst may be src).  With more sweeps the first reads src and writes a scratch buffer, the middle ones work there in
// place, the last reads it and scatters to dst -- dst may be src again.
//
// Twiddles.  In the tile: w[10]^i, i < 512 (the layer of distance 2^t reads entry j << (9 - t)): 16 KB per direction, L1-resident.  At the
// seams: w[n]^E for any E < 2^n as lo[E mod 2^ceil(n/2)] * hi[E >> ceil(n/2)], one product of two table entries; both tables are built
// on the host on first use of a size (bn_params.cpp) and kept.  No exponentiation on the device.
//
// LDS: the tile as two planes of 16-byte halves (plane h, element e at h*2048 + e), e = q*cg + c.  Lanes take consecutive (j, c): a layer's
// a-operands, and its b-operands, are runs of 2^t * cg consecutive 16-byte slots with gaps of the same length, so a wave's ds_read_b128 /
// ds_write_b128 are conflict-free on runs of a lane group or more and two-way at worst -- there is no power-of-two stride between lanes
// to pad away.  Global accesses are two 16-byte halves per element with the half as the fastest lane index: a wave covers whole rows of the
// column group.
#include "common.h"
#include "bn_consts.h"
#include "bn_params.h"
#include "bn_field.cuh"
#include <string.h>
#include <map>
#include <vector>

using namespace pil2gl;
using bn::u32;

namespace {

using namespace bnc;
constexpr int NTT_THREADS = 512;
constexpr u32 PLANE = BN_NTT_TILE_ELEMS;             // 16-byte slots per plane
constexpr size_t NTT_LDS_BYTES = (size_t)2 * PLANE * 16;

struct SweepParams {
    const uint4 *src; uint4 *dst;
    const uint4 *twTile;                             // w[10]^i or its inverse, i < 512
    const uint4 *twLo, *twHi;                        // seam tables of this size and direction (not read by the last sweep)
    u64 nPols;
    u32 n, m, K, CG, nCG, loBits;
    u32 last, scale;                                 // last sweep: scatter to bit-reversed rows;  scale: times ninv on the way
    u32 ninv[8];
};

__device__ __forceinline__ void ld_elem(const uint4 *lds, u32 e, u32 x[8]) {
    const uint4 a = lds[e], b = lds[PLANE + e];
    x[0] = a.x; x[1] = a.y; x[2] = a.z; x[3] = a.w; x[4] = b.x; x[5] = b.y; x[6] = b.z; x[7] = b.w;
}
__device__ __forceinline__ void st_elem(uint4 *lds, u32 e, const u32 x[8]) {
    lds[e] = make_uint4(x[0], x[1], x[2], x[3]);
    lds[PLANE + e] = make_uint4(x[4], x[5], x[6], x[7]);
}
__device__ __forceinline__ void ld_table(const uint4 *__restrict__ t, u32 i, u32 x[8]) {
    const uint4 a = t[2 * (size_t)i], b = t[2 * (size_t)i + 1];
    x[0] = a.x; x[1] = a.y; x[2] = a.z; x[3] = a.w; x[4] = b.x; x[5] = b.y; x[6] = b.z; x[7] = b.w;
}
__device__ __forceinline__ u32 brev_bits(u32 x, u32 bits) { return bits ? __brev(x) >> (32 - bits) : 0u; }

__global__ void __launch_bounds__(NTT_THREADS) bn_ntt_sweep_kernel(SweepParams P) {
    extern __shared__ __attribute__((aligned(16))) uint4 tile[];
    const u32 K = P.K, rows = 1u << K, sub = P.m - K;
    const u32 cgi = blockIdx.x % P.nCG;
    const u64 tix = blockIdx.x / P.nCG;
    const u64 c0 = (u64)cgi * P.CG;
    const u32 cg = (u32)(P.nPols - c0 < P.CG ? P.nPols - c0 : P.CG);     // the last group may be narrower
    const u64 n2 = tix & ((1ull << sub) - 1), blk = tix >> sub;
    const u64 rowBase = (blk << P.m) + n2;                                // tile row q is row rowBase + (q << sub)
    const u32 elems = rows * cg;

    for (u32 i = threadIdx.x; i < 2 * elems; i += NTT_THREADS) {
        const u32 h = i & 1, e = i >> 1, q = e / cg, c = e - q * cg;
        tile[h * PLANE + e] = P.src[((rowBase + ((u64)q << sub)) * P.nPols + c0 + c) * 2 + h];
    }
    __syncthreads();

    const u32 nbf = (rows >> 1) * cg;
    for (int t = (int)K - 1; t >= 0; t--) {
        for (u32 bf = threadIdx.x; bf < nbf; bf += NTT_THREADS) {
            const u32 pi = bf / cg, c = bf - pi * cg, j = pi & ((1u << t) - 1), q0 = ((pi >> t) << (t + 1)) | j;
            const u32 e0 = q0 * cg + c, e1 = e0 + (cg << t);
            u32 a[8], b[8], d[8];
            ld_elem(tile, e0, a); ld_elem(tile, e1, b);
#pragma unroll
            for (int l = 0; l < 8; l++) d[l] = a[l];
            bn::fr_add(a, b);
            bn::fr_sub(d, b);
            if (t > 0) {                                                  // (the distance-1 layer's twiddle is 1)
                u32 w[8];
                ld_table(P.twTile, j << (BN_NTT_KMAX - 1 - t), w);
                bn::fr_mul(d, d, w);
            }
            st_elem(tile, e0, a); st_elem(tile, e1, d);
        }
        __syncthreads();
    }

    if (!P.last || P.scale) {
        for (u32 e = threadIdx.x; e < elems; e += NTT_THREADS) {
            u32 x[8], f[8];
            if (P.last) {
#pragma unroll
                for (int l = 0; l < 8; l++) f[l] = P.ninv[l];
            } else {                                                      // w[m]^(n2 k1) = w[n]^E
                const u32 q = e / cg;
                const u32 E = (u32)((n2 * brev_bits(q, K)) << (P.n - P.m));
                u32 lo[8], hi[8];
                ld_table(P.twLo, E & ((1u << P.loBits) - 1), lo); ld_table(P.twHi, E >> P.loBits, hi);
                bn::fr_mul(f, lo, hi);
            }
            ld_elem(tile, e, x);
            bn::fr_mul(x, x, f);
            st_elem(tile, e, x);
        }
        __syncthreads();
    }

    const u32 rest = P.n - K;                                            // last sweep: tile row q of block blk is output row brev(q) 2^rest + brev(blk)
    const u64 outLow = P.last ? brev_bits((u32)blk, rest) : 0;
    for (u32 i = threadIdx.x; i < 2 * elems; i += NTT_THREADS) {
        const u32 h = i & 1, e = i >> 1, q = e / cg, c = e - q * cg;
        const u64 row = P.last ? ((u64)brev_bits(q, K) << rest) + outLow : rowBase + ((u64)q << sub);
        P.dst[(row * P.nPols + c0 + c) * 2 + h] = tile[h * PLANE + e];
    }
}

// ---------------------------------------------------------------- tables
struct SeamTables { uint4 *lo = nullptr, *hi = nullptr; };
struct NttTables { uint4 *tile[2] = { nullptr, nullptr }; SeamTables seam[2][BN_NTT_MAX_BITS + 1]; };
std::map<int, NttTables> g_tabs;                    // by device: a device's tables stay valid for it

int upload_elems(const std::vector<bnp::U256> &v, uint4 **out) {
    void *d = nullptr;
    HIP_TRY(hipMalloc(&d, v.size() * 32));
    const hipError_t e = hipMemcpy(d, v.data(), v.size() * 32, hipMemcpyHostToDevice);
    if (e != hipSuccess) { (void)hipFree(d); return hip_fail(e, "BN128 transform table upload"); }
    *out = (uint4 *)d;
    return PIL2GL_OK;
}

// the tables a transform of 2^n rows needs in direction inv, built on first use and kept for the device they were made on
int get_tables(u32 n, int inv, u32 nSweeps, const uint4 **tile, SeamTables *seam, u32 *loBits) {
    std::lock_guard<std::recursive_mutex> lk(runtime_lock());
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    NttTables &g_tab = g_tabs[dev];
    const bnp::BnNttConsts &C = bnp::bn_ntt_consts();
    if (!g_tab.tile[inv]) {
        std::vector<bnp::U256> v((size_t)1 << (BN_NTT_KMAX - 1));
        bnp::bn_powers(inv ? C.wi[BN_NTT_KMAX] : C.w[BN_NTT_KMAX], v.size(), v.data());
        P2_TRY(upload_elems(v, &g_tab.tile[inv]));
    }
    *tile = g_tab.tile[inv];
    *loBits = (n + 1) / 2;
    *seam = SeamTables();
    if (nSweeps > 1) {
        SeamTables &S = g_tab.seam[inv][n];
        if (!S.lo) {
            const size_t nLo = (size_t)1 << *loBits, nHi = (size_t)1 << (n - *loBits);
            std::vector<bnp::U256> v(nLo + nHi);
            const bnp::U256 g = inv ? C.wi[n] : C.w[n];
            bnp::bn_powers(g, nLo, v.data());
            bnp::bn_powers(bnp::bn_mont_mul(v[nLo - 1], g), nHi, v.data() + nLo);      // g^(2^loBits)
            uint4 *d = nullptr;
            P2_TRY(upload_elems(v, &d));
            S.lo = d; S.hi = d + 2 * nLo;
        }
        *seam = S;
    }
    return PIL2GL_OK;
}

// ---------------------------------------------------------------- launching
int bn_ntt_launch(const u64 *src, u64 nPols, u32 n, u64 *dst, bool inverse, hipStream_t st) {
    if (nPols == 0) return PIL2GL_OK;
    if (n == 0) {
        if (src != dst) HIP_TRY(hipMemcpyAsync(dst, src, nPols * 32, hipMemcpyDeviceToDevice, st));
        return PIL2GL_OK;
    }
    unsigned layers[BN_NTT_MAX_SWEEPS];
    const int S = bnp::bn_ntt_plan(n, layers);
    if (S < 1) return fail(PIL2GL_EINVAL, "no plan for 2^%u rows", n);
    SweepParams P;
    SeamTables seam;
    P2_TRY(get_tables(n, inverse ? 1 : 0, (u32)S, &P.twTile, &seam, &P.loBits));
    P.twLo = seam.lo; P.twHi = seam.hi;
    u64 *work = nullptr;
    if (S > 1) P2_TRY(scratch(SCR_BN_NTT_TMP, (nPols << n) * 4, &work));
    HIP_TRY(hipFuncSetAttribute((const void *)bn_ntt_sweep_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)NTT_LDS_BYTES));
    memcpy(P.ninv, bnp::bn_ntt_consts().ninv[n].w, 32);
    P.nPols = nPols; P.n = n;
    u32 m = n;
    for (int s = 0; s < S; s++) {
        const u32 K = layers[s];
        const u64 cap = BN_NTT_TILE_ELEMS >> K;
        P.K = K; P.m = m; P.CG = (u32)(nPols < cap ? nPols : cap); P.nCG = (u32)((nPols + P.CG - 1) / P.CG);
        P.last = s == S - 1; P.scale = P.last && inverse;
        P.src = (const uint4 *)(s == 0 ? src : work); P.dst = (uint4 *)(P.last ? dst : work);
        const u64 blocks = ((1ull << n) >> K) * P.nCG;
        if (blocks > 0x7fffffffull) return fail(PIL2GL_EINVAL, "grid too large (2^%u rows x %llu columns)", n, (unsigned long long)nPols);
        bn_ntt_sweep_kernel<<<(unsigned)blocks, NTT_THREADS, NTT_LDS_BYTES, st>>>(P);
        KERNEL_CHECK();
        m -= K;
    }
    return PIL2GL_OK;
}

// fft_p.bn128.js:225-285: coefficients (already times 1/n, :265-266) to dstCoefs, zero rows up to 2^nBitsExt, one forward transform of that
// size, no coset shift (fft_worker.bn128.js:15-22 multiplies every row by the same 1/n).  Built as written: the padded matrix and the plain fft.
int bn_interpolate_launch(const u64 *src, u64 nPols, u32 n, u64 *dstCoefs, u64 *dst, u32 nExt, hipStream_t st) {
    if (nPols == 0) return PIL2GL_OK;
    const u64 nIn = (nPols << n) * 4, nOut = (nPols << nExt) * 4;
    P2_TRY(bn_ntt_launch(src, nPols, n, dst, true, st));
    if (dstCoefs) HIP_TRY(hipMemcpyAsync(dstCoefs, dst, nIn * 8, hipMemcpyDeviceToDevice, st));
    if (nOut > nIn) HIP_TRY(hipMemsetAsync(dst + nIn, 0, (nOut - nIn) * 8, st));
    return bn_ntt_launch(dst, nPols, nExt, dst, false, st);
}

int check_args(const void *src, const void *dst, uint64_t nPols, uint32_t nBits, uint32_t nBitsExt) {
    if (!src || !dst) return fail(PIL2GL_EINVAL, "null buffer");
    if (nBits > BN_NTT_MAX_BITS || nBitsExt > BN_NTT_MAX_BITS) return fail(PIL2GL_EINVAL, "domain of 2^%u rows: Fr has roots of unity up to 2^%u", nBits > nBitsExt ? nBits : nBitsExt, BN_NTT_MAX_BITS);
    if (nBitsExt < nBits) return fail(PIL2GL_EINVAL, "nBitsExt (%u) < nBits (%u)", nBitsExt, nBits);
    if (nPols >> (56 - nBitsExt)) return fail(PIL2GL_EINVAL, "matrix too large");
    return PIL2GL_OK;
}
int check_dev_ptrs(const void *src, const void *dst, const void *coefs) {
    if (((uintptr_t)src | (uintptr_t)dst | (uintptr_t)coefs) & 15) return fail(PIL2GL_EINVAL, "device buffers must be 16-byte aligned");
    return PIL2GL_OK;
}

}  // namespace

extern "C" {

uint32_t pil2gl_debug_bn128_fft_tile_bytes(void) { return (uint32_t)NTT_LDS_BYTES; }

int pil2gl_debug_bn128_fft_plan(uint32_t nBits, uint32_t *layersPerSweep, uint32_t room, uint32_t *nSweeps) {
    if (!nSweeps || (!layersPerSweep && room)) return fail(PIL2GL_EINVAL, "null argument");
    unsigned layers[BN_NTT_MAX_SWEEPS];
    const int S = bnp::bn_ntt_plan(nBits, layers);
    if (S < 0) return fail(PIL2GL_EINVAL, "domain of 2^%u rows: Fr has roots of unity up to 2^%u", nBits, BN_NTT_MAX_BITS);
    *nSweeps = (uint32_t)S;
    if ((uint32_t)S > room) return fail(PIL2GL_EINVAL, "%d sweeps, room for %u", S, room);
    for (int i = 0; i < S; i++) layersPerSweep[i] = layers[i];
    return PIL2GL_OK;
}

int pil2gl_bn128_fft_dev(const uint64_t *src, uint64_t nPols, uint32_t nBits, uint64_t *dst, void *stream) {
    P2_TRY(check_args(src, dst, nPols, nBits, nBits));
    P2_TRY(ensure_init());
    P2_TRY(check_dev_ptrs(src, dst, nullptr));
    return bn_ntt_launch(src, nPols, nBits, dst, false, as_stream(stream));
}
int pil2gl_bn128_ifft_dev(const uint64_t *src, uint64_t nPols, uint32_t nBits, uint64_t *dst, void *stream) {
    P2_TRY(check_args(src, dst, nPols, nBits, nBits));
    P2_TRY(ensure_init());
    P2_TRY(check_dev_ptrs(src, dst, nullptr));
    return bn_ntt_launch(src, nPols, nBits, dst, true, as_stream(stream));
}
int pil2gl_bn128_interpolate_dev(const uint64_t *src, uint64_t nPols, uint32_t nBits, uint64_t *dstCoefs, uint64_t *dst, uint32_t nBitsExt, void *stream) {
    P2_TRY(check_args(src, dst, nPols, nBits, nBitsExt));
    P2_TRY(ensure_init());
    P2_TRY(check_dev_ptrs(src, dst, dstCoefs));
    return bn_interpolate_launch(src, nPols, nBits, dstCoefs, dst, nBitsExt, as_stream(stream));
}

// ---- host-pointer forms: staged through device copies ----
static int host_transform(const uint64_t *src, uint64_t nPols, uint32_t nBits, uint64_t *dstCoefs, uint64_t *dst, uint32_t nBitsExt, int mode) {
    P2_TRY(check_args(src, dst, nPols, nBits, nBitsExt));
    const uint64_t nIn = (nPols << nBits) * 4, nOut = (nPols << nBitsExt) * 4, nCoef = dstCoefs ? nIn : 0;
    Stage s(nIn + nOut + nCoef);
    P2_TRY(s.rc());
    if (nIn == 0) return PIL2GL_OK;
    const uint64_t *dIn = s.put(src, nIn);
    uint64_t *dOut = s.take(nOut), *dCoef = nCoef ? s.take(nCoef) : nullptr;
    P2_TRY(s.rc());
    P2_TRY(mode == 2 ? bn_interpolate_launch(dIn, nPols, nBits, dCoef, dOut, nBitsExt, 0) : bn_ntt_launch(dIn, nPols, nBits, dOut, mode == 1, 0));
    if (dCoef) P2_TRY(s.get(dstCoefs, dCoef, nCoef));
    return s.get(dst, dOut, nOut);
}
int pil2gl_bn128_fft(const uint64_t *src, uint64_t nPols, uint32_t nBits, uint64_t *dst) { return host_transform(src, nPols, nBits, nullptr, dst, nBits, 0); }
int pil2gl_bn128_ifft(const uint64_t *src, uint64_t nPols, uint32_t nBits, uint64_t *dst) { return host_transform(src, nPols, nBits, nullptr, dst, nBits, 1); }
int pil2gl_bn128_interpolate(const uint64_t *src, uint64_t nPols, uint32_t nBits, uint64_t *dstCoefs, uint64_t *dst, uint32_t nBitsExt) {
    return host_transform(src, nPols, nBits, dstCoefs, dst, nBitsExt, 2);
}

}  // extern "C"
