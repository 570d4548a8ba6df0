// The recursion witness on the device, gfx950: the step that turns a circom witness into the trace of a compressor or of the final
// circuit -- compressorExec (src/compressor/compressor_exec.js:5-32) over Goldilocks, the loop of src/final/main_final_exec.js:50-67
// over the BN254 scalar field Fr.  Two steps, both bit-exact to the reference's loops:
//   additions   w[nWitness + i] = w[a_i] ca_i + w[b_i] cb_i, i in order.  The host sorts them by dependency level (wtns_plan.h); a launch
//               per level, a lane per addition, grid-stride.  The record (a, b, dst, source position) is one 16-byte load and the two
//               coefficients follow the same order, so both are read coalesced; the two operand reads are gathers.
//   gather      dst[i dstCols + j] = (s = sMap[i nCols + j]) ? w[s] : 0 for j < nCols, 0 for nCols <= j < dstCols (the widening rule of
//               land_rows).  Goldilocks: a lane per cell.  Fr: a cell is two neighbouring lanes, each moving one 16-byte half, so that
//               a wave's stores to dst are one contiguous kilobyte; the halves are exchanged within the pair and both lanes compute
//               the element.  sMap reads and dst writes run along the row-major order; the read of w is the gather.
// Goldilocks: any u64 in w or a coefficient counts as its value mod p; what is written is canonical.  Fr: w holds NORMAL-form values
// (what circom's calculator and a .wtns hold), any 256-bit pattern counting as its value mod r; coefficients are Montgomery words (the
// exec file's section 4), so fr_mul(w, c) is already the normal-form product and the additions convert nothing.  The one conversion
// happens per gathered cell (fr_mul by R^2), which costs a product per cell and saves a pass over w and a second copy of it.
//
// Safety: no index read from a table is used unchecked.  An addition whose a or b is >= nW, or whose dst is outside [nWitness, nW), writes
// nothing.  A gather index >= nW writes zero and lowers the bad cell (scratch slot SCR_WTNS) to its flat index (i nCols + j) by an atomic
// minimum.  The level table is a host array and is checked before the first launch.  Shared with conn_pols.hip: that report, the cell walk
// and the fields as template parameters (smap_cells.cuh); the grid, the overlap test and the sMap's narrowing (smap_plan.h).
#include "common.h"
#include "smap_cells.cuh"
#include "wtns_plan.h"
#include <string.h>
#include <vector>

using namespace pil2gl;

namespace {

using namespace smapcells;
using namespace smapplan;

// ---- additions ----
// coefs: two elements an addition (ca, cb), in the records' order.  w times a coefficient: for Fr normal x Montgomery = the normal-form
// product, canonical
template <class F>
__global__ void __launch_bounds__(THREADS) wtns_adds_kernel(typename F::Mem *w, u32 nWitness, u32 nW, const uint4 *__restrict__ adds,
                                                            const typename F::Mem *__restrict__ coefs, u32 count) {
    for (u64 k = (u64)blockIdx.x * THREADS + threadIdx.x; k < count; k += (u64)gridDim.x * THREADS) {      // 64 bits: a level near 2^32 records must not wrap
        const uint4 r = adds[k];
        if (r.x >= nW || r.y >= nW || r.z < nWitness || r.z >= nW) continue;
        const typename F::Elem x = F::mul(F::load(w, r.x), F::reduce(F::load(coefs, 2 * k)));
        const typename F::Elem y = F::mul(F::load(w, r.y), F::reduce(F::load(coefs, 2 * k + 1)));
        F::store(w, r.z, F::add(x, y));
    }
}

// ---- gather ----
// Two kernels on purpose: the Fr one is another algorithm (two lanes a cell, the halves exchanged within the pair), not the Goldilocks one
// over another element.  Both walk the dstCols-wide output by CellWalk and report through report_bad.
__global__ void __launch_bounds__(THREADS) wtns_gather_gl_kernel(const u64 *__restrict__ w, u32 nW, const u32 *__restrict__ sMap, u64 nRows,
                                                                 u64 nCols, u64 *__restrict__ dst, u64 dstCols, unsigned long long *firstBad) {
    u64 best = NO_BAD;
    for (CellWalk c((u64)blockIdx.x * THREADS + threadIdx.x, (u64)gridDim.x * THREADS, dstCols); c.r < nRows; c.next()) {
        u64 v = 0;
        if (c.j < nCols) {
            const u64 flat = c.r * nCols + c.j;
            const u32 s = sMap[flat];
            if (s >= nW) best = flat < best ? flat : best;
            else if (s) v = gl::canon(w[s]);
        }
        dst[c.r * dstCols + c.j] = v;
    }
    report_bad(best, firstBad);
}

// lanes 2 c and 2 c + 1 of the launch hold cell c: lane parity = the half it loads and stores
__global__ void __launch_bounds__(THREADS) wtns_gather_fr_kernel(const uint4 *__restrict__ w, u32 nW, const u32 *__restrict__ sMap, u64 nRows,
                                                                 u64 nCols, uint4 *__restrict__ dst, u64 dstCols, int toMontgomery,
                                                                 unsigned long long *firstBad) {
    const u32 h = threadIdx.x & 1;
    u64 best = NO_BAD;
    for (CellWalk c(((u64)blockIdx.x * THREADS + threadIdx.x) >> 1, (u64)gridDim.x * (THREADS / 2), dstCols); c.r < nRows; c.next()) {
        uint4 mine = make_uint4(0, 0, 0, 0);
        bool live = false;                           // the same for both lanes of a cell
        if (c.j < nCols) {
            const u64 flat = c.r * nCols + c.j;
            const u32 s = sMap[flat];
            if (s >= nW) best = flat < best ? flat : best;
            else if (s) { mine = w[2 * (size_t)s + h]; live = true; }
        }
        uint4 other;
        other.x = __shfl_xor(mine.x, 1, 64); other.y = __shfl_xor(mine.y, 1, 64);
        other.z = __shfl_xor(mine.z, 1, 64); other.w = __shfl_xor(mine.w, 1, 64);
        uint4 out = mine;
        if (live) {
            u32 x[8];
            bn::unpack(h ? other : mine, h ? mine : other, x);
            if (toMontgomery) {
                u32 r2[8];
                bn::ld_r2(r2);
                bn::fr_mul(x, x, r2);
            } else {
                bn::reduce256(x);
            }
            out = h ? make_uint4(x[4], x[5], x[6], x[7]) : make_uint4(x[0], x[1], x[2], x[3]);
        }
        dst[2 * (c.r * dstCols + c.j) + h] = out;
    }
    report_bad(best, firstBad);
}

// ---- host side ----
// everything the additions refuse, before any device call; words = 1 (Goldilocks) or 4 (Fr) 64-bit words an element
int check_adds(const void *w, u64 nWitness, const void *adds, const void *coefs, u64 nAdds, const uint32_t *levelStart, u32 nLevels, u32 words) {
    if (const char *m = wtnsplan::check_sizes(nWitness, nAdds)) return fail(PIL2GL_EINVAL, "%s", m);
    if (nAdds == 0 && nLevels == 0) return PIL2GL_OK;
    if (!levelStart) return fail(PIL2GL_EINVAL, "null level table");
    if (!wtnsplan::check_level_starts(levelStart, nLevels, nAdds))
        return fail(PIL2GL_EINVAL, "the level table must start at 0, ascend and end at nAdds = %llu", (unsigned long long)nAdds);
    if (nAdds == 0) return PIL2GL_OK;
    if (!w || !adds || !coefs) return fail(PIL2GL_EINVAL, "null buffer");
    if (((uintptr_t)adds | (uintptr_t)coefs) & 15 || (uintptr_t)w & (words == 4 ? 15 : 7))
        return fail(PIL2GL_EINVAL, "adds and coefs must be 16-byte aligned, w %u-byte aligned", words == 4 ? 16u : 8u);
    const u64 wBytes = (nWitness + nAdds) * 8 * words;
    if (meets(w, wBytes, adds, nAdds * 16) || meets(w, wBytes, coefs, nAdds * 16 * words)) return fail(PIL2GL_EINVAL, "w overlaps a table");
    return PIL2GL_OK;
}

int launch_adds(u64 *w, u64 nWitness, const uint32_t *adds, const u64 *coefs, u64 nAdds, const uint32_t *levelStart, u32 nLevels, u32 words,
                hipStream_t st) {
    const u32 nW = (u32)(nWitness + nAdds);
    auto levelsOf = [&](auto field) -> int {           // every level's launch in one field
        typedef decltype(field) F;
        for (u32 l = 0; l < nLevels; l++) {
            const u32 first = levelStart[l], count = levelStart[l + 1] - first;
            if (!count) continue;
            wtns_adds_kernel<F><<<blocks(count), THREADS, 0, st>>>((typename F::Mem *)w, (u32)nWitness, nW, (const uint4 *)adds + first,
                                                                   (const typename F::Mem *)coefs + 2 * (size_t)first, count);
            KERNEL_CHECK();
        }
        return PIL2GL_OK;
    };
    return words == 1 ? levelsOf(GlField{}) : levelsOf(FrField{});
}

// everything the gather refuses, before any device call; *nothing: no cell to write
int check_gather(const void *w, u64 nW, const void *sMap, u64 nRows, u64 nCols, const void *dst, u64 dstCols, u32 words, bool *nothing) {
    *nothing = false;
    if (nW >= wtnsplan::MAX_SIGNALS) return fail(PIL2GL_EINVAL, "nW must stay below 2^32");
    if (dstCols < nCols) return fail(PIL2GL_EINVAL, "dstCols %llu < nCols %llu", (unsigned long long)dstCols, (unsigned long long)nCols);
    if (!nRows || !dstCols) { *nothing = true; return PIL2GL_OK; }
    if (nRows > NO_BAD / 64 / dstCols) return fail(PIL2GL_EINVAL, "size overflows");
    if (!dst || (nCols && !sMap) || (nW && !w)) return fail(PIL2GL_EINVAL, "null buffer");
    const uintptr_t al = words == 4 ? 15 : 7;
    if (((uintptr_t)w | (uintptr_t)dst) & al || (uintptr_t)sMap & 3)
        return fail(PIL2GL_EINVAL, "w and dst must be %u-byte aligned, sMap 4-byte aligned", (unsigned)al + 1);
    const u64 dBytes = nRows * dstCols * 8 * words;
    if (meets(dst, dBytes, w, nW * 8 * words) || meets(dst, dBytes, sMap, nRows * nCols * 4)) return fail(PIL2GL_EINVAL, "dst overlaps w or sMap");
    return PIL2GL_OK;
}

int launch_gather(const u64 *w, u64 nW, const uint32_t *sMap, u64 nRows, u64 nCols, u64 *dst, u64 dstCols, u32 words, int toMontgomery,
                  u64 *hostFirstBad, hipStream_t st) {
    // the bad cell of a checked gather: SCR_WTNS, kept across calls and reset to NO_BAD on this call's stream before every launch
    u64 *cell = nullptr;
    if (hostFirstBad) {
        P2_TRY(scratch(SCR_WTNS, 2, &cell));
        HIP_TRY(hipMemsetAsync(cell, 0xFF, 8, st));
    }
    unsigned long long *bad = (unsigned long long *)cell;
    const u64 cells = nRows * dstCols;
    if (words == 1)
        wtns_gather_gl_kernel<<<blocks(cells), THREADS, 0, st>>>(w, (u32)nW, sMap, nRows, nCols, dst, dstCols, bad);
    else
        wtns_gather_fr_kernel<<<blocks(2 * cells), THREADS, 0, st>>>((const uint4 *)w, (u32)nW, sMap, nRows, nCols, (uint4 *)dst, dstCols, toMontgomery, bad);
    KERNEL_CHECK();
    if (hostFirstBad) {
        HIP_TRY(hipMemcpyAsync(hostFirstBad, bad, 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    return PIL2GL_OK;
}

int gather_dev(const u64 *w, u64 nW, const uint32_t *sMap, u64 nRows, u64 nCols, u64 *dst, u64 dstCols, u32 words, int toMontgomery,
               u64 *hostFirstBad, void *stream) {
    if (hostFirstBad) *hostFirstBad = NO_BAD;
    bool nothing;
    P2_TRY(check_gather(w, nW, sMap, nRows, nCols, dst, dstCols, words, &nothing));
    if (nothing) return PIL2GL_OK;
    P2_TRY(ensure_init());
    return launch_gather(w, nW, sMap, nRows, nCols, dst, dstCols, words, toMontgomery, hostFirstBad, as_stream(stream));
}

int adds_dev(u64 *w, u64 nWitness, const uint32_t *adds, const u64 *coefs, u64 nAdds, const uint32_t *levelStart, u32 nLevels, u32 words, void *stream) {
    P2_TRY(check_adds(w, nWitness, adds, coefs, nAdds, levelStart, nLevels, words));
    if (nAdds == 0) return PIL2GL_OK;
    P2_TRY(ensure_init());
    return launch_adds(w, nWitness, adds, coefs, nAdds, levelStart, nLevels, words, as_stream(stream));
}

// plan, stage, compute, copy out.  idx / coef strides as the files hold the tables: Goldilocks 4 and 4, Fr 2 and 8.
int exec_host(const u64 *hostW, u64 nWitness, const u64 *idx, u64 idxStride, const u64 *coef, u64 coefStride, u64 nAdds, const u64 *sMap64,
              u64 nRows, u64 nCols, u64 *hostDst, u32 words, int toMontgomery) {
    if (const char *m = wtnsplan::check_sizes(nWitness, nAdds)) return fail(PIL2GL_EINVAL, "%s", m);
    const u64 nW = nWitness + nAdds, cells = nCols && nRows > NO_BAD / 64 / nCols ? NO_BAD : nRows * nCols;
    if (cells == NO_BAD) return fail(PIL2GL_EINVAL, "size overflows");
    if ((nWitness && !hostW) || (nAdds && (!idx || !coef)) || (cells && (!sMap64 || !hostDst))) return fail(PIL2GL_EINVAL, "null buffer");
    std::vector<uint32_t> level, levelStart, recs(4 * nAdds);
    std::vector<u64> coefs(2 * words * nAdds);
    u32 nLevels = 0;
    char err[200];
    if (!wtnsplan::levels(idx, idxStride, nAdds, nWitness, level, &nLevels, err, sizeof err)) return fail(PIL2GL_EINVAL, "%s", err);
    levelStart.resize(nLevels + 1);
    wtnsplan::emit(idx, idxStride, nAdds, nWitness, level, nLevels, coef, coefStride, words, recs.data(), coefs.data(), levelStart.data());
    const u64 recWords = pad16(2 * nAdds), mapWords = smapplan::packed_words(cells);
    std::vector<u64> packed(recWords + mapWords);                 // the 32-bit tables travel as whole words
    if (nAdds) memcpy(packed.data(), recs.data(), 16 * nAdds);
    u64 badCell, badValue;
    if (!smapplan::narrow(sMap64, false, 0, nRows, nCols, nW, packed.data() + recWords, &badCell, &badValue))
        return fail(PIL2GL_EINVAL, "sMap[%llu] = %llu names no signal (nWitness + nAdds = %llu)", (unsigned long long)badCell,
                    (unsigned long long)badValue, (unsigned long long)nW);
    const u64 dBytes = cells * 8 * words;
    if (meets(hostDst, dBytes, hostW, nWitness * 8 * words) || meets(hostDst, dBytes, sMap64, cells * 8) ||
        meets(hostDst, dBytes, idx, nAdds ? ((nAdds - 1) * idxStride + 2) * 8 : 0) ||
        meets(hostDst, dBytes, coef, nAdds ? ((nAdds - 1) * coefStride + 2 * words) * 8 : 0))
        return fail(PIL2GL_EINVAL, "dst overlaps w or a table");
    if (!cells) return PIL2GL_OK;
    const u64 wWords = pad16(nW * words), coefWords = pad16(coefs.size());
    Stage s(wWords + recWords + coefWords + mapWords + cells * words);
    P2_TRY(s.rc());
    u64 *dW = s.take(wWords);
    if (dW && nWitness) HIP_TRY(hipMemcpy(dW, hostW, nWitness * 8 * words, hipMemcpyHostToDevice));
    const u64 *dTab = s.put(packed.data(), packed.size());
    const u64 *dCoef = nAdds ? s.put(coefs.data(), coefWords) : nullptr;
    u64 *dDst = s.take(cells * words);
    P2_TRY(s.rc());
    P2_TRY(launch_adds(dW, nWitness, (const uint32_t *)dTab, dCoef, nAdds, levelStart.data(), nLevels, words, 0));
    P2_TRY(launch_gather(dW, nW, (const uint32_t *)(dTab + recWords), nRows, nCols, dDst, nCols, words, toMontgomery, nullptr, 0));
    return s.get(hostDst, dDst, cells * words);
}

}  // namespace

extern "C" {

int pil2gl_wtns_adds_plan(const uint64_t *hostAddIdx, uint64_t idxStride, uint64_t nAdds, uint64_t nWitness, const uint64_t *hostCoef,
                          uint64_t coefStride, uint32_t coefWords, uint32_t *outAdds, uint64_t *outCoef, uint32_t *outLevelStart,
                          uint32_t levelCap, uint32_t *nLevels) {
    if (!nLevels) return fail(PIL2GL_EINVAL, "null nLevels");
    *nLevels = 0;
    if (coefWords != 1 && coefWords != 4) return fail(PIL2GL_EINVAL, "coefWords is 1 (Goldilocks) or 4 (BN254 Fr)");
    if (const char *m = wtnsplan::check_sizes(nWitness, nAdds)) return fail(PIL2GL_EINVAL, "%s", m);
    if (nAdds && (!hostAddIdx || idxStride < 2)) return fail(PIL2GL_EINVAL, "null operand table or idxStride < 2");
    std::vector<uint32_t> level;
    char err[200];
    uint32_t n = 0;
    if (!wtnsplan::levels(hostAddIdx, idxStride, nAdds, nWitness, level, &n, err, sizeof err)) return fail(PIL2GL_EINVAL, "%s", err);
    *nLevels = n;
    if (!outAdds && !outCoef && !outLevelStart) return PIL2GL_OK;
    if (!outLevelStart || (nAdds && !outAdds)) return fail(PIL2GL_EINVAL, "outAdds and outLevelStart go together");
    if (levelCap < n + 1) return fail(PIL2GL_EINVAL, "outLevelStart holds %u entries, %u needed", levelCap, n + 1);
    if (outCoef && nAdds && (!hostCoef || coefStride < 2ull * coefWords)) return fail(PIL2GL_EINVAL, "null coefficient table or coefStride < 2 coefWords");
    wtnsplan::emit(hostAddIdx, idxStride, nAdds, nWitness, level, n, hostCoef, coefStride, coefWords, outAdds, outCoef, outLevelStart);
    return PIL2GL_OK;
}

int pil2gl_debug_wtns_plan(const uint64_t *hostAddIdx, uint64_t idxStride, uint64_t nAdds, uint64_t nWitness, uint32_t *outInfo,
                           uint32_t *outWidths, uint32_t widthCap) {
    if (!outInfo) return fail(PIL2GL_EINVAL, "null argument");
    uint32_t n = 0;
    P2_TRY(pil2gl_wtns_adds_plan(hostAddIdx, idxStride, nAdds, nWitness, nullptr, 0, 1, nullptr, nullptr, nullptr, 0, &n));
    std::vector<uint32_t> level, width(n, 0);
    char err[200];
    wtnsplan::levels(hostAddIdx, idxStride, nAdds, nWitness, level, &n, err, sizeof err);
    for (uint64_t i = 0; i < nAdds; i++) width[level[i]]++;
    uint32_t widest = 0;
    for (uint32_t l = 0; l < n; l++) { if (width[l] > widest) widest = width[l]; if (outWidths && l < widthCap) outWidths[l] = width[l]; }
    outInfo[0] = n; outInfo[1] = n; outInfo[2] = widest; outInfo[3] = THREADS; outInfo[4] = n ? blocks(widest) : 0;
    return PIL2GL_OK;
}

int pil2gl_wtns_adds_dev(uint64_t *w, uint64_t nWitness, const uint32_t *adds, const uint64_t *coefs, uint64_t nAdds,
                         const uint32_t *hostLevelStart, uint32_t nLevels, void *stream) {
    return adds_dev(w, nWitness, adds, coefs, nAdds, hostLevelStart, nLevels, 1, stream);
}
int pil2gl_bn128_wtns_adds_dev(uint64_t *w, uint64_t nWitness, const uint32_t *adds, const uint64_t *coefs, uint64_t nAdds,
                               const uint32_t *hostLevelStart, uint32_t nLevels, void *stream) {
    return adds_dev(w, nWitness, adds, coefs, nAdds, hostLevelStart, nLevels, 4, stream);
}

int pil2gl_wtns_gather_dev(const uint64_t *w, uint64_t nW, const uint32_t *sMap32, uint64_t nRows, uint64_t nCols, uint64_t *dst,
                           uint64_t dstCols, uint64_t *hostFirstBad, void *stream) {
    return gather_dev(w, nW, sMap32, nRows, nCols, dst, dstCols, 1, 0, hostFirstBad, stream);
}
int pil2gl_bn128_wtns_gather_dev(const uint64_t *w, uint64_t nW, const uint32_t *sMap32, uint64_t nRows, uint64_t nCols, uint64_t *dst,
                                 uint64_t dstCols, int toMontgomery, uint64_t *hostFirstBad, void *stream) {
    return gather_dev(w, nW, sMap32, nRows, nCols, dst, dstCols, 4, toMontgomery, hostFirstBad, stream);
}

int pil2gl_wtns_exec(const uint64_t *hostW, uint64_t nWitness, const uint64_t *hostAddIdx, const uint64_t *hostAddCoef, uint64_t nAdds,
                     const uint64_t *hostSMap64, uint64_t nRows, uint64_t nCols, uint64_t *hostDst) {
    return exec_host(hostW, nWitness, hostAddIdx, 4, hostAddCoef, 4, nAdds, hostSMap64, nRows, nCols, hostDst, 1, 0);
}
int pil2gl_bn128_wtns_exec(const uint64_t *hostW, uint64_t nWitness, const uint64_t *hostAddIdx, const uint64_t *hostAddCoef, uint64_t nAdds,
                           const uint64_t *hostSMap64, uint64_t nRows, uint64_t nCols, uint64_t *hostDst, int toMontgomery) {
    return exec_host(hostW, nWitness, hostAddIdx, 2, hostAddCoef, 8, nAdds, hostSMap64, nRows, nCols, hostDst, 4, toMontgomery);
}

}  // extern "C"
