// Host-only half of the recursion witness expansion (wtns_exec.hip): what the entries refuse about the additions of an `exec` file, and
// the order in which the device runs them.  No HIP header: it builds with the plain C++ compiler (tests/wtns_plan_dump.cpp runs it under
// the sanitizers).  The launch grid, the signal limit and the sMap's narrowing are smap_plan.h's, shared with conn_plan.h.
//
// The reference runs the additions serially, w.push(w[a] ca + w[b] cb) (src/compressor/compressor_exec.js:17-19,
// src/final/main_final_exec.js:55-57); a_i, b_i may name an earlier addition.  On the device every addition whose operands are ready
// runs at once:
//   level(i) = 0                                              when both operands are witness signals (below nWitness)
//            = 1 + the highest level among its operands that are additions   otherwise
// The additions are emitted sorted by level, stable within a level (source order), each as four 32-bit words (a, b, dst, source position)
// with dst = nWitness + source position, the coefficients permuted alike, and levelStart[0 .. nLevels]: level l is the records
// [levelStart[l], levelStart[l + 1]).  Every level's operands were written by lower levels, so the result equals the serial loop's for
// every table, whatever its depth.
//
// ONE LAUNCH PER LEVEL: a chain of depth D costs D launches.  r1cs2plonk.js:49-67 reduces a linear combination of n terms through a queue
// (two terms off the front, their sum to the back), which gives depth ceil(log2 n), so a circuit's tables have a few tens of levels at
// most.  Narrow tail levels are not fused into one workgroup.
//
// Refused: nWitness + nAdds >= 2^32 (the reference's sMap is Uint32Array, compressor18_setup.js:62, and the device records are 32-bit);
// an operand >= nWitness + i in addition i (a forward or self reference: the reference would read `undefined`).
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <vector>
#include "smap_plan.h"

namespace wtnsplan {

using smapplan::MAX_SIGNALS;
using smapplan::blocks;                              // the additions' grid, under the name this planner's callers know

// 0, or a message for PIL2GL_EINVAL
inline const char *check_sizes(uint64_t nWitness, uint64_t nAdds) {
    if (nWitness >= MAX_SIGNALS || nAdds >= MAX_SIGNALS || nWitness + nAdds >= MAX_SIGNALS) return "nWitness + nAdds must stay below 2^32";
    return nullptr;
}

// Addition i reads idx[idxStride * i] and idx[idxStride * i + 1].  level[i] for every addition, the number of levels as the result
// (0 for no additions); false with a message naming the addition when an operand is not yet defined.
inline bool levels(const uint64_t *idx, uint64_t idxStride, uint64_t nAdds, uint64_t nWitness, std::vector<uint32_t> &level, uint32_t *nLevels,
                   char *err, size_t errLen) {
    level.assign(nAdds, 0);
    uint32_t top = 0;
    for (uint64_t i = 0; i < nAdds; i++) {
        uint32_t lv = 0;
        for (int k = 0; k < 2; k++) {
            const uint64_t s = idx[idxStride * i + k];
            if (s >= nWitness + i) {
                snprintf(err, errLen, "addition %llu: operand %c = %llu is not defined before it (signals below %llu are)", (unsigned long long)i,
                         k ? 'b' : 'a', (unsigned long long)s, (unsigned long long)(nWitness + i));
                return false;
            }
            if (s >= nWitness && level[s - nWitness] + 1 > lv) lv = level[s - nWitness] + 1;
        }
        level[i] = lv;
        if (lv + 1 > top) top = lv + 1;
    }
    *nLevels = top;
    return true;
}

// The stable sort by level: levelStart[0 .. nLevels], outAdds[4 k ..] = (a, b, dst, source position) of the k-th record, and
// outCoef[2 coefWords k ..] = the two coefficients of that addition (coefWords words each, read at coef[coefStride * i] and the
// coefWords words after).  coef and outCoef may both be null (the order alone).
inline void emit(const uint64_t *idx, uint64_t idxStride, uint64_t nAdds, uint64_t nWitness, const std::vector<uint32_t> &level, uint32_t nLevels,
                 const uint64_t *coef, uint64_t coefStride, uint32_t coefWords, uint32_t *outAdds, uint64_t *outCoef, uint32_t *levelStart) {
    std::vector<uint32_t> at(nLevels + 1, 0);
    for (uint64_t i = 0; i < nAdds; i++) at[level[i] + 1]++;
    for (uint32_t l = 0; l < nLevels; l++) at[l + 1] += at[l];
    for (uint32_t l = 0; l <= nLevels; l++) levelStart[l] = at[l];
    for (uint64_t i = 0; i < nAdds; i++) {
        const uint64_t k = at[level[i]]++;
        outAdds[4 * k + 0] = (uint32_t)idx[idxStride * i];
        outAdds[4 * k + 1] = (uint32_t)idx[idxStride * i + 1];
        outAdds[4 * k + 2] = (uint32_t)(nWitness + i);
        outAdds[4 * k + 3] = (uint32_t)i;
        if (coef && outCoef)
            for (uint32_t c = 0; c < 2 * coefWords; c++) outCoef[2 * coefWords * k + c] = coef[coefStride * i + c];
    }
}

// what the device entries check about a level table before the first launch: it starts at 0, ascends, ends at nAdds
inline bool check_level_starts(const uint32_t *levelStart, uint32_t nLevels, uint64_t nAdds) {
    if (levelStart[0] != 0 || levelStart[nLevels] != nAdds) return false;
    for (uint32_t l = 0; l < nLevels; l++) if (levelStart[l] > levelStart[l + 1]) return false;
    return true;
}

}  // namespace wtnsplan
