// The wave merge in front of an atomic add of 1, gfx950: what lookup_mult.hip and range_mult.hip do when many lanes of a wave add to the
// same 32-bit counter.  Up to MERGE_ROUNDS times the wave takes its first lane with an add still to make, reads that lane's counter number
// (v_readlane), ballots the lanes on the same counter and lets the first lane add their number in ONE atomic; lanes left after the rounds
// add 1 each.  One value: one atomic a wave instead of 64 on one address.  All distinct: four rounds of a readlane, a compare and a ballot
// retire four lanes, the other sixty add as before.  No LDS of its own; the counters may lie in global memory or in LDS.
#pragma once
#include "common.h"

namespace wavemerge {

using pil2gl::u32;
using pil2gl::u64;

constexpr int MERGE_ROUNDS = 4;

// one add to counter s for every lane with `add` set, lanes on one counter merged; every lane of the wave arrives here.  Counter s is the
// word words[SPACING s + OFFSET]: lookup_mult.hip keeps it beside a slot's row (2, 1), range_mult.hip's counters are dense (1, 0)
template <int SPACING, int OFFSET>
__device__ __forceinline__ void add_merged(u32 *words, u32 s, bool add) {
    u64 todo = __ballot(add);
    const u32 lane = threadIdx.x & 63;
    for (int round = 0; round < MERGE_ROUNDS && todo; round++) {
        const u32 first = (u32)__ffsll((unsigned long long)todo) - 1;
        const u32 slot = (u32)__builtin_amdgcn_readlane((int)s, (int)first);
        const bool mine = add && s == slot;
        const u64 group = __ballot(mine);
        if (lane == first) atomicAdd(&words[SPACING * (u64)slot + OFFSET], (u32)__popcll((unsigned long long)group));
        add = add && !mine;
        todo &= ~group;
    }
    if (add) atomicAdd(&words[SPACING * (u64)s + OFFSET], 1u);
}

// the same merge in front of a 64-bit counter (mult_session.hip: a session's counts pass 2^32).  Counter s is the 64-bit word
// words[SPACING s + OFFSET]; the rounds are the 32-bit form's, the atomic a global_atomic_add_x2 with a zero high half
template <int SPACING, int OFFSET>
__device__ __forceinline__ void add_merged64(unsigned long long *words, u32 s, bool add) {
    u64 todo = __ballot(add);
    const u32 lane = threadIdx.x & 63;
    for (int round = 0; round < MERGE_ROUNDS && todo; round++) {
        const u32 first = (u32)__ffsll((unsigned long long)todo) - 1;
        const u32 slot = (u32)__builtin_amdgcn_readlane((int)s, (int)first);
        const bool mine = add && s == slot;
        const u64 group = __ballot(mine);
        if (lane == first) atomicAdd(&words[SPACING * (u64)slot + OFFSET], (unsigned long long)__popcll((unsigned long long)group));
        add = add && !mine;
        todo &= ~group;
    }
    if (add) atomicAdd(&words[SPACING * (u64)s + OFFSET], 1ull);
}

}  // namespace wavemerge
