// Device half of the index table of conn_check.hip, tuple_check.hip and lookup_mult.hip, gfx950.  The host half is index_table_plan.h.
//   the table  open addressing, linear probing, capacity a power of two >= twice the items that can be inserted.  A slot holds a 32-bit
//            INDEX (a cell, a row; EMPTY = 2^32 - 1), never the key: the unit re-derives the key from the index (`holds`, below), so no
//            claimed slot has a half-written key and a slot costs the same over Fr as over Goldilocks.  Slots lie SPACING 32-bit words apart:
//            1, or 2 where a unit keeps a word of its own beside each slot.
//   insert   atomicCAS claims an EMPTY slot; a slot whose index has the SAME key is lowered to the smaller index by atomicMin.  A slot never
//            moves and its content only falls, so after all inserts a slot holds the smallest index of its key, whatever the order of
//            arrival, and every index of one key went to one slot.
//   find     after the inserts: an empty slot ends the run.
// What a lane met: insert gives back the content it found in its slot -- the value it read or, when it lowered the slot, what atomicMin
// returned.  A read may be stale, but a stale value is only LARGER than the slot's present content, so c > met holds for the present
// content too and c need not issue an atomicMin it cannot win.  For an index c, max(met, c) is thus an index of the key that is not its
// smallest, and over all lanes of a key the smallest such maximum is the key's second smallest index: when the two smallest meet in the
// slot, in either order, one of them reports the larger.  conn_check.hip's IDS_NOT_DISTINCT report rests on this; the others need the slot.
// Safety: a slot's content is used as an index only below `limit`; every probe loop runs at most `capacity` times whatever the data.
// Plain vector loads and global atomics only.
#pragma once
#include "smap_cells.cuh"
#include "index_table_plan.h"

namespace indextable {

using namespace smapcells;
constexpr u32 EMPTY = 0xFFFFFFFFu;

// ---- what the two fields do not share: zero and equality of canonical elements, their limbs for the hash ----
__device__ __forceinline__ bool is_zero(u64 a) { return a == 0; }
__device__ __forceinline__ bool is_zero(const FrField::Elem &a) { return bn::is_zero(a.v); }
__device__ __forceinline__ bool same(u64 a, u64 b) { return a == b; }
__device__ __forceinline__ bool same(const FrField::Elem &a, const FrField::Elem &b) {
    return ((a.v[0] ^ b.v[0]) | (a.v[1] ^ b.v[1]) | (a.v[2] ^ b.v[2]) | (a.v[3] ^ b.v[3]) |
            (a.v[4] ^ b.v[4]) | (a.v[5] ^ b.v[5]) | (a.v[6] ^ b.v[6]) | (a.v[7] ^ b.v[7])) == 0;
}
// one more element of a key that is a tuple; hash_of: a key of one element
__device__ __forceinline__ void absorb(TupleHash &x, u64 e) { x.absorb((u32)e); x.absorb((u32)(e >> 32)); }
__device__ __forceinline__ void absorb(TupleHash &x, const FrField::Elem &e) {
#pragma unroll
    for (int i = 0; i < 8; i++) x.absorb(e.v[i]);
}
template <class E> __device__ __forceinline__ u64 hash_of(const E &e) { TupleHash x; absorb(x, e); return x.finish(); }

// a lane's slot (NONE: none), what it met there (EMPTY: nothing, it claimed the slot), the slot's distance from the key's home, at most 2^32 - 1
struct Hit { u64 slot; u32 met, displaced; };

// Puts index idx < limit into the table, slot `home` & mask first.  holds(cur): does index cur < limit have idx's key.
template <int SPACING, class Holds>
__device__ __forceinline__ Hit insert(u32 *slots, u64 mask, u64 home, u32 idx, u32 limit, Holds holds) {
    u64 s = home & mask;
    for (u64 probe = 0; probe <= mask; probe++, s = (s + 1) & mask) {
        const u32 displaced = probe > EMPTY ? EMPTY : (u32)probe;
        u32 cur = slots[SPACING * s];
        if (cur == EMPTY) {
            cur = atomicCAS(&slots[SPACING * s], EMPTY, idx);
            if (cur == EMPTY) return Hit{ s, EMPTY, displaced };             // claimed
        }
        if (cur < limit && holds(cur)) {                                     // the same key: the slot keeps the smaller index
            if (idx < cur) cur = atomicMin(&slots[SPACING * s], idx);
            return Hit{ s, cur, displaced };
        }
    }
    return Hit{ NONE, EMPTY, 0 };
}

// the slot whose index has the key, and that index in `met`; slot NONE when no slot has it.  After the inserts.
template <int SPACING, class Holds>
__device__ __forceinline__ Hit find(const u32 *slots, u64 mask, u64 home, u32 limit, Holds holds) {
    u64 s = home & mask;
    for (u64 probe = 0; probe <= mask; probe++, s = (s + 1) & mask) {
        const u32 cur = slots[SPACING * s];
        if (cur >= limit) return Hit{ NONE, EMPTY, 0 };                      // an empty slot ends the run
        if (holds(cur)) return Hit{ s, cur, 0 };
    }
    return Hit{ NONE, EMPTY, 0 };
}

// the longest displacement of a launch's inserts into one header word: a wave maximum, then one atomic a wave that saw one.  A lane that
// joined a slot counts like the lane that claimed it: one key, one home, one slot.  Every lane of the wave arrives here.
__device__ __forceinline__ void report_probe(u32 longest, unsigned long long *word) {
    for (int o = 32; o > 0; o >>= 1) { const u32 other = __shfl_xor(longest, o, 64); longest = other > longest ? other : longest; }
    if ((threadIdx.x & 63) == 0 && longest) atomicMax(word, (unsigned long long)longest);
}

}  // namespace indextable
