// Host half of the index table that conn_check.hip, tuple_check.hip and lookup_mult.hip build on the device: its capacity, and the hash as
// ONE function for host and device, so that a test can ask where a key lands (pil2gl_debug_tuple_home).  No HIP header: it builds with the
// plain C++ compiler (tests/*_plan_dump.cpp run it under the sanitizers).  The device half, and what the table is, is index_table.cuh.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define INDEX_TABLE_HD __host__ __device__
#else
#define INDEX_TABLE_HD
#endif

namespace indextable {

constexpr uint64_t MIN_CAPACITY = 16;
constexpr uint64_t NONE = ~0ull;                     // no slot; the units' reports say "no row" with the same word

// the smallest power of two >= twice the items that can be inserted and >= MIN_CAPACITY: the load factor never exceeds 1 / 2
struct Capacity { uint64_t slots; uint32_t bits; };
inline Capacity capacity_for(uint64_t items) {
    Capacity c{ MIN_CAPACITY, 0 };
    while (c.slots < 2 * items) c.slots <<= 1;
    while ((1ull << c.bits) < c.slots) c.bits++;
    return c;
}

// ---- the hash of a key: bn_h1h2.hip's mixing over the canonical elements' 32-bit limbs, low limb first, element after element (xor a
// limb, multiply, shift; murmur3's finaliser; 32-bit multiplies only).  Two lanes of it give 64 bits: conn_check.hip's table may have more
// than 2^32 slots.
struct TupleHash {
    uint32_t h = 0x9E3779B9u, g = 0x7F4A7C15u;
    INDEX_TABLE_HD inline void absorb(uint32_t w) {
        h = (h ^ w) * 0x85EBCA6Bu; h ^= h >> 15;
        g = (g ^ w) * 0xC2B2AE35u; g ^= g >> 13;
    }
    INDEX_TABLE_HD inline uint64_t finish() const {
        uint32_t a = h * 0xC2B2AE35u, b = g * 0x85EBCA6Bu;
        a ^= a >> 16; b ^= b >> 16;
        return ((uint64_t)b << 32) | a;
    }
};

// the home slot of a tuple given as k elemWords canonical 64-bit words; capacity a power of two
inline uint64_t home(const uint64_t *words, uint64_t k, uint32_t elemWords, uint64_t capacity) {
    TupleHash x;
    for (uint64_t i = 0; i < k * elemWords; i++) { x.absorb((uint32_t)words[i]); x.absorb((uint32_t)(words[i] >> 32)); }
    return x.finish() & (capacity - 1);
}

}  // namespace indextable
