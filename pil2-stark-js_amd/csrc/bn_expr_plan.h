// Host-only half of the BN254 Fr expression evaluator (bn_expr.hip): what is refused before any device call, and the one place that
// decides the kernel form and the launch geometry.  No HIP header: the tests compile it on its own (tests/bn_expr_dump.cpp).
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <set>
#include <map>
#include <utility>
#include "../../include/pil2gl_bn_expr.h"

namespace bnx {

constexpr uint32_t MAX_BITS = 28;
constexpr uint32_t LDS_BYTES = 60 * 1024;            // temporaries of one workgroup, as expr.hip budgets them
constexpr uint32_t MIN_THREADS = 64, MAX_THREADS = 256;
constexpr uint32_t LDS_SLOT_LIMIT = LDS_BYTES / (32 * MIN_THREADS);      // 30: the most live temporaries a one-wave workgroup holds in LDS
// Persistent workgroups: the LDS form's 56-60 KiB leave room for two workgroups in a CU's 160 KiB, and the chip has 256 CUs.  The global
// form keeps the same grid, so its working buffer is slots * 32 B * 2^17 lanes whatever the domain.
constexpr uint32_t MAX_BLOCKS = 512;
constexpr uint32_t MAX_SLOTS = 4096;                 // live temporaries a program may need: a 16 GiB working buffer at the full grid; more is refused

struct Geometry {
    uint32_t form;                                   // 0: temporaries in LDS, 1: in the global working buffer
    uint32_t threads, blocks;                        // blocks: of this domain (rows / threads, at most MAX_BLOCKS)
    uint32_t ldsBytes;
    uint64_t lanesPerLaunch;                         // threads * MAX_BLOCKS: a domain above it takes the grid-stride loop's second turn
    uint64_t tmpBytes;                               // global form: slots * 32 * threads * blocks
};

// [slot][half][lane]: a slot is 32 bytes per lane.  LDS when the slots fit at some workgroup size from 256 down to one wave.
inline Geometry geometry(uint32_t nSlots, uint32_t nBits) {
    Geometry g;
    const uint32_t slots = nSlots ? nSlots : 1;
    const uint64_t rows = 1ull << nBits;
    g.form = slots <= LDS_SLOT_LIMIT ? 0 : 1;
    g.threads = MAX_THREADS;
    if (g.form == 0) while ((uint64_t)slots * 32 * g.threads > LDS_BYTES) g.threads /= 2;
    const uint64_t want = (rows + g.threads - 1) / g.threads;
    g.blocks = (uint32_t)(want < MAX_BLOCKS ? want : MAX_BLOCKS);
    g.ldsBytes = g.form == 0 ? slots * 32 * g.threads : 0;
    g.lanesPerLaunch = (uint64_t)g.threads * MAX_BLOCKS;
    g.tmpBytes = g.form == 1 ? (uint64_t)slots * 32 * g.threads * g.blocks : 0;
    return g;
}

// Everything that is refused before any device call.  Returns true when the program may run; else a message in err.
inline bool validate(const glx_program *prog, const bnx_ctx *ctx, char *err, size_t errLen) {
#define BNX_FAIL(...) do { snprintf(err, errLen, __VA_ARGS__); return false; } while (0)
    if (!prog || !ctx) BNX_FAIL("null program or context");
    if (prog->nOps && !prog->ops) BNX_FAIL("null op-list");
    if (ctx->nBits > MAX_BITS) BNX_FAIL("nBits = %u: at most %u", ctx->nBits, MAX_BITS);
    if (ctx->primeShift > MAX_BITS) BNX_FAIL("primeShift = %u: at most %u", ctx->primeShift, MAX_BITS);
    if (ctx->nSections > PIL2GL_BNX_MAX_SECTIONS) BNX_FAIL("too many sections (%u > %d)", ctx->nSections, PIL2GL_BNX_MAX_SECTIONS);
    if (ctx->nSections && !ctx->sections) BNX_FAIL("null section table");
    for (uint32_t i = 0; i < ctx->nSections; i++) if (ctx->sections[i].width >> 32) BNX_FAIL("section %u too wide", i);
    // (section, column) -> the row offsets it is read / written at
    std::map<std::pair<uint32_t, uint32_t>, std::set<int32_t>> reads, writes;
    for (uint32_t k = 0; k < prog->nOps; k++) {
        const glx_op &o = prog->ops[k];
        if (o.op > GLX_OP_COPY) BNX_FAIL("Invalid op: %u", o.op);                        // prover_helpers.js:97
        const int ns = o.op == GLX_OP_COPY ? 1 : 2;
        for (int s = 0; s < ns + 1; s++) {
            const glx_ref &r = s < ns ? o.src[s] : o.dest;
            if (r.dim != 1) BNX_FAIL("dim %u in op %u: Fr elements have dim 1", r.dim, k);
            if (r.kind == GLX_TMP) {
                if (r.index >= prog->nTmp) BNX_FAIL("tmp %u out of range in op %u", r.index, k);
            } else if (r.kind == GLX_SEC) {
                if (r.section >= ctx->nSections) BNX_FAIL("section %u out of range in op %u", r.section, k);
                const bnx_section &sec = ctx->sections[r.section];
                if (r.index >= sec.width) BNX_FAIL("column %u out of range in op %u", r.index, k);
                if (!sec.ptr) BNX_FAIL("section %u is read or written in op %u and has a null pointer", r.section, k);
                const int64_t off = (int64_t)r.prime * ((int64_t)1 << ctx->primeShift);
                if (off != (int64_t)(int32_t)off) BNX_FAIL("row offset overflow in op %u", k);
                (s < ns ? reads : writes)[std::make_pair((uint32_t)r.section, r.index)].insert(r.prime);
            } else if (r.kind == GLX_SCALAR) {
                if (s == ns) BNX_FAIL("Invalid reference type set");                      // prover_helpers.js:148
                if (r.index >= ctx->nScalars) BNX_FAIL("scalar %u out of range in op %u", r.index, k);
                if (!ctx->scalars) BNX_FAIL("null scalar pool");
            } else BNX_FAIL("Invalid reference type get");                               // prover_helpers.js:216
        }
    }
    // The reference's row loop is serial; here every row is a lane of its own.  A column that is written may be read by the lane that
    // writes it, at the cell it writes (x = x * x), and by nobody else: any non-zero row offset on a column that is both read and
    // written, or two different offsets among its writes, would be order-dependent there and a race here.
    for (const auto &w : writes) {
        if (w.second.size() > 1) BNX_FAIL("section %u column %u is written at more than one row offset", w.first.first, w.first.second);
        const auto rd = reads.find(w.first);
        if (rd == reads.end()) continue;
        bool shifted = *w.second.begin() != 0;
        for (int32_t p : rd->second) shifted |= p != 0;
        if (shifted) BNX_FAIL("section %u column %u is written and also read at a non-zero row offset", w.first.first, w.first.second);
    }
    return true;
#undef BNX_FAIL
}

}  // namespace bnx
