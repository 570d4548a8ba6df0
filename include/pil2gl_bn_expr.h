/*
 * pil2gl_bn_expr.h -- context of the BN254 Fr expression evaluator (pil2-stark-js_amd/csrc/bn_expr.hip).
 *
 * The fflonk final prover evaluates its op-lists row by row over Fr (src/prover/prover.js:212-219,
 * src/prover/prover_helpers.js:31-72 calculateExps, :83-107 compileCode, :109-259 setRef / getRef / evalMap,
 * src/prover/fflonk_prover_worker.js:5-41) with ctx.F = curve.Fr on 32-byte elements.  The op-list itself has the
 * encoding of pil2gl_expr.h (glx_program / glx_op / glx_ref and the three operand classes); what differs is what
 * an element is and how it is counted:
 *
 *   element      4 little-endian u64 words (32 bytes) of a * 2^256 mod r, MONTGOMERY form and canonical (< r): the
 *                bytes ffjavascript keeps in its BigBuffers and pil2gl_bn128_ifft leaves.  No conversion anywhere.
 *   glx_ref.dim  must be 1 (this prover has no extension field)
 *   GLX_TMP      index = tmp id
 *   GLX_SEC      const{id,prime}, cm{id,prime} as source or destination, x, Zi{boundaryId}, the destination q with
 *                dim == 1 (prover_helpers.js:121-122): index counts COLUMNS of a section whose width counts ELEMENTS
 *   GLX_SCALAR   number{value} (the host encodes F.e(value); a negative value is value + r), public, challenge,
 *                subproofValue: index counts ELEMENTS of bnx_ctx.scalars
 *
 * Row addressing is evalMap's (prover_helpers.js:220-233): (i + prime * 2^primeShift) mod 2^nBits.
 */
#pragma once
#include <stdint.h>
#include "pil2gl_expr.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
    uint64_t *ptr;      /* row-major rows x width elements of 4 u64 words, 16-byte aligned */
    uint64_t  width;    /* elements per row */
} bnx_section;

typedef struct {
    uint32_t nBits;         /* log2(rows) of the evaluated domain, at most 28 */
    uint32_t primeShift;    /* 0 ("n") or nBitsExt-nBits ("ext") */
    uint32_t nSections;     /* at most PIL2GL_BNX_MAX_SECTIONS */
    uint32_t nScalars;      /* 32-byte elements in scalars[] */
    const bnx_section *sections;
    const uint64_t    *scalars;     /* host pointer: 4 * nScalars words */
} bnx_ctx;

#define PIL2GL_BNX_MAX_SECTIONS 24

#ifdef __cplusplus
}
#endif
