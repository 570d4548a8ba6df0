// G1.toAffine(G1.multiExpAffine(bases, scalars)) of ffjavascript's BN254 curve, computed by libpil2gl on the MI355X: the commitment of one
// polynomial (fflonk's commit(..., { multiExp: true })).
//   bases    n affine points of 64 bytes (x then y, Fq Montgomery bytes; infinity all zero), as zkey.pTau / ptau section 2 holds them
//   scalars  32 bytes per element; element i at byte 32 * i * stride (stride = nPols commits one column of a row-major matrix in place)
//   options  { stride = 1, montgomery = true, n = what bases holds }: montgomery false = normal form, what multiExpAffine takes after
//            Fr.batchFromMontgomery
// multiExpPacked(bases, coefs, polys, { stride, montgomery }) is a stage's commit in one call: the points of K packed polynomials
// (fflonk's CPolynomial, f(X) = sum_j X^j p_j(X^m)) read as columns of the row-major coefficient matrix `coefs` of `stride` elements per
// row, no packed copy built.  polys[k] = { first = 0, rows, slots: [col | null, ...] }: coefficient i of polynomial k is element
// first + floor(i / m) * stride + slots[i mod m], 0 where the slot is null; it has m * rows coefficients, m = slots.length.  Returns a
// Promise of K 64-byte Uint8Arrays, downloaded together.
// A buffer is a DevBuffer (resident, nothing staged), a Uint8Array, or anything with ffjavascript BigBuffer's surface
// { byteLength, slice(a, b) -> Uint8Array }, staged in 256 MB pieces.  Returns a Promise of the 64-byte affine point as a Uint8Array.
"use strict";
const { addon, isDev } = require("./native.js");
const { byteLength, scope, input, output } = require("./bn128_stage.js").native();

async function multiExpAffine(bases, scalars, options = {}) {
    const stride = options.stride === undefined ? 1 : options.stride;
    const montgomery = options.montgomery === undefined ? true : !!options.montgomery;
    const n = options.n === undefined ? Math.floor(byteLength(bases) / 64) : options.n;
    if (!Number.isInteger(stride) || stride < 1) throw new Error("g1_msm: stride must be a positive integer");
    if (!Number.isInteger(n) || n < 0) throw new Error("g1_msm: bad point count");
    const scalarBytes = n ? ((n - 1) * stride + 1) * 32 : 0;
    if (byteLength(bases) < n * 64) throw new Error("g1_msm: bases hold " + byteLength(bases) + " bytes, need " + n * 64);
    if (byteLength(scalars) < scalarBytes) throw new Error("g1_msm: scalars hold " + byteLength(scalars) + " bytes, need " + scalarBytes);
    const out = new Uint8Array(64);
    scope([input(bases, n * 64), input(scalars, scalarBytes), output(out, 64)],
        ([dBases, dScalars, dOut]) => addon.bn128G1MsmDev(dBases, dScalars, n, stride, montgomery ? 1 : 0, dOut));
    return out;
}

const EMPTY_SLOT = 0xFFFFFFFF;

async function multiExpPacked(bases, coefs, polys, options = {}) {
    const stride = options.stride === undefined ? 1 : options.stride;
    const montgomery = options.montgomery === undefined ? true : !!options.montgomery;
    if (!Number.isInteger(stride) || stride < 1) throw new Error("g1_msm: stride must be a positive integer");
    if (!Array.isArray(polys) || polys.length < 1) throw new Error("g1_msm: polys must be a non-empty array");
    const K = polys.length, desc = new BigUint64Array(3 * K), slots = [];
    let nMax = 0, extent = 0;                            // points and coefficient elements the descriptors reach
    polys.forEach((p, k) => {
        const first = p.first === undefined ? 0 : p.first;
        if (!Number.isInteger(first) || first < 0 || !Number.isInteger(p.rows) || p.rows < 0 || !Array.isArray(p.slots))
            throw new Error("g1_msm: polynomial " + k + " needs { first, rows, slots }");
        let top = -1;
        for (const c of p.slots) {
            if (c !== null && (!Number.isInteger(c) || c < 0 || c >= stride)) throw new Error("g1_msm: polynomial " + k + ": column " + c + " outside a row of " + stride);
            slots.push(BigInt(c === null ? EMPTY_SLOT : c));
            if (c !== null) top = Math.max(top, c);
        }
        desc[3 * k] = BigInt(first); desc[3 * k + 1] = BigInt(p.rows); desc[3 * k + 2] = BigInt(p.slots.length);
        nMax = Math.max(nMax, p.rows * p.slots.length);
        if (p.rows && top >= 0) extent = Math.max(extent, first + (p.rows - 1) * stride + top + 1);
    });
    if (byteLength(bases) < nMax * 64) throw new Error("g1_msm: bases hold " + byteLength(bases) + " bytes, need " + nMax * 64);
    if (byteLength(coefs) < extent * 32) throw new Error("g1_msm: coefs hold " + byteLength(coefs) + " bytes, need " + extent * 32);
    const out = new Uint8Array(64 * K);                  // all K points come back in one copy
    scope([input(bases, nMax * 64), input(coefs, extent * 32), output(out, 64 * K)], ([dBases, dCoefs, dOut]) =>
        addon.bn128G1CommitDev(dBases, isDev(bases) ? Math.floor(byteLength(bases) / 64) : nMax, dCoefs, stride, montgomery ? 1 : 0, desc, BigUint64Array.from(slots), dOut));
    return polys.map((_, k) => out.subarray(64 * k, 64 * k + 64));
}

module.exports.multiExpAffine = multiExpAffine;
module.exports.multiExpPacked = multiExpPacked;
