// G1.toAffine(G1.multiExpAffine(bases, scalars)) of ffjavascript's BN254 curve, computed by libpil2gl on the MI355X: the commitment of one
// polynomial (fflonk's commit(..., { multiExp: true })).
//   bases    n affine points of 64 bytes (x then y, Fq Montgomery bytes; infinity all zero), as zkey.pTau / ptau section 2 holds them
//   scalars  32 bytes per element; element i at byte 32 * i * stride (stride = nPols commits one column of a row-major matrix in place)
//   options  { stride = 1, montgomery = true, n = what bases holds }: montgomery false = normal form, what multiExpAffine takes after
//            Fr.batchFromMontgomery
// A buffer is a DevBuffer (resident, nothing staged), a Uint8Array, or anything with ffjavascript BigBuffer's surface
// { byteLength, slice(a, b) -> Uint8Array }, staged in 256 MB pieces.  Returns a Promise of the 64-byte affine point as a Uint8Array.
"use strict";
const { addon, isDev } = require("./native.js");

const CHUNK_BYTES = 1 << 28;

function asWords(u8) {       // a BigUint64Array over the same bytes where alignment allows, over a copy otherwise
    if (u8.byteOffset % 8 === 0) return new BigUint64Array(u8.buffer, u8.byteOffset, u8.byteLength / 8);
    const c = new Uint8Array(u8.byteLength); c.set(u8);
    return new BigUint64Array(c.buffer);
}
function byteLength(buf) { return isDev(buf) ? buf.length * 8 : buf.byteLength; }

async function multiExpAffine(bases, scalars, options = {}) {
    const stride = options.stride === undefined ? 1 : options.stride;
    const montgomery = options.montgomery === undefined ? true : !!options.montgomery;
    const n = options.n === undefined ? Math.floor(byteLength(bases) / 64) : options.n;
    if (!Number.isInteger(stride) || stride < 1) throw new Error("g1_msm: stride must be a positive integer");
    if (!Number.isInteger(n) || n < 0) throw new Error("g1_msm: bad point count");
    const scalarBytes = n ? ((n - 1) * stride + 1) * 32 : 0;
    if (byteLength(bases) < n * 64) throw new Error("g1_msm: bases hold " + byteLength(bases) + " bytes, need " + n * 64);
    if (byteLength(scalars) < scalarBytes) throw new Error("g1_msm: scalars hold " + byteLength(scalars) + " bytes, need " + scalarBytes);
    const owned = [];
    const resident = (buf, bytes) => {
        if (isDev(buf)) return buf.ptr;
        const p = addon.devAlloc(Math.max(1, bytes / 8)); owned.push(p);
        for (let o = 0; o < bytes; o += CHUNK_BYTES) {
            const e = Math.min(bytes, o + CHUNK_BYTES);
            addon.devUpload(p, o / 8, asWords(buf instanceof Uint8Array ? buf.subarray(o, e) : buf.slice(o, e)));
        }
        return p;
    };
    try {
        const dBases = resident(bases, n * 64), dScalars = resident(scalars, scalarBytes);
        const dOut = addon.devAlloc(8); owned.push(dOut);
        addon.bn128G1MsmDev(dBases, dScalars, n, stride, montgomery ? 1 : 0, dOut);
        const out = new BigUint64Array(8);
        addon.devDownload(out, dOut, 0);                 // a synchronous copy: ordered after the kernels
        return new Uint8Array(out.buffer);
    } finally {
        for (const p of owned) addon.devFree(p);
    }
}

module.exports.multiExpAffine = multiExpAffine;
