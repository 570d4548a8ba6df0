// The long-vector operations of shplonkjs / ffjavascript's Polynomial over BN254 Fr that the fflonk prover's last two steps use
// (fflonk_prover_helpers.js:147-148 Q.divZh; :212 open: divByXNSubValue-style divisions and evaluate), computed by libpil2gl on the
// MI355X (csrc/bn_poly.hip).  A polynomial is its coefficient buffer: 32 bytes per element (Fr Montgomery bytes, what curve.Fr keeps
// and what fft_p_bn128's ifft leaves), element i at byte 32 * i * stride -- stride = nPols works on one column of a row-major matrix in
// place.  One recurrence serves all three, d[i] = c[i] + beta d[i + k]: d[k..n) is the quotient by x^k - beta (coefficient m at m + k),
// d[0..k) the remainder.
//   buf      a DevBuffer (resident: worked on where it is, nothing staged), a Uint8Array, or anything with ffjavascript BigBuffer's
//            surface { byteLength, slice(a, b) -> Uint8Array, set(u8, byteOffset) }; the last two are staged in 256 MB pieces and the
//            result is written back into them
//   opts     { n = what buf holds at this stride, stride = 1 }
//   beta, points   Uint8Array(32) Montgomery bytes (F.e(...)); evaluate returns such arrays
"use strict";
const { addon, isDev } = require("./native.js");

const CHUNK_BYTES = 1 << 28;
const NONE = 0xFFFFFFFFFFFFFFFFn;

function asWords(u8) {       // a BigUint64Array over the same bytes where alignment allows, over a copy otherwise
    if (u8.byteOffset % 8 === 0) return new BigUint64Array(u8.buffer, u8.byteOffset, u8.byteLength / 8);
    const c = new Uint8Array(u8.byteLength); c.set(u8);
    return new BigUint64Array(c.buffer);
}
function byteLength(buf) { return isDev(buf) ? buf.length * 8 : buf.byteLength; }
function elem(u8, what) {
    if (!(u8 instanceof Uint8Array) || u8.byteLength !== 32) throw new Error("polynomial_bn128: " + what + " must be a Uint8Array of 32 bytes");
    return asWords(u8);
}
function shape(buf, opts) {
    const stride = opts.stride === undefined ? 1 : opts.stride;
    if (!Number.isInteger(stride) || stride < 1) throw new Error("polynomial_bn128: stride must be a positive integer");
    const n = opts.n === undefined ? Math.ceil(Math.floor(byteLength(buf) / 32) / stride) : opts.n;
    if (!Number.isInteger(n) || n < 0) throw new Error("polynomial_bn128: bad coefficient count");
    const bytes = n ? ((n - 1) * stride + 1) * 32 : 0;
    if (byteLength(buf) < bytes) throw new Error("polynomial_bn128: the buffer holds " + byteLength(buf) + " bytes, needs " + bytes);
    return { n, stride, bytes };
}
// fn(device address of the coefficients); a staged buffer is uploaded first and, with writeBack, downloaded into buf afterwards
function withResident(buf, bytes, writeBack, fn) {
    if (isDev(buf)) return fn(buf.ptr);
    const p = addon.devAlloc(Math.max(1, bytes / 8));
    try {
        for (let o = 0; o < bytes; o += CHUNK_BYTES) {
            const e = Math.min(bytes, o + CHUNK_BYTES);
            addon.devUpload(p, o / 8, asWords(buf instanceof Uint8Array ? buf.subarray(o, e) : buf.slice(o, e)));
        }
        const res = fn(p);
        for (let o = 0; writeBack && o < bytes; o += CHUNK_BYTES) {
            const t = new BigUint64Array((Math.min(bytes, o + CHUNK_BYTES) - o) / 8);
            addon.devDownload(t, p, o / 8);                  // a synchronous copy: ordered after the kernels
            buf.set(new Uint8Array(t.buffer), o);
        }
        return res;
    } finally {
        addon.devFree(p);
    }
}

// buf <- d, in place; returns buf
function divByXNSubValue(buf, k, beta, opts = {}) {
    const { n, stride, bytes } = shape(buf, opts);
    if (!Number.isInteger(k) || k < 1) throw new Error("polynomial_bn128: k must be a positive integer");
    const b = elem(beta, "beta");
    withResident(buf, bytes, true, (p) => addon.bn128PolyDivDev(p, n, stride, k, b, p));
    return buf;
}

// Polynomial.divZh(domainSize): buf <- the division by x^domainSize - 1, the quotient from element domainSize on; throws the
// reference's "Polynomial is not divisible" when an element below domainSize is left non-zero
function divZh(buf, domainSize, opts = {}) {
    const { n, stride, bytes } = shape(buf, opts);
    if (!Number.isInteger(domainSize) || domainSize < 1) throw new Error("polynomial_bn128: bad domain size");
    const one = new BigUint64Array(4);
    new Uint8Array(one.buffer).set(ONE_MONT);
    let row = NONE;
    withResident(buf, bytes, true, (p) => {
        addon.bn128PolyDivDev(p, n, stride, domainSize, one, p);
        row = addon.bn128FirstNonzeroRowDev(p, stride, 0, 0, Math.min(domainSize, n))[0];
    });
    if (row !== NONE) throw new Error("Polynomial is not divisible");
    return buf;
}

// [p(z) for z of points]; buf is only read
function evaluate(buf, points, opts = {}) {
    const { n, stride, bytes } = shape(buf, opts);
    if (!Array.isArray(points) || points.length < 1 || points.length > 64) throw new Error("polynomial_bn128: 1 to 64 points per call");
    const z = new BigUint64Array(4 * points.length);
    points.forEach((pt, i) => z.set(elem(pt, "a point"), 4 * i));
    const dOut = addon.devAlloc(z.length);
    try {
        withResident(buf, bytes, false, (p) => addon.bn128PolyEvalDev(p, n, stride, z, dOut));
        const out = new BigUint64Array(z.length);
        addon.devDownload(out, dOut, 0);                     // a synchronous copy: ordered after the kernels
        return points.map((_, i) => new Uint8Array(out.buffer.slice(32 * i, 32 * i + 32)));
    } finally {
        addon.devFree(dOut);
    }
}

// 1 in Montgomery form: 2^256 mod r, little-endian
const ONE_MONT = (() => {
    const r = 21888242871839275222246405745257275088548364400416034343698204186575808495617n;
    let v = (1n << 256n) % r;
    const u = new Uint8Array(32);
    for (let i = 0; i < 32; i++) { u[i] = Number(v & 0xFFn); v >>= 8n; }
    return u;
})();

module.exports = { divZh, divByXNSubValue, evaluate };
