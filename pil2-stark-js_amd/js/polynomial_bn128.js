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
//
// What open does between its evaluations and its divisions -- Polynomial.add, sub, mulScalar, byXSubValue, byXNSubValue, degree -- is
// one more library form (csrc/bn_polymul.hip): acc[i] <- scale acc[i] + sum_j coef_j src[i - exp_j], the product of src by the sparse
// polynomial sum_j coef_j x^exp_j added to the scaled accumulator.  fma is that form; the others are its special cases.
//   terms    [{ coef: Uint8Array(32) Montgomery bytes, exp: integer }], 1 to 64 of them, exponents strictly increasing;
//            zerofierTerms(factors) multiplies prod_j (x^k_j - beta_j) out into such a list on the host
//   a shifted product is never in place: the result goes to a second buffer (as the reference's byXSubValue fills a new BigBuffer),
//   which must hold src's coefficients + the largest exponent
"use strict";
const { addon } = require("./native.js");
const { byteLength, scope, input, output, inout, asWords } = require("./bn128_stage.js").native();

const NONE = 0xFFFFFFFFFFFFFFFFn;

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
// buf <- d, in place; returns buf
function divByXNSubValue(buf, k, beta, opts = {}) {
    const { n, stride, bytes } = shape(buf, opts);
    if (!Number.isInteger(k) || k < 1) throw new Error("polynomial_bn128: k must be a positive integer");
    const b = elem(beta, "beta");
    scope([inout(buf, bytes)], ([p]) => addon.bn128PolyDivDev(p, n, stride, k, b, p));
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
    scope([inout(buf, bytes)], ([p]) => {
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
    const out = new Uint8Array(32 * points.length);
    scope([input(buf, bytes), output(out, out.length)], ([p, dOut]) => addon.bn128PolyEvalDev(p, n, stride, z, dOut));
    return points.map((_, i) => out.slice(32 * i, 32 * i + 32));
}

// 1 in Montgomery form: 2^256 mod r, little-endian
const ONE_MONT = (() => {
    const r = 21888242871839275222246405745257275088548364400416034343698204186575808495617n;
    let v = (1n << 256n) % r;
    const u = new Uint8Array(32);
    for (let i = 0; i < 32; i++) { u[i] = Number(v & 0xFFn); v >>= 8n; }
    return u;
})();


// ---- products with a sparse polynomial, scaled sums, degree ----
const R = 21888242871839275222246405745257275088548364400416034343698204186575808495617n;
const MONT = (1n << 256n) % R, MONT_INV = (() => {     // 2^-256 mod r by Fermat
    let b = MONT, e = R - 2n, v = 1n;
    for (; e; e >>= 1n) { if (e & 1n) v = v * b % R; b = b * b % R; }
    return v;
})();
function fromMont(u8) { let v = 0n; for (let i = 31; i >= 0; i--) v = (v << 8n) | BigInt(u8[i]); return v * MONT_INV % R; }
function toMont(x) {
    let v = ((x % R) + R) % R * MONT % R;
    const u = new Uint8Array(32);
    for (let i = 0; i < 32; i++) { u[i] = Number(v & 0xFFn); v >>= 8n; }
    return u;
}
const MINUS_ONE_MONT = toMont(R - 1n);

// prod_j (x^k_j - beta_j) for factors = [{ k: positive integer, beta: Uint8Array(32) }], multiplied out with BigInt arithmetic mod r ->
// terms (zero coefficients dropped); more than 64 terms is refused, as the library would
function zerofierTerms(factors) {
    if (!Array.isArray(factors)) throw new Error("polynomial_bn128: factors must be an array of { k, beta }");
    let poly = new Map([[0, 1n]]);
    for (const f of factors) {
        if (!Number.isInteger(f.k) || f.k < 1) throw new Error("polynomial_bn128: k must be a positive integer");
        elem(f.beta, "beta");
        const b = fromMont(f.beta), next = new Map();
        for (const [e, c] of poly) {
            next.set(e + f.k, ((next.get(e + f.k) || 0n) + c) % R);
            next.set(e, ((next.get(e) || 0n) + (R - b) * c) % R);
        }
        for (const [e, c] of next) if (c === 0n) next.delete(e);
        if (next.size > 64) throw new Error("polynomial_bn128: the zerofier has " + next.size + " terms, at most 64");
        poly = next;
    }
    return [...poly.keys()].sort((x, y) => x - y).map((e) => ({ coef: toMont(poly.get(e)), exp: e }));
}

function packTerms(terms) {
    if (!Array.isArray(terms) || terms.length < 1 || terms.length > 64) throw new Error("polynomial_bn128: 1 to 64 terms per call");
    const coefs = new BigUint64Array(4 * terms.length), exps = new BigUint64Array(terms.length);
    terms.forEach((t, j) => {
        if (!Number.isInteger(t.exp) || t.exp < 0) throw new Error("polynomial_bn128: an exponent must be a non-negative integer");
        coefs.set(elem(t.coef, "a coefficient"), 4 * j);
        exps[j] = BigInt(t.exp);
    });
    return { coefs, exps };
}

// acc[i] <- scale acc[i] + sum_j coef_j src[i - exp_j], i < nAcc; src counts as zero outside [0, nSrc).  opts = { nAcc, nSrc = what the
// buffers hold, accStride = 1, srcStride = 1, scale = Uint8Array(32) | null }: with scale null (the default) acc is written and never
// read.  acc may be src itself only with terms = [{ coef, exp: 0 }].  Returns acc.
function fma(acc, src, terms, opts = {}) {
    const a = shape(acc, { n: opts.nAcc, stride: opts.accStride });
    const s = src === null || src === undefined ? { n: 0, stride: 1, bytes: 0 } : shape(src, { n: opts.nSrc, stride: opts.srcStride });
    const { coefs, exps } = packTerms(terms);
    const scale = opts.scale === undefined || opts.scale === null ? null : elem(opts.scale, "scale");
    const run = (pa, ps) => addon.bn128PolyFmaDev(pa, a.n, a.stride, scale, ps, s.n, s.stride, coefs, exps);
    const bufs = [inout(acc, a.bytes)];                      // acc === src is one copy; no src, or an empty one, is address 0
    if (src === acc || s.n) bufs.push(input(src, s.bytes));
    scope(bufs, ([pa, ps = 0n]) => run(pa, ps));
    return acc;
}

const one = (coef) => [{ coef, exp: 0 }];
// Polynomial.add / sub: acc <- acc + src, acc <- acc - src (src no longer than acc); opts = { nAcc, nSrc, accStride, srcStride }
function add(acc, src, opts = {}) { return fma(acc, src, one(ONE_MONT), Object.assign({}, opts, { scale: ONE_MONT })); }
function sub(acc, src, opts = {}) { return fma(acc, src, one(MINUS_ONE_MONT), Object.assign({}, opts, { scale: ONE_MONT })); }
// Polynomial.mulScalar: buf <- value buf, in place; opts = { n, stride }
function mulScalar(buf, value, opts = {}) {
    return fma(buf, buf, one(value), { nAcc: opts.n, nSrc: opts.n, accStride: opts.stride, srcStride: opts.stride });
}
// dst <- src times the sparse polynomial `terms`; opts = { n = what src holds, stride = 1, dstStride = 1 }; dst takes n + the largest
// exponent coefficients and must not be src
function mulSparse(src, terms, dst, opts = {}) {
    const { n } = shape(src, opts);
    if (!Array.isArray(terms) || !terms.length) throw new Error("polynomial_bn128: 1 to 64 terms per call");
    const top = terms[terms.length - 1].exp;
    return fma(dst, src, terms, { nAcc: n + top, nSrc: n, accStride: opts.dstStride, srcStride: opts.stride });
}
// Polynomial.byXSubValue(v) / byXNSubValue(n, v): dst <- src (x - v), dst <- src (x^n - v)
function byXNSubValue(src, n, value, dst, opts = {}) {
    if (!Number.isInteger(n) || n < 1) throw new Error("polynomial_bn128: n must be a positive integer");
    return mulSparse(src, [{ coef: toMont(R - fromMont(elem8(value))), exp: 0 }, { coef: ONE_MONT, exp: n }], dst, opts);
}
function byXSubValue(src, value, dst, opts = {}) { return byXNSubValue(src, 1, value, dst, opts); }
function elem8(u8) { elem(u8, "value"); return u8; }

// Polynomial.degree: the largest index whose coefficient is not zero; -1 for the zero polynomial (and for no coefficients)
function degree(buf, opts = {}) {
    const { n, stride, bytes } = shape(buf, opts);
    if (n === 0) return -1;
    const d = scope([input(buf, bytes)], ([p]) => addon.bn128PolyDegreeDev(p, n, stride));
    return d === NONE ? -1 : Number(d);
}

module.exports = { divZh, divByXNSubValue, evaluate, fma, add, sub, mulScalar, byXSubValue, byXNSubValue, mulSparse, degree, zerofierTerms };
