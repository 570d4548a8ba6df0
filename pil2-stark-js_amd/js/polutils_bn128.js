// Drop-ins for calculateZ, calculateS (src/helpers/polutils.js:132-164) and F.batchInverse with F = curve.Fr, the field a fflonk stage
// resolves its gprod / gsum hints over (src/prover/hints_helpers.js:92-113), computed by libpil2gl on the MI355X (csrc/bn_scan.hip).
//   calculateZ(F, num, den)   z[0] = 1, z[i] = z[i-1] num[i-1] / den[i-1]
//   calculateS(F, num, den)   s[i] = s[i-1] + num / den[i], num ONE element
//   calculateSCol(F, num, den)   s[i] = s[i-1] + num[i] / den[i], num a column like den (a pil2 gsum hint over a multiplicity; no reference counterpart)
//   batchInverse(F, a)        a[i]^-1
//   calculateH1H2(F, f, t)    [h1, h2] of polutils.js:105-130, the h1h2 hint (hints_helpers.js:115-121; csrc/bn_h1h2.hip): elements are
//                             compared as their 32 bytes; a value of f that t lacks throws the reference's message
// Array forms: arrays of Uint8Array(32), Fr Montgomery bytes (what curve.Fr keeps), in and out; `F` is accepted and ignored.  They are
// packed, staged through device copies and unpacked, as js/polutils.js does for Goldilocks.
// Resident forms (calculateZDev, calculateSDev, calculateSColDev, batchInverseDev): a column is { buf: DevBuffer, stride = 1, offset = 0 }, element i at
// element offset + i * stride of buf (a section of prover_helpers_bn128.js: stride = its width, offset = the column).  Nothing is staged;
// the result is written into the `out` column and `out` is returned.  The hint's `result` field is element n - 1: lastElement(out, n).
// calculateH1H2Dev(f, t, n, h1, h2, stream) writes two columns and returns [h1, h2]; h1 and h2 may be two columns of one section, and
// overlap nothing otherwise.
// A zero denominator inverts to zero and stays out of every running product (include/pil2gl.h): its ratio is 0.
"use strict";
const { addon, isDev, DevBuffer } = require("./native.js");
const { scope, input, output } = require("./bn128_stage.js").native();

function pack(col, what) {
    const a = new BigUint64Array(4 * col.length);
    const bytes = new Uint8Array(a.buffer);
    for (let i = 0; i < col.length; i++) {
        const e = col[i];
        if (!(e instanceof Uint8Array) || e.byteLength !== 32) throw new Error("polutils_bn128: " + what + "[" + i + "] must be a Uint8Array of 32 bytes");
        bytes.set(e, 32 * i);
    }
    return a;
}
// fn([device addresses of the inputs, then of nOut results of n elements]) -> the results, each an array of Uint8Array(32)
function onDevice(arrays, n, nOut, fn) {
    const outs = Array.from({ length: nOut }, () => new Uint8Array(32 * n));
    scope(arrays.map((a) => input(new Uint8Array(a.buffer), a.byteLength)).concat(outs.map((o) => output(o, o.length))), fn);
    return outs.map((o) => Array.from({ length: n }, (_, i) => o.slice(32 * i, 32 * i + 32)));
}

async function calculateZ(F, num, den) {
    const n = den.length;
    if (num.length !== n) throw new Error("polutils_bn128: num and den must have the same length");
    return onDevice([pack(num, "num"), pack(den, "den")], n, 1, ([dn, dd, dz]) => addon.bn128GprodDev(dn, 1, dd, 1, n, dz, 1))[0];
}
async function calculateS(F, num, den) {
    const n = den.length, c = pack([num], "num");
    return onDevice([pack(den, "den")], n, 1, ([dd, ds]) => addon.bn128GsumDev(c, dd, 1, n, ds, 1))[0];
}
async function calculateSCol(F, num, den) {
    const n = den.length;
    if (num.length !== n) throw new Error("polutils_bn128: num and den must have the same length");
    return onDevice([pack(num, "num"), pack(den, "den")], n, 1, ([dn, dd, ds]) => addon.bn128GsumColDev(dn, 1, dd, 1, n, ds, 1))[0];
}
function batchInverse(F, a) {
    const n = a.length;
    return onDevice([pack(a, "a")], n, 1, ([da, di]) => addon.bn128BatchInverseDev(da, 1, n, di, 1))[0];
}

// the reference's message for a value t lacks (polutils.js:115): the row, and the element as F.toString gives it -- the decimal normal form of
// the Montgomery bytes
const FR = 21888242871839275222246405745257275088548364400416034343698204186575808495617n;
const R_INV = 9915499612839321149637521777990102151350674507940716049588462388200839649614n;       // (2^256)^-1 mod r
function decimal(e) {
    let v = 0n;
    for (let i = 31; i >= 0; i--) v = (v << 8n) | BigInt(e[i]);
    return (v * R_INV % FR).toString();
}
function notIncluded(row, e) { return new Error("Number not included: w:" + row + ", value:" + decimal(e)); }

function calculateH1H2(F, f, t) {
    const n = t.length;
    if (f.length !== n) throw new Error("polutils_bn128: f and t must have the same length");
    return onDevice([pack(f, "f"), pack(t, "t")], n, 2, ([df, dt, d1, d2]) => {
        const miss = addon.bn128H1h2Dev(df, 1, dt, 1, n, d1, 1, d2, 1);
        if (miss !== undefined) throw notIncluded(miss, f[Number(miss)]);
    });
}

// ---- resident columns ----
function column(c, n, what) {
    if (!c || !isDev(c.buf)) throw new Error("polutils_bn128: " + what + " must be { buf: DevBuffer, stride, offset }");
    const stride = c.stride === undefined ? 1 : c.stride, offset = c.offset === undefined ? 0 : c.offset;
    if (!Number.isInteger(stride) || stride < 1 || !Number.isInteger(offset) || offset < 0) throw new Error("polutils_bn128: bad stride or offset of " + what);
    const words = n ? 4 * (offset + (n - 1) * stride + 1) : 0;
    if (c.buf.length < words) throw new Error("polutils_bn128: " + what + " holds " + c.buf.length + " words, needs " + words);
    return { ptr: c.buf.addr(4 * offset), stride };
}
function rows(n) {
    if (!Number.isInteger(n) || n < 0) throw new Error("polutils_bn128: bad row count");
    return n;
}
function calculateZDev(num, den, n, out, stream) {
    const a = column(num, rows(n), "num"), b = column(den, n, "den"), o = column(out, n, "out");
    addon.bn128GprodDev(a.ptr, a.stride, b.ptr, b.stride, n, o.ptr, o.stride, stream);
    return out;
}
function calculateSDev(num, den, n, out, stream) {
    if (!(num instanceof Uint8Array) || num.byteLength !== 32) throw new Error("polutils_bn128: num must be a Uint8Array of 32 bytes");
    const b = column(den, rows(n), "den"), o = column(out, n, "out");
    addon.bn128GsumDev(pack([num], "num"), b.ptr, b.stride, n, o.ptr, o.stride, stream);
    return out;
}
function calculateSColDev(num, den, n, out, stream) {
    const a = column(num, rows(n), "num"), b = column(den, n, "den"), o = column(out, n, "out");
    addon.bn128GsumColDev(a.ptr, a.stride, b.ptr, b.stride, n, o.ptr, o.stride, stream);
    return out;
}
// out may be the same column as src (in place)
function batchInverseDev(src, n, out, stream) {
    const a = column(src, rows(n), "src"), o = column(out, n, "out");
    addon.bn128BatchInverseDev(a.ptr, a.stride, n, o.ptr, o.stride, stream);
    return out;
}
function calculateH1H2Dev(f, t, n, h1, h2, stream) {
    const a = column(f, rows(n), "f"), b = column(t, n, "t"), o1 = column(h1, n, "h1"), o2 = column(h2, n, "h2");
    const miss = addon.bn128H1h2Dev(a.ptr, a.stride, b.ptr, b.stride, n, o1.ptr, o1.stride, o2.ptr, o2.stride, stream);
    if (miss !== undefined) {                                     // the message carries the value: download that one element
        const off = 4 * ((f.offset || 0) + Number(miss) * a.stride);
        throw notIncluded(miss, new Uint8Array(f.buf.slice(off, off + 4).buffer));
    }
    return [h1, h2];
}
// the `result` field of a hint: element n - 1 of its column, as Montgomery bytes
function lastElement(col, n) {
    const c = column(col, rows(n), "the column");
    if (n < 1) throw new Error("polutils_bn128: an empty column has no last element");
    const off = 4 * ((col.offset || 0) + (n - 1) * c.stride);
    return new Uint8Array(col.buf.slice(off, off + 4).buffer);
}


// The grand product of a permutation or a connection from the trace columns in one call (js/pil_checks.js grandProduct; include/pil2gl.h
// states it): what calculateZ gives on the two product columns of grandProductPermutation.js / grandProductConnection.js, without them.
// f, t = { buf, stride, cols, sel }; aCols, sCols = arrays of { buf, stride, col }, x = { buf, stride, col }; deltaKs[j] = delta ks'_j;
// out = { buf, stride, col }.  The Dev forms take DevBuffers and only enqueue; the others take host words and write out in place.
function zPermutation(dev, f, t, alpha, beta, gamma, out, n, stream) {
    const pc = require("./pil_checks.js");
    return (dev ? pc.grandProductDev : pc.grandProduct)(pc.permutationTerms(f, t), alpha, beta, gamma, out, n, { bn128: true, stream });
}
function zConnection(dev, aCols, sCols, x, gamma, delta, deltaKs, out, n, stream) {
    const pc = require("./pil_checks.js");
    return (dev ? pc.grandProductDev : pc.grandProduct)(pc.connectionTerms(aCols, sCols, x, delta, deltaKs), gamma, gamma, gamma, out, n, { bn128: true, stream });
}
const calculateZPermutation = (f, t, alpha, beta, gamma, out, n) => zPermutation(false, f, t, alpha, beta, gamma, out, n);
const calculateZPermutationDev = (f, t, alpha, beta, gamma, out, n, stream) => zPermutation(true, f, t, alpha, beta, gamma, out, n, stream);
const calculateZConnection = (aCols, sCols, x, gamma, delta, deltaKs, out, n) => zConnection(false, aCols, sCols, x, gamma, delta, deltaKs, out, n);
const calculateZConnectionDev = (aCols, sCols, x, gamma, delta, deltaKs, out, n, stream) => zConnection(true, aCols, sCols, x, gamma, delta, deltaKs, out, n, stream);

// The plookup argument of pil1 from the trace columns (js/pil_checks.js plookupFold / plookupProduct; include/pil2gl.h states it).
// f, t = { buf, stride, cols, sel } with their own column counts, strides and columns in elements.
//   calculateH1H2Plookup(f, t, alpha, beta, n)            host words -> [h1, h2] as calculateH1H2 returns them (arrays of Uint8Array(32)): the
//                                                         fold into scratch, then calculateH1H2; a value of f that t lacks throws its message
//   calculateH1H2PlookupDev(f, t, alpha, beta, n, stream) DevBuffers -> [h1, h2], the two columns { buf, stride: 2, offset } of ONE new DevBuffer
//                                                         (the caller frees h1.buf), through calculateH1H2Dev
//   calculateZPlookup(f, t, h1, h2, alpha, beta, gamma, delta, out, n)   h1, h2, out = { buf, stride, col }; writes z in place -> out
//   calculateZPlookupDev(.., n, stream)                   the same on DevBuffers; only enqueues
function h1h2Plookup(dev, f, t, alpha, beta, n, stream) {
    const pc = require("./pil_checks.js"), opts = { bn128: true, stream };
    if (!dev) {
        const FT = new BigUint64Array(8 * n), bytes = new Uint8Array(FT.buffer);
        pc.plookupFold(f, t, alpha, beta, { buf: FT, stride: 2, col: 0 }, { buf: FT, stride: 2, col: 1 }, n, opts);
        const col = (c) => Array.from({ length: n }, (_, i) => bytes.slice(64 * i + 32 * c, 64 * i + 32 * c + 32));
        return calculateH1H2(null, col(0), col(1));
    }
    const FT = new DevBuffer(8 * n), H = new DevBuffer(8 * n);
    try {
        pc.plookupFoldDev(f, t, alpha, beta, { buf: FT, stride: 2, col: 0 }, { buf: FT, stride: 2, col: 1 }, n, opts);
        return calculateH1H2Dev({ buf: FT, stride: 2, offset: 0 }, { buf: FT, stride: 2, offset: 1 }, n, { buf: H, stride: 2, offset: 0 }, { buf: H, stride: 2, offset: 1 }, stream);
    } catch (e) { H.free(); throw e; } finally { FT.free(); }
}
function zPlookup(dev, f, t, h1, h2, alpha, beta, gamma, delta, out, n, stream) {
    const pc = require("./pil_checks.js");
    return (dev ? pc.plookupProductDev : pc.plookupProduct)(f, t, h1, h2, alpha, beta, gamma, delta, out, n, { bn128: true, stream });
}
const calculateH1H2Plookup = (f, t, alpha, beta, n) => h1h2Plookup(false, f, t, alpha, beta, n);
const calculateH1H2PlookupDev = (f, t, alpha, beta, n, stream) => h1h2Plookup(true, f, t, alpha, beta, n, stream);
const calculateZPlookup = (f, t, h1, h2, alpha, beta, gamma, delta, out, n) => zPlookup(false, f, t, h1, h2, alpha, beta, gamma, delta, out, n);
const calculateZPlookupDev = (f, t, h1, h2, alpha, beta, gamma, delta, out, n, stream) => zPlookup(true, f, t, h1, h2, alpha, beta, gamma, delta, out, n, stream);
// the grand sum of range checks with the ranges as numbers, no t column (js/pil_checks.js rangeSum): elements are 4 Montgomery words
const calculateSRange = (terms, ranges, alpha, beta, out, n) => require("./pil_checks.js").rangeSum(terms, ranges, alpha, beta, out, n, { bn128: true });
const calculateSRangeDev = (terms, ranges, alpha, beta, out, n, stream) => require("./pil_checks.js").rangeSumDev(terms, ranges, alpha, beta, out, n, { bn128: true, stream });
// s and the im columns of a clustered logUp sum (js/pil_checks.js logupCluster): elements are 4 Montgomery words
const calculateSClustered = (terms, ranges, cluster, im, alpha, beta, out, n) => require("./pil_checks.js").logupCluster(terms, ranges, cluster, im, alpha, beta, out, n, { bn128: true });
const calculateSClusteredDev = (terms, ranges, cluster, im, alpha, beta, out, n, stream) => require("./pil_checks.js").logupClusterDev(terms, ranges, cluster, im, alpha, beta, out, n, { bn128: true, stream });

module.exports = { calculateSClustered, calculateSClusteredDev, calculateSRange, calculateSRangeDev, calculateH1H2Plookup, calculateH1H2PlookupDev, calculateZPlookup, calculateZPlookupDev, calculateZPermutation, calculateZPermutationDev, calculateZConnection, calculateZConnectionDev, calculateZ, calculateS, calculateSCol, batchInverse, calculateH1H2, calculateZDev, calculateSDev, calculateSColDev, batchInverseDev, calculateH1H2Dev, lastElement };
