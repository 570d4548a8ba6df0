// Drop-ins for the data-parallel functions of src/helpers/polutils.js, same names and argument lists:
//   buildZhInv(buffTo, offset, F, nBits, nBitsExt, stark)                                   polutils.js:39-55
//   buildOneRowZerofierInv(buffTo, offset, F, buffZhInv, nBits, nBitsExt, rowIndex, stark)  polutils.js:57-71
//   buildFrameZerofierInv(buffTo, offset, F, buffZhInv, nBits, nBitsExt, frame, stark)      polutils.js:74-102
//   calculateZ(F, num, den), calculateS(F, num, den), calculateH1H2(F, f, t)                polutils.js:105-164
// and, beside them, the grand sum with a COLUMN numerator that a pil2 gsum hint over a multiplicity needs (no reference counterpart):
//   calculateSCol(F, num, den)                          s[i] = s[i-1] + num[i] / den[i], num an array like den
//   calculateSColDev(num, dimNum, den, dimDen, n, out, stream)   the same on DevBuffers (dense columns of dim 1 or 3); only enqueues; -> out
// `F` and `buffZhInv` are accepted and ignored (the field is Goldilocks, the device rebuilds what it needs).
// Only the stark = true forms exist (coset 7 * <w>): the plain-subgroup forms invert zero and are not used by the prover.
// One deviation, on purpose: buildZhInv honours `offset` when it fills rows >= 2^extendBits; the reference's second loop
// (polutils.js:51-53) ignores it and overwrites the table at offset 0 (harmless there because everyRow is boundary 0).
"use strict";
const { addon, isFlat, isDev, download, DevBuffer } = require("./native.js");

function setRange(buffTo, offset, tmp) {
    if (isFlat(buffTo)) buffTo.set(tmp, offset); else buffTo.set(tmp, offset);
}
function withOut(n, fn, buffTo, offset) {
    if (isDev(buffTo)) { fn(buffTo.addr(offset)); return; }         // resident table: written in place
    const d = addon.devAlloc(n);
    try {
        fn(d);
        const CH = 1 << 24;
        for (let o = 0; o < n; o += CH) {
            const tmp = new BigUint64Array(Math.min(CH, n - o));
            addon.devDownload(tmp, d, o);
            setRange(buffTo, offset + o, tmp);
        }
    } finally { addon.devFree(d); }
}
function needStark(stark) { if (!stark) throw new Error("only the stark (coset) form is implemented"); }

module.exports.buildZhInv = function buildZhInv(buffTo, offset, F, nBits, nBitsExt, stark) {
    needStark(stark);
    withOut(1 << nBitsExt, (d) => addon.buildZhInvDev(nBits, nBitsExt, d), buffTo, offset);
};
module.exports.buildOneRowZerofierInv = function buildOneRowZerofierInv(buffTo, offset, F, buffZhInv, nBits, nBitsExt, rowIndex, stark) {
    needStark(stark);
    withOut(1 << nBitsExt, (d) => addon.buildOneRowZerofierInvDev(nBits, nBitsExt, rowIndex, d), buffTo, offset);
};
module.exports.buildFrameZerofierInv = function buildFrameZerofierInv(buffTo, offset, F, buffZhInv, nBits, nBitsExt, frame, stark) {
    needStark(stark);
    withOut(1 << nBitsExt, (d) => addon.buildFrameZerofierDev(nBits, nBitsExt, frame.offsetMin, frame.offsetMax, d), buffTo, offset);
};

// columns as the reference passes them: arrays of BigInt (dim 1) or of [a,b,c] (dim 3)
function pack(col) {
    const dim = Array.isArray(col[0]) ? 3 : 1;
    const a = new BigUint64Array(col.length * dim);
    if (dim === 1) for (let i = 0; i < col.length; i++) a[i] = BigInt(col[i]);
    else for (let i = 0; i < col.length; i++) { a[3 * i] = BigInt(col[i][0]); a[3 * i + 1] = BigInt(col[i][1]); a[3 * i + 2] = BigInt(col[i][2]); }
    return { a, dim };
}
function unpack(a, dim) {
    const n = a.length / dim, out = new Array(n);
    if (dim === 1) for (let i = 0; i < n; i++) out[i] = a[i];
    else for (let i = 0; i < n; i++) out[i] = [a[3 * i], a[3 * i + 1], a[3 * i + 2]];
    return out;
}
function onDevice(arrays, nOutWords, fn) {
    const ptrs = [];
    try {
        for (const a of arrays) { const d = addon.devAlloc(a.length); ptrs.push(d); addon.devUpload(d, 0, a); }
        const outs = nOutWords.map((n) => { const d = addon.devAlloc(n); ptrs.push(d); return d; });
        fn(ptrs.slice(0, arrays.length), outs);
        return outs.map((d, i) => { const r = new BigUint64Array(nOutWords[i]); addon.devDownload(r, d, 0); return r; });
    } finally { for (const d of ptrs) addon.devFree(d); }
}

module.exports.calculateZ = async function calculateZ(F, num, den) {
    const N = den.length, pn = pack(num), pd = pack(den), dimOut = Math.max(pn.dim, pd.dim);
    const [z] = onDevice([pn.a, pd.a], [N * dimOut], ([dn, dd], [dz]) => addon.gprodDev(dn, pn.dim, dd, pd.dim, N, dz));
    return unpack(z, dimOut);
};
module.exports.calculateS = async function calculateS(F, num, den) {
    const N = den.length, pn = pack([num]), pd = pack(den), dimOut = Math.max(pn.dim, pd.dim);
    const [s] = onDevice([pn.a, pd.a], [N * dimOut], ([dn, dd], [ds]) => addon.gsumDev(dn, pn.dim, dd, pd.dim, N, ds));
    return unpack(s, dimOut);
};
module.exports.calculateSCol = async function calculateSCol(F, num, den) {
    const N = den.length, pn = pack(num), pd = pack(den), dimOut = Math.max(pn.dim, pd.dim);
    if (num.length !== N) throw new Error("calculateSCol: num and den must have the same length");
    const [s] = onDevice([pn.a, pd.a], [N * dimOut], ([dn, dd], [ds]) => addon.gsumColDev(dn, pn.dim, dd, pd.dim, N, ds));
    return unpack(s, dimOut);
};
module.exports.calculateSColDev = function calculateSColDev(num, dimNum, den, dimDen, n, out, stream) {
    const dimOut = Math.max(dimNum, dimDen);
    for (const [b, words, what] of [[num, n * dimNum, "num"], [den, n * dimDen, "den"], [out, n * dimOut, "out"]])
        if (!isDev(b) || b.length < words) throw new Error("calculateSColDev: " + what + " must be a DevBuffer of at least " + words + " words");
    addon.gsumColDev(num.ptr, dimNum, den.ptr, dimDen, n, out.ptr, stream);
    return out;
};
module.exports.calculateH1H2 = function calculateH1H2(F, f, t) {
    const pf = pack(f), pt = pack(t);
    if (pf.dim !== pt.dim || f.length !== t.length) throw new Error("calculateH1H2: f and t must have the same shape");
    const n = t.length;
    const [h1, h2] = onDevice([pf.a, pt.a], [n * pt.dim, n * pt.dim], ([df, dt], [d1, d2]) => addon.h1h2Dev(df, dt, n, pt.dim, d1, d2));
    return [unpack(h1, pt.dim), unpack(h2, pt.dim)];
};


// The grand product of a permutation or a connection from the trace columns in one call (js/pil_checks.js grandProduct; include/pil2gl.h
// states it): what calculateZ gives on the two product columns of grandProductPermutation.js / grandProductConnection.js, without them.
// f, t = { buf, stride, cols, sel }; aCols, sCols = arrays of { buf, stride, col }, x = { buf, stride, col }; deltaKs[j] = delta ks'_j;
// out = { buf, stride, col }.  The Dev forms take DevBuffers and only enqueue; the others take host words and write out in place.
function zPermutation(dev, f, t, alpha, beta, gamma, out, n, stream) {
    const pc = require("./pil_checks.js");
    return (dev ? pc.grandProductDev : pc.grandProduct)(pc.permutationTerms(f, t), alpha, beta, gamma, out, n, { bn128: false, stream });
}
function zConnection(dev, aCols, sCols, x, gamma, delta, deltaKs, out, n, stream) {
    const pc = require("./pil_checks.js");
    return (dev ? pc.grandProductDev : pc.grandProduct)(pc.connectionTerms(aCols, sCols, x, delta, deltaKs), gamma, gamma, gamma, out, n, { bn128: false, stream });
}
const calculateZPermutation = (f, t, alpha, beta, gamma, out, n) => zPermutation(false, f, t, alpha, beta, gamma, out, n);
const calculateZPermutationDev = (f, t, alpha, beta, gamma, out, n, stream) => zPermutation(true, f, t, alpha, beta, gamma, out, n, stream);
const calculateZConnection = (aCols, sCols, x, gamma, delta, deltaKs, out, n) => zConnection(false, aCols, sCols, x, gamma, delta, deltaKs, out, n);
const calculateZConnectionDev = (aCols, sCols, x, gamma, delta, deltaKs, out, n, stream) => zConnection(true, aCols, sCols, x, gamma, delta, deltaKs, out, n, stream);
Object.assign(module.exports, { calculateZPermutation, calculateZPermutationDev, calculateZConnection, calculateZConnectionDev });


// The plookup argument of pil1 from the trace columns (js/pil_checks.js plookupFold / plookupProduct; include/pil2gl.h states it).
// f, t = { buf, stride, cols, sel } with their own column counts; hDim = words of an h element (3, or 1 when kF = kT = 1 and there is no selT).
//   calculateH1H2Plookup(f, t, alpha, beta, n, hDim)        host words -> [h1, h2], dense BigUint64Arrays of n hDim words: the fold into
//                                                           scratch, then calculateH1H2's device call; a value of f that t lacks throws its error
//   calculateH1H2PlookupDev(f, t, alpha, beta, n, hDim, stream)   DevBuffers -> [h1, h2], new dense DevBuffers (the caller frees them)
//   calculateZPlookup(f, t, h1, h2, alpha, beta, gamma, delta, out, n, hDim)   h1, h2, out = { buf, stride, col }; writes z in place -> out
//   calculateZPlookupDev(.., hDim, stream)                  the same on DevBuffers; only enqueues
function h1h2Plookup(dev, f, t, alpha, beta, n, hDim, stream) {
    const pc = require("./pil_checks.js"), dim = hDim === undefined ? 3 : hDim, opts = { bn128: false, hDim: dim, stream };
    if (!dev) {
        const F = new BigUint64Array(n * dim), T = new BigUint64Array(n * dim);
        pc.plookupFold(f, t, alpha, beta, { buf: F, stride: dim, col: 0 }, { buf: T, stride: dim, col: 0 }, n, opts);
        return onDevice([F, T], [n * dim, n * dim], ([df, dt], [d1, d2]) => addon.h1h2Dev(df, dt, n, dim, d1, d2));
    }
    const bufs = [0, 1, 2, 3].map(() => new DevBuffer(n * dim));
    try {
        pc.plookupFoldDev(f, t, alpha, beta, { buf: bufs[0], stride: dim, col: 0 }, { buf: bufs[1], stride: dim, col: 0 }, n, opts);
        addon.h1h2Dev(bufs[0].ptr, bufs[1].ptr, n, dim, bufs[2].ptr, bufs[3].ptr, stream);
    } catch (e) { bufs[2].free(); bufs[3].free(); throw e; } finally { bufs[0].free(); bufs[1].free(); }
    return [bufs[2], bufs[3]];
}
function zPlookup(dev, f, t, h1, h2, alpha, beta, gamma, delta, out, n, hDim, stream) {
    const pc = require("./pil_checks.js");
    return (dev ? pc.plookupProductDev : pc.plookupProduct)(f, t, h1, h2, alpha, beta, gamma, delta, out, n, { bn128: false, hDim: hDim === undefined ? 3 : hDim, stream });
}
const calculateH1H2Plookup = (f, t, alpha, beta, n, hDim) => h1h2Plookup(false, f, t, alpha, beta, n, hDim);
const calculateH1H2PlookupDev = (f, t, alpha, beta, n, hDim, stream) => h1h2Plookup(true, f, t, alpha, beta, n, hDim, stream);
const calculateZPlookup = (f, t, h1, h2, alpha, beta, gamma, delta, out, n, hDim) => zPlookup(false, f, t, h1, h2, alpha, beta, gamma, delta, out, n, hDim);
const calculateZPlookupDev = (f, t, h1, h2, alpha, beta, gamma, delta, out, n, hDim, stream) => zPlookup(true, f, t, h1, h2, alpha, beta, gamma, delta, out, n, hDim, stream);
Object.assign(module.exports, { calculateH1H2Plookup, calculateH1H2PlookupDev, calculateZPlookup, calculateZPlookupDev });

// The grand sum of range checks from the f columns, the multiplicities and the ranges as numbers, no t column (js/pil_checks.js rangeSum;
// include/pil2gl.h states it): terms = 0 .. 8 f terms, ranges = 1 .. 8 of { m, lo, size, row0, coef, busId }, out = { buf, stride, col }.
//   calculateSRange(terms, ranges, alpha, beta, out, n)               host words; writes s in place -> out
//   calculateSRangeDev(terms, ranges, alpha, beta, out, n, stream)    the same on DevBuffers; only enqueues
const calculateSRange = (terms, ranges, alpha, beta, out, n) => require("./pil_checks.js").rangeSum(terms, ranges, alpha, beta, out, n, { bn128: false });
const calculateSRangeDev = (terms, ranges, alpha, beta, out, n, stream) => require("./pil_checks.js").rangeSumDev(terms, ranges, alpha, beta, out, n, { bn128: false, stream });
Object.assign(module.exports, { calculateSRange, calculateSRangeDev });

// s and the im columns of a clustered logUp sum in one call (js/pil_checks.js logupCluster; include/pil2gl.h states it): cluster holds an
// entry a term, f terms first, a cluster id or pil_checks.DIRECT; im one { buf, stride, col } a cluster.
//   calculateSClustered(terms, ranges, cluster, im, alpha, beta, out, n)               host words; writes in place -> out
//   calculateSClusteredDev(terms, ranges, cluster, im, alpha, beta, out, n, stream)    the same on DevBuffers; only enqueues
const calculateSClustered = (terms, ranges, cluster, im, alpha, beta, out, n) => require("./pil_checks.js").logupCluster(terms, ranges, cluster, im, alpha, beta, out, n, { bn128: false });
const calculateSClusteredDev = (terms, ranges, cluster, im, alpha, beta, out, n, stream) => require("./pil_checks.js").logupClusterDev(terms, ranges, cluster, im, alpha, beta, out, n, { bn128: false, stream });
Object.assign(module.exports, { calculateSClustered, calculateSClusteredDev });
