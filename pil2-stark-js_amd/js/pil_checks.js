// PIL's lookup and permutation identities checked on the device as statements about the trace (csrc/tuple_check.hip; include/pil2gl.h
// states what is checked):
//     selF {f0..fk-1} in selT {t0..tk-1}     checkLookup / checkLookupDev
//     selF {f0..fk-1} is selT {t0..tk-1}     checkPermutation / checkPermutationDev
//   checkLookup(f, t, n, opts) / checkPermutation(f, t, n, opts)
//       f, t: { buf: BigUint64Array | Uint8Array, stride, cols: [..], sel: { buf, stride, col } | undefined } -- a row-major host matrix of n
//       rows of `stride` elements, the tuple's columns in the tuple's order, an optional selector column of a matrix of its own
//   checkLookupDev(f, t, n, opts) / checkPermutationDev(f, t, n, opts)
//       the same with buf a DevBuffer: sections of the stage-1 buffer, before it is committed; f and t may be one buffer
//   opts.bn128: elements are 32-byte Montgomery values of curve.Fr instead of Goldilocks words
//   -> null when the trace is clean, else { kind, row, partner, cntF, cntT, side, message() }: include/pil2gl.h's five words; side = "f" for
//      kinds 1 and 2, "t" for kind 3; message() reads the reported row's k elements back, and only when it is called
//   formatReport(report, values, name)   the message from the five words and the tuple's values as decimal strings
//   tupleHome(words, k, capacity, bn128), tupleCheckProbe()   the library's two debug entries
// Node 12: no optional chaining.
"use strict";
const { addon, DevBuffer, isDev } = require("./native.js");
const stage = require("./bn128_stage.js");

const GL_P = 0xFFFFFFFF00000001n;
const FR = 21888242871839275222246405745257275088548364400416034343698204186575808495617n;
const FR_R_INV = 9915499612839321149637521777990102151350674507940716049588462388200839649614n;       // (2^256)^-1 mod r
const NONE = 0xFFFFFFFFFFFFFFFFn;
const LOOKUP = 0, PERMUTATION = 1;

// an element's words as the decimal the reference's F.toString prints: the value mod p, the normal form of Montgomery words
function decimalOf(wordsOfElem) {
    if (wordsOfElem.length === 1) return (wordsOfElem[0] % GL_P).toString();
    let v = 0n;
    for (let k = 3; k >= 0; k--) v = (v << 64n) | wordsOfElem[k];
    return (v % FR * FR_R_INV % FR).toString();
}
// The wording, once (INTEGRATION.md):
//   kind 1  "<name>: f row R = (v0, v1, ..) occurs in no selected row of t (cntF = A, cntT = 0)"
//   kind 2  "<name>: f row R = (v0, v1, ..) occurs A times in f and B times in t, first in t at row Q (cntF = A, cntT = B)"
//   kind 3  "<name>: t row R = (v0, v1, ..) occurs B times in t and A times in f, first in f at row Q | nowhere in f (cntF = A, cntT = B)"
function formatReport(r, values, name) {
    const tup = "(" + values.join(", ") + ")", counts = " (cntF = " + r.cntF + ", cntT = " + r.cntT + ")";
    if (r.kind === 1) return name + ": f row " + r.row + " = " + tup + " occurs in no selected row of t" + counts;
    if (r.kind === 2) return name + ": f row " + r.row + " = " + tup + " occurs " + r.cntF + " times in f and " + r.cntT + " times in t, first in t at row " + r.partner + counts;
    return name + ": t row " + r.row + " = " + tup + " occurs " + r.cntT + " times in t and " + r.cntF + " times in f, " +
        (r.partner === null ? "nowhere in f" : "first in f at row " + r.partner) + counts;
}
function report(rep, mode, sides, ew, read) {
    const kind = Number(rep[0]);
    if (!kind) return null;
    const r = { kind, row: Number(rep[1]), partner: rep[2] === NONE ? null : Number(rep[2]), cntF: Number(rep[3]), cntT: Number(rep[4]), side: kind === 3 ? "t" : "f" };
    r.message = () => {
        const s = sides[r.side];
        return formatReport(r, s.cols.map((c) => decimalOf(read(s.buf, (r.row * s.stride + c) * ew, ew))), mode === LOOKUP ? "lookup" : "permutation");
    };
    return r;
}

// one side as the addon's description takes it
function side(x, what, n, ew, dev) {
    if (!x || !Array.isArray(x.cols) || !(x.stride > 0)) throw new Error(what + " must be { buf, stride, cols: [..] }");
    const matrix = (m, top, name) => {
        if (dev !== isDev(m.buf)) throw new Error(name + ": buf must be a " + (dev ? "DevBuffer" : "BigUint64Array or Uint8Array"));
        const buf = dev ? m.buf : stage.asWords(m.buf);
        if (n && buf.length < ((n - 1) * m.stride + top + 1) * ew) throw new Error(name + " holds " + buf.length + " words, " + n + " rows of " + m.stride + " elements need more");
        return buf;
    };
    const out = { buf: matrix(x, Math.max(0, ...x.cols), what), stride: x.stride, cols: x.cols, sel: null };
    if (x.sel) out.sel = { buf: matrix({ buf: x.sel.buf, stride: x.sel.stride }, x.sel.col, "the selector of " + what), stride: x.sel.stride, col: x.sel.col };
    return out;
}
function describe(f, t, n, mode, dev) {
    const k = f.cols.length;
    if (t.cols.length !== k) throw new Error("f has " + k + " columns and t " + t.cols.length);
    const ptr = (b) => dev && b ? b.ptr : 0n, sel = (s) => s.sel ? [ptr(s.sel.buf), s.sel.stride, s.sel.col] : [0n, 0, 0];
    return BigUint64Array.from([ptr(f.buf), f.stride, ptr(t.buf), t.stride].concat(sel(f), sel(t), [n, k, mode], f.cols, t.cols).map((v) => BigInt(v)));
}
function check(mode, dev, fIn, tIn, n, opts) {
    const ew = opts && opts.bn128 ? 4 : 1;
    const f = side(fIn, "f", n, ew, dev), t = side(tIn, "t", n, ew, dev), rep = new BigUint64Array(5);
    const desc = describe(f, t, n, mode, dev);
    if (!dev) {
        addon.tupleCheck(desc, f.buf, t.buf, f.sel ? f.sel.buf : null, t.sel ? t.sel.buf : null, rep, ew);
        return report(rep, mode, { f, t }, ew, (buf, at, len) => buf.subarray(at, at + len));
    }
    const plan = addon.tupleCheckPlan(n, f.cols.length, ew, mode);
    const work = new DevBuffer(Math.max(2, plan.scratchBytes / 8));
    try { addon.tupleCheckDev(desc, work.ptr, plan.scratchBytes, rep, ew); } finally { work.free(); }
    return report(rep, mode, { f, t }, ew, (buf, at, len) => buf.slice(at, at + len));
}
const checkLookup = (f, t, n, opts) => check(LOOKUP, false, f, t, n, opts);
const checkPermutation = (f, t, n, opts) => check(PERMUTATION, false, f, t, n, opts);
const checkLookupDev = (f, t, n, opts) => check(LOOKUP, true, f, t, n, opts);
const checkPermutationDev = (f, t, n, opts) => check(PERMUTATION, true, f, t, n, opts);

function tupleHome(words, k, capacity, bn128) {
    const h = addon.tupleHome(stage.asWords(words), k, bn128 ? 4 : 1, capacity);
    if (h === NONE) throw new Error("tupleHome: k is 1 .. 16 and the capacity a power of two");
    return Number(h);
}
const tupleCheckProbe = () => Number(addon.tupleCheckProbe());

module.exports = { checkLookup, checkPermutation, checkLookupDev, checkPermutationDev, formatReport, tupleHome, tupleCheckProbe, LOOKUP, PERMUTATION };
