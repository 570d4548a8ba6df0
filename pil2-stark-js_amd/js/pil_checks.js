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
// and the multiplicity column a pil2 grand sum needs to PROVE the lookups `selF_s {f_s} in selT {t}` (csrc/lookup_mult.hip):
//   lookupMultiplicities(fs, t, m, n, opts) / lookupMultiplicitiesDev(fs, t, m, n, opts)
//       fs: 1 .. 8 sides as above, t: one side, m: { buf, stride, col } -- the column written, for every row j < n: how many selected rows of
//       all fs hold the tuple of row j of t, at the tuple's first selected row of t, 0 elsewhere; m may be a spare column of t's or an f's buffer
//   -> { matched, missing: null | { side, row, message() } }: matched = the selected f rows whose tuple t holds (the sum of m); missing = the
//      smallest (side, row) of f whose tuple no selected row of t holds; m is written in full either way
//   formatMissing(missing, values)   the message; lookupMultProbe()   the library's debug entry
// and the same column for a range check `selF_s f_s in [lo, lo + size)`, which has no table column (csrc/range_mult.hip):
//   rangeMultiplicities(fs, lo, size, m, n, opts) / rangeMultiplicitiesDev(fs, lo, size, m, n, opts)
//       fs: 1 .. 8 sides as above with ONE column each; lo: a BigInt or an integer, negative allowed (a signed 64-bit value); size: 1 .. 2^28;
//       m: { buf, stride, col }: rows opts.row0 (0) .. row0 + size - 1 take the counts of lo, lo + 1, ..; every other row of the n takes 0
//   -> { matched, missing: null | { side, row, message() } } as above; missing = the smallest (side, row) whose value is out of range
//   formatOutOfRange(missing, value, lo, size)   the message; rangeMultPlan(n, size, nF, bn128)   the library's plan
// and the grand-sum column that consumes m (csrc/logup_sum_plan.h; include/pil2gl.h states it):
//   logupSum(terms, alpha, beta, out, n, opts) / logupSumDev(terms, alpha, beta, out, n, opts)
//       terms: 1 .. 9 sides as above, each with coef and busId beside buf / stride / cols / sel: a BigInt (canonical) over Goldilocks, a
//       BigUint64Array(4) or Uint8Array(32) of Montgomery words with opts.bn128; sel is the NUMERATOR column (its field value multiplies
//       coef; for t it is m) or undefined for 1.  alpha, beta: BigUint64Array(3), a cubic-extension element; BigUint64Array(4) /
//       Uint8Array(32) with opts.bn128.  out: { buf, stride, col }: over Goldilocks the words col .. col + 2 of a row of `stride` words,
//       over Fr one element.  Written in place for every row; s[n-1] is the hint's result.  logupSumDev only enqueues (opts.stream).
//   logupSumPlan(n, nTerms, bn128)   the library's plan
//   rangeSum(terms, ranges, alpha, beta, out, n, opts) / rangeSumDev(..) / rangeSumPlan(n, nF, nR, bn128)
//       logupSum with the table side of a range check given as numbers (csrc/range_sum_plan.h): terms: 0 .. 8 f terms as above; ranges:
//       1 .. 8 of { m: { buf, stride, col }, lo, size, row0, coef, busId } -- lo a BigInt or an integer (signed 64-bit), coef and busId as a
//       term's.  No t column exists; outside rows row0 .. row0 + size - 1 a range adds 0 and m is not read.  rangeSumDev only enqueues.
//   logupCluster(terms, ranges, cluster, im, alpha, beta, out, n, opts) / logupClusterDev(..) / logupClusterPlan(n, nF, nR, nIm, bn128)
//       s AND one im column a cluster in one call (csrc/logup_cluster_plan.h): terms and ranges as above, either may be empty; cluster: an
//       entry a term, f terms first, 0 .. im.length - 1 or DIRECT; im: { buf, stride, col } a cluster, of out's shape.  s and the im columns
//       are normally columns of one matrix: give the same buf.  logupClusterDev only enqueues.
//   grandProduct(terms, alpha, beta, gamma, out, n, opts) / grandProductDev(..) / grandProductPlan(n, nTerms, sumK, bn128)
//       the column z of a permutation or a connection from the trace columns (include/pil2gl.h states it); permutationTerms and
//       connectionTerms build the term lists of the reference's two identities
//   plookupFold(f, t, alpha, beta, outF, outT, n, opts) / plookupFoldDev(..)      the two kept expressions F and T of a pil1 plookup
//   plookupProduct(f, t, h1, h2, alpha, beta, gamma, delta, out, n, opts) / plookupProductDev(..) / plookupPlan(n, kF, kT, bn128)
//       the column z of a pil1 plookup from f, t, h1 and h2 (include/pil2gl.h states it); opts.hDim: words of an h element over
//       Goldilocks (3, or 1 for a base column)
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

// ---- lookup multiplicities ----
// The wording, once (INTEGRATION.md):
//   "lookup: f side S row R = (v0, v1, ..) occurs in no selected row of t"
const formatMissing = (x, values) => "lookup: f side " + x.side + " row " + x.row + " = (" + values.join(", ") + ") occurs in no selected row of t";
// What the two multiplicity calls share.  The arguments every one refuses alike:
function checkMultArgs(fsIn, mIn) {
    if (!Array.isArray(fsIn) || fsIn.length < 1 || fsIn.length > 8) throw new Error("fs must be an array of 1 .. 8 sides");
    if (!mIn || !(mIn.stride > 0) || !(mIn.col >= 0)) throw new Error("m must be { buf, stride, col }");
}
// the caller's bytes from the words the addon wrote, where asWords copied (bytes off 8)
function copyBack(words, given) {
    if (words.buffer !== given.buffer) new Uint8Array(given.buffer, given.byteOffset, given.byteLength).set(new Uint8Array(words.buffer));
}
// the host matrices as the addon's array takes them: a side's matrix, then its selector's or null
const matrices = (sides) => [].concat(...sides.map((x) => [x.buf, x.sel ? x.sel.buf : null]));
// The call itself: the sides (tIn null: no table side), their six words in pil2gl_tuple_side's order, m written and copied back, the scratch
// of the device form from the plan and for the call, and { matched, missing } with a message() that reads the row only when it is called.
// unit: columns(fs, t) -> k, or throws; third(x): the word in the columns' place of a side's six; desc(k, m's three words, the sides' six
// words, sides) -> the description; plan(k, nF), host, dev: the addon's entries; format(missing, the row's values)
function multColumn(dev, tIn, fsIn, mIn, n, ew, unit) {
    const t = tIn ? side(tIn, "t", n, ew, dev) : null, fs = fsIn.map((f, s) => side(f, "f " + s, n, ew, dev)), k = unit.columns(fs, t);
    const m = side({ buf: mIn.buf, stride: mIn.stride, cols: [mIn.col] }, "m", n, ew, dev);
    const sides = (t ? [t] : []).concat(fs), ptr = (b) => dev && b ? b.ptr : 0n;
    const six = sides.map((x) => [ptr(x.buf), x.stride, unit.third(x)].concat(x.sel ? [ptr(x.sel.buf), x.sel.stride, x.sel.col] : [0n, 0, 0]));
    const desc = BigUint64Array.from(unit.desc(k, [ptr(m.buf), m.stride, mIn.col], six, sides).map((v) => BigInt(v)));
    const rep = new BigUint64Array(4);
    let read;
    if (!dev) {
        unit.host(desc, matrices(sides).concat([m.buf]), rep, ew);
        copyBack(m.buf, mIn.buf);
        read = (buf, at, len) => buf.subarray(at, at + len);
    } else {
        const plan = unit.plan(k, fs.length);
        const work = new DevBuffer(Math.max(2, plan.scratchBytes / 8));
        try { unit.dev(desc, work.ptr, plan.scratchBytes, rep, ew); } finally { work.free(); }
        read = (buf, at, len) => buf.slice(at, at + len);
    }
    const out = { matched: Number(rep[3]), missing: null };
    if (rep[0] !== 0n) {
        const x = out.missing = { side: Number(rep[1]), row: Number(rep[2]) };
        x.message = () => { const f = fs[x.side]; return unit.format(x, f.cols.map((c) => decimalOf(read(f.buf, (x.row * f.stride + c) * ew, ew)))); };
    }
    return out;
}
function multiplicities(dev, fsIn, tIn, mIn, n, opts) {
    const ew = opts && opts.bn128 ? 4 : 1;
    checkMultArgs(fsIn, mIn);
    return multColumn(dev, tIn || {}, fsIn, mIn, n, ew, {                        // {}: refused as a side, where null would say "no table side"
        columns: (fs, t) => { const k = t.cols.length; fs.forEach((f, s) => { if (f.cols.length !== k) throw new Error("t has " + k + " columns and f " + s + " " + f.cols.length); }); return k; },
        third: () => 0,
        desc: (k, m, six, sides) => [n, k, sides.length - 1].concat(m, ...six, ...sides.map((x) => x.cols)),
        plan: (k, nF) => addon.lookupMultPlan(n, k, nF, ew), host: addon.lookupMult, dev: addon.lookupMultDev, format: formatMissing,
    });
}
const lookupMultiplicities = (fs, t, m, n, opts) => multiplicities(false, fs, t, m, n, opts);
const lookupMultiplicitiesDev = (fs, t, m, n, opts) => multiplicities(true, fs, t, m, n, opts);
const lookupMultProbe = () => Number(addon.lookupMultProbe());

// ---- range-check multiplicities ----
// The wording, once (INTEGRATION.md):
//   "range: f side S row R = V is outside [LO, HI]"
const formatOutOfRange = (x, value, lo, size) => "range: f side " + x.side + " row " + x.row + " = " + value + " is outside [" + lo + ", " + (lo + BigInt(size) - 1n) + "]";
function rangeCounts(dev, fsIn, loIn, size, mIn, n, opts) {
    const ew = opts && opts.bn128 ? 4 : 1, row0 = opts && opts.row0 ? opts.row0 : 0;
    checkMultArgs(fsIn, mIn);
    const lo = BigInt(loIn);
    if (lo < -(1n << 63n) || lo >= 1n << 63n) throw new Error("lo must be a signed 64-bit integer");
    return multColumn(dev, null, fsIn, mIn, n, ew, {
        columns: (fs) => { fs.forEach((f, s) => { if (f.cols.length !== 1) throw new Error("f " + s + " must have one column"); }); return 1; },
        third: (x) => x.cols[0],
        desc: (k, m, six, sides) => [n, sides.length, BigInt.asUintN(64, lo), size, row0].concat(m, ...six),
        plan: (k, nF) => addon.rangeMultPlan(n, size, nF, ew), host: addon.rangeMult, dev: addon.rangeMultDev,
        format: (x, values) => formatOutOfRange(x, values[0], lo, size),
    });
}
const rangeMultiplicities = (fs, lo, size, m, n, opts) => rangeCounts(false, fs, lo, size, m, n, opts);
const rangeMultiplicitiesDev = (fs, lo, size, m, n, opts) => rangeCounts(true, fs, lo, size, m, n, opts);
const rangeMultPlan = (n, size, nF, bn128) => addon.rangeMultPlan(n, size, nF, bn128 ? 4 : 1);

// ---- multiplicity sessions: a table's m counted over the f sides of other AIRs, each of its own length (csrc/mult_session.hip) ----
//   const s = new RangeSession(lo, size, opts) | new LookupSession(t, nT, opts)     open; the session owns its scratch; t stays unchanged
//   s.add(fs, rows) -> { matched, missing: null | { side, row } } of THIS add, matched a BigInt; fs: DevBuffer sides as above, rows[i] the rows of side i
//   s.write(m, nM, row0) | s.write(m) -> the session's matched rows (a BigInt: counts pass 2^32); m: { buf: DevBuffer, stride, col }; may be called again
//   s.free()                                                                        the scratch
const sixOf = (x, third) => [x.buf.ptr, x.stride, third].concat(x.sel ? [x.sel.buf.ptr, x.sel.stride, x.sel.col] : [0n, 0, 0]);
const descWords = (list) => BigUint64Array.from(list.map((v) => BigInt(v)));
function addReport(rep) {
    return { matched: rep[3], missing: rep[0] === 0n ? null : { side: Number(rep[1]), row: Number(rep[2]) } };      // matched: a BigInt, as every 64-bit count of a session
}
function sessionSides(fsIn, rows, ew, k) {
    if (!Array.isArray(fsIn) || fsIn.length < 1 || fsIn.length > 8 || !Array.isArray(rows) || rows.length !== fsIn.length) throw new Error("fs must be an array of 1 .. 8 sides, rows their row counts");
    return fsIn.map((f, s) => {
        const x = side(f, "f " + s, rows[s], ew, true);
        if (x.cols.length !== k) throw new Error("f " + s + " must have " + k + " column(s)");
        return x;
    });
}
class LookupSession {
    constructor(tIn, nT, opts) {
        this.ew = opts && opts.bn128 ? 4 : 1;
        this.nT = nT;
        this.t = side(tIn, "t", nT, this.ew, true);
        this.k = this.t.cols.length;
        this.plan = addon.lookupSessionPlan(nT, this.k, this.ew);
        this.work = new DevBuffer(Math.max(2, this.plan.scratchBytes / 8));
        addon.lookupSessionOpenDev(this.desc([], [0n, 1, 0], []), this.work.ptr, this.plan.scratchBytes, this.ew);
    }
    desc(fs, m, rows) {
        const sides = [this.t].concat(fs);
        return descWords([this.nT, this.k, fs.length].concat(m, ...sides.map((x) => sixOf(x, 0)), ...sides.map((x) => x.cols), rows));
    }
    add(fsIn, rows) {
        const fs = sessionSides(fsIn, rows, this.ew, this.k), rep = new BigUint64Array(4);
        addon.lookupSessionAddDev(this.desc(fs, [0n, 1, 0], rows), this.work.ptr, this.plan.scratchBytes, rep, this.ew);
        return addReport(rep);
    }
    write(mIn) {
        const m = side({ buf: mIn.buf, stride: mIn.stride, cols: [mIn.col] }, "m", this.nT, this.ew, true);
        return addon.lookupSessionWriteDev(this.desc([], [m.buf.ptr, m.stride, mIn.col], []), this.work.ptr, this.plan.scratchBytes, this.ew);
    }
    free() { this.work.free(); }
}
class RangeSession {
    constructor(loIn, size, opts) {
        this.ew = opts && opts.bn128 ? 4 : 1;
        this.lo = BigInt(loIn);
        if (this.lo < -(1n << 63n) || this.lo >= 1n << 63n) throw new Error("lo must be a signed 64-bit integer");
        this.size = size;
        this.plan = addon.rangeSessionPlan(size, this.ew);
        this.work = new DevBuffer(Math.max(2, this.plan.scratchBytes / 8));
        addon.rangeSessionOpenDev(size, this.work.ptr, this.plan.scratchBytes);
    }
    desc(nM, fs, row0, m, rows) {
        return descWords([nM, fs.length, BigInt.asUintN(64, this.lo), this.size, row0].concat(m, ...fs.map((x) => sixOf(x, x.cols[0])), rows));
    }
    add(fsIn, rows) {
        const fs = sessionSides(fsIn, rows, this.ew, 1), rep = new BigUint64Array(4);
        addon.rangeSessionAddDev(this.desc(0, fs, 0, [0n, 1, 0], rows), this.work.ptr, this.plan.scratchBytes, rep, this.ew);
        return addReport(rep);
    }
    write(mIn, nM, row0) {
        const m = side({ buf: mIn.buf, stride: mIn.stride, cols: [mIn.col] }, "m", nM, this.ew, true);
        return addon.rangeSessionWriteDev(this.desc(nM, [], row0 || 0, [m.buf.ptr, m.stride, mIn.col], []), this.work.ptr, this.plan.scratchBytes, this.ew);
    }
    free() { this.work.free(); }
}
const lookupSessionPlan = (nT, k, bn128) => addon.lookupSessionPlan(nT, k, bn128 ? 4 : 1);
const rangeSessionPlan = (size, bn128) => addon.rangeSessionPlan(size, bn128 ? 4 : 1);

// ---- lookup grand sum ----
function logup(dev, termsIn, alpha, beta, outIn, n, opts) {
    const bn = !!(opts && opts.bn128), ew = bn ? 4 : 1, width = bn ? 1 : 3;
    if (!Array.isArray(termsIn) || termsIn.length < 1 || termsIn.length > 9) throw new Error("terms must be an array of 1 .. 9 terms");
    if (!outIn || !(outIn.stride > 0) || !(outIn.col >= 0)) throw new Error("out must be { buf, stride, col }");
    const elem = (v, what, words) => {
        if (!bn && words === 1) { if (typeof v !== "bigint") throw new Error(what + " must be a BigInt"); return [v, 0n, 0n, 0n]; }
        const w = Array.from(stage.asWords(v));
        if (w.length !== words) throw new Error(what + " must hold " + words + " words");
        return w.concat([0n, 0n, 0n, 0n]).slice(0, 4);
    };
    const terms = termsIn.map((t, u) => {
        const s = side(t, "term " + u, n, ew, dev);
        if (s.cols.length < 1 || s.cols.length > 16) throw new Error("term " + u + ": 1 .. 16 columns");
        s.coef = elem(t.coef, "coef of term " + u, ew); s.busId = elem(t.busId, "busId of term " + u, ew);
        return s;
    });
    const out = side({ buf: outIn.buf, stride: outIn.stride, cols: [outIn.col, outIn.col + width - 1] }, "out", n, ew, dev);
    const ptr = (b) => dev && b ? b.ptr : 0n;
    const head = [n, terms.length, ptr(out.buf), out.stride, outIn.col].concat(elem(alpha, "alpha", bn ? 4 : 3), elem(beta, "beta", bn ? 4 : 3));
    const fourteen = terms.map((x) => [ptr(x.buf), x.stride, x.cols.length].concat(x.sel ? [ptr(x.sel.buf), x.sel.stride, x.sel.col] : [0n, 0, 0], x.coef, x.busId));
    const slots = terms.map((x) => x.cols.concat(new Array(16 - x.cols.length).fill(0)));
    const desc = BigUint64Array.from(head.concat(...fourteen, ...slots).map((v) => BigInt(v)));
    if (dev) { addon.logupSumDev(desc, ew, opts && opts.stream); return outIn; }
    addon.logupSum(desc, matrices(terms).concat([out.buf]), ew);
    copyBack(out.buf, outIn.buf);
    return outIn;
}
const logupSum = (terms, alpha, beta, out, n, opts) => logup(false, terms, alpha, beta, out, n, opts);
const logupSumDev = (terms, alpha, beta, out, n, opts) => logup(true, terms, alpha, beta, out, n, opts);
const logupSumPlan = (n, nTerms, bn128) => addon.logupSumPlan(n, nTerms, bn128 ? 4 : 1);

// ---- range-check grand sum ----
function rangeLogup(dev, termsIn, rangesIn, alpha, beta, outIn, n, opts) {
    const bn = !!(opts && opts.bn128), ew = bn ? 4 : 1, width = bn ? 1 : 3;
    if (!Array.isArray(termsIn) || termsIn.length > 8) throw new Error("terms must be an array of 0 .. 8 terms");
    if (!Array.isArray(rangesIn) || rangesIn.length < 1 || rangesIn.length > 8 || termsIn.length + rangesIn.length > 9) throw new Error("ranges must be an array of 1 .. 8 ranges, 9 with the terms at most");
    if (!outIn || !(outIn.stride > 0) || !(outIn.col >= 0)) throw new Error("out must be { buf, stride, col }");
    const elem = (v, what, words) => {
        if (!bn && words === 1) { if (typeof v !== "bigint") throw new Error(what + " must be a BigInt"); return [v, 0n, 0n, 0n]; }
        const w = Array.from(stage.asWords(v));
        if (w.length !== words) throw new Error(what + " must hold " + words + " words");
        return w.concat([0n, 0n, 0n, 0n]).slice(0, 4);
    };
    const terms = termsIn.map((t, u) => {
        const s = side(t, "term " + u, n, ew, dev);
        if (s.cols.length < 1 || s.cols.length > 16) throw new Error("term " + u + ": 1 .. 16 columns");
        s.coef = elem(t.coef, "coef of term " + u, ew); s.busId = elem(t.busId, "busId of term " + u, ew);
        return s;
    });
    const ranges = rangesIn.map((r, i) => {
        if (!r || !r.m || !(r.m.stride > 0) || !(r.m.col >= 0)) throw new Error("range " + i + " must be { m: { buf, stride, col }, lo, size, row0, coef, busId }");
        const lo = BigInt(r.lo);
        if (lo < -(1n << 63n) || lo >= 1n << 63n) throw new Error("range " + i + ": lo must be a signed 64-bit integer");
        const s = side({ buf: r.m.buf, stride: r.m.stride, cols: [r.m.col] }, "m of range " + i, n, ew, dev);
        return Object.assign(s, { lo: BigInt.asUintN(64, lo), size: r.size, row0: r.row0 || 0, coef: elem(r.coef, "coef of range " + i, ew), busId: elem(r.busId, "busId of range " + i, ew) });
    });
    const out = side({ buf: outIn.buf, stride: outIn.stride, cols: [outIn.col, outIn.col + width - 1] }, "out", n, ew, dev);
    const ptr = (b) => dev && b ? b.ptr : 0n;
    const head = [n, terms.length, ranges.length, ptr(out.buf), out.stride, outIn.col].concat(elem(alpha, "alpha", bn ? 4 : 3), elem(beta, "beta", bn ? 4 : 3));
    const fourteen = terms.map((x) => [ptr(x.buf), x.stride, x.cols.length].concat(x.sel ? [ptr(x.sel.buf), x.sel.stride, x.sel.col] : [0n, 0, 0], x.coef, x.busId));
    const rangeWords = ranges.map((x) => [ptr(x.buf), x.stride, x.cols[0], x.lo, x.size, x.row0].concat(x.coef, x.busId));
    const slots = terms.map((x) => x.cols.concat(new Array(16 - x.cols.length).fill(0)));
    const desc = BigUint64Array.from(head.concat(...fourteen, ...rangeWords, ...slots).map((v) => BigInt(v)));
    if (dev) { addon.rangeSumDev(desc, ew, opts && opts.stream); return outIn; }
    addon.rangeSum(desc, matrices(terms.concat(ranges)).concat([out.buf]), ew);
    copyBack(out.buf, outIn.buf);
    return outIn;
}
const rangeSum = (terms, ranges, alpha, beta, out, n, opts) => rangeLogup(false, terms, ranges, alpha, beta, out, n, opts);
const rangeSumDev = (terms, ranges, alpha, beta, out, n, opts) => rangeLogup(true, terms, ranges, alpha, beta, out, n, opts);
const rangeSumPlan = (n, nF, nR, bn128) => addon.rangeSumPlan(n, nF, nR, bn128 ? 4 : 1);

// ---- clustered logUp sum: s and one im column a cluster ----
// terms and ranges as rangeSum's (either may be empty); cluster: an entry a term, f terms first, a cluster id or DIRECT; im: one
// { buf, stride, col } a cluster.  A host buffer given twice (s and its im columns in one matrix) is ONE matrix: converted once, written once.
const DIRECT = NONE;
function logupClustered(dev, termsIn, rangesIn, clusterIn, imIn, alpha, beta, outIn, n, opts) {
    const bn = !!(opts && opts.bn128), ew = bn ? 4 : 1, width = bn ? 1 : 3;
    if (!Array.isArray(termsIn) || termsIn.length > 8) throw new Error("terms must be an array of 0 .. 8 terms");
    if (!Array.isArray(rangesIn) || rangesIn.length > 8 || termsIn.length + rangesIn.length < 1 || termsIn.length + rangesIn.length > 9) throw new Error("ranges must be an array of 0 .. 8 ranges, 1 .. 9 with the terms");
    if (!Array.isArray(clusterIn) || clusterIn.length !== termsIn.length + rangesIn.length) throw new Error("cluster must hold an entry for every term and range");
    if (!Array.isArray(imIn) || imIn.length < 1 || imIn.length > 9) throw new Error("im must be an array of 1 .. 9 columns { buf, stride, col }");
    if (!outIn || !(outIn.stride > 0) || !(outIn.col >= 0)) throw new Error("out must be { buf, stride, col }");
    const held = new Map();                          // a host buffer -> its words, made once
    const own = (b) => { if (dev || !b) return b; if (!held.has(b)) held.set(b, stage.asWords(b)); return held.get(b); };
    const elem = (v, what, words) => {
        if (!bn && words === 1) { if (typeof v !== "bigint") throw new Error(what + " must be a BigInt"); return [v, 0n, 0n, 0n]; }
        const w = Array.from(stage.asWords(v));
        if (w.length !== words) throw new Error(what + " must hold " + words + " words");
        return w.concat([0n, 0n, 0n, 0n]).slice(0, 4);
    };
    const terms = termsIn.map((t, u) => {
        const s = side(Object.assign({}, t, { buf: own(t.buf), sel: t.sel ? Object.assign({}, t.sel, { buf: own(t.sel.buf) }) : t.sel }), "term " + u, n, ew, dev);
        if (s.cols.length < 1 || s.cols.length > 16) throw new Error("term " + u + ": 1 .. 16 columns");
        s.coef = elem(t.coef, "coef of term " + u, ew); s.busId = elem(t.busId, "busId of term " + u, ew);
        return s;
    });
    const ranges = rangesIn.map((r, i) => {
        if (!r || !r.m || !(r.m.stride > 0) || !(r.m.col >= 0)) throw new Error("range " + i + " must be { m: { buf, stride, col }, lo, size, row0, coef, busId }");
        const lo = BigInt(r.lo);
        if (lo < -(1n << 63n) || lo >= 1n << 63n) throw new Error("range " + i + ": lo must be a signed 64-bit integer");
        const s = side({ buf: own(r.m.buf), stride: r.m.stride, cols: [r.m.col] }, "m of range " + i, n, ew, dev);
        return Object.assign(s, { lo: BigInt.asUintN(64, lo), size: r.size, row0: r.row0 || 0, coef: elem(r.coef, "coef of range " + i, ew), busId: elem(r.busId, "busId of range " + i, ew) });
    });
    const column = (x, what) => {
        if (!x || !(x.stride > 0) || !(x.col >= 0)) throw new Error(what + " must be { buf, stride, col }");
        return Object.assign(side({ buf: own(x.buf), stride: x.stride, cols: [x.col, x.col + width - 1] }, what, n, ew, dev), { col: x.col });
    };
    const im = imIn.map((x, c) => column(x, "im " + c)), out = column(outIn, "out");
    const cluster = clusterIn.map((c) => BigInt.asUintN(64, BigInt(c)));
    const ptr = (b) => dev && b ? b.ptr : 0n;
    const head = [n, terms.length, ranges.length, im.length, ptr(out.buf), out.stride, out.col].concat(elem(alpha, "alpha", bn ? 4 : 3), elem(beta, "beta", bn ? 4 : 3));
    const fourteen = terms.map((x) => [ptr(x.buf), x.stride, x.cols.length].concat(x.sel ? [ptr(x.sel.buf), x.sel.stride, x.sel.col] : [0n, 0, 0], x.coef, x.busId));
    const rangeWords = ranges.map((x) => [ptr(x.buf), x.stride, x.cols[0], x.lo, x.size, x.row0].concat(x.coef, x.busId));
    const imWords = im.map((x) => [ptr(x.buf), x.stride, x.col]);
    const slots = terms.map((x) => x.cols.concat(new Array(16 - x.cols.length).fill(0)));
    const desc = BigUint64Array.from(head.concat(...fourteen, ...rangeWords, cluster, ...imWords, ...slots).map((v) => BigInt(v)));
    if (dev) { addon.logupClusterDev(desc, ew, opts && opts.stream); return outIn; }
    addon.logupCluster(desc, matrices(terms.concat(ranges, im)).concat([out.buf]), ew);
    const back = new Set();
    for (const x of imIn.concat([outIn])) if (!back.has(x.buf)) { back.add(x.buf); copyBack(held.get(x.buf), x.buf); }
    return outIn;
}
const logupCluster = (terms, ranges, cluster, im, alpha, beta, out, n, opts) => logupClustered(false, terms, ranges, cluster, im, alpha, beta, out, n, opts);
const logupClusterDev = (terms, ranges, cluster, im, alpha, beta, out, n, opts) => logupClustered(true, terms, ranges, cluster, im, alpha, beta, out, n, opts);
const logupClusterPlan = (n, nF, nR, nIm, bn128) => addon.logupClusterPlan(n, nF, nR, nIm, bn128 ? 4 : 1);

// ---- grand product of a permutation or a connection ----
// A term is a side { buf, stride, cols, sel } with den: 0 | 1 and optionally id: { buf, stride, col } and idCoef (3 words over Goldilocks,
// 4 Montgomery words over Fr); alpha, beta, gamma are 3 or 4 words each; out is logupSum's.  z[n-1] is the hint's result.
function grandProd(dev, termsIn, alpha, beta, gamma, outIn, n, opts) {
    const bn = !!(opts && opts.bn128), ew = bn ? 4 : 1, width = bn ? 1 : 3, cw = bn ? 4 : 3;
    if (!Array.isArray(termsIn) || termsIn.length < 1 || termsIn.length > 40) throw new Error("terms must be an array of 1 .. 40 terms");
    if (!outIn || !(outIn.stride > 0) || !(outIn.col >= 0)) throw new Error("out must be { buf, stride, col }");
    const elem = (v, what) => {
        const w = Array.from(stage.asWords(v));
        if (w.length !== cw) throw new Error(what + " must hold " + cw + " words");
        return w.concat([0n]).slice(0, 4);
    };
    const terms = termsIn.map((t, u) => {
        const s = side(t, "term " + u, n, ew, dev);
        if (s.cols.length < 1 || s.cols.length > 16) throw new Error("term " + u + ": 1 .. 16 columns");
        s.den = t.den ? 1 : 0;
        s.id = t.id ? side({ buf: t.id.buf, stride: t.id.stride, cols: [t.id.col] }, "the id of term " + u, n, ew, dev) : null;
        s.idCoef = t.id ? elem(t.idCoef, "idCoef of term " + u) : [0n, 0n, 0n, 0n];
        return s;
    });
    const out = side({ buf: outIn.buf, stride: outIn.stride, cols: [outIn.col, outIn.col + width - 1] }, "out", n, ew, dev);
    const ptr = (b) => dev && b ? b.ptr : 0n;
    const head = [n, terms.length, ptr(out.buf), out.stride, outIn.col].concat(elem(alpha, "alpha"), elem(beta, "beta"), elem(gamma, "gamma"));
    const fourteen = terms.map((x) => [ptr(x.buf), x.stride, x.cols.length].concat(x.sel ? [ptr(x.sel.buf), x.sel.stride, x.sel.col] : [0n, 0, 0], [x.den],
        x.id ? [ptr(x.id.buf), x.id.stride, x.id.cols[0]] : [0n, 0, 0], x.idCoef));
    const slots = terms.map((x) => x.cols.concat(new Array(16 - x.cols.length).fill(0)));
    const desc = BigUint64Array.from(head.concat(...fourteen, ...slots).map((v) => BigInt(v)));
    if (dev) { addon.grandProdDev(desc, ew, opts && opts.stream); return outIn; }
    const four = [].concat(...terms.map((x) => [x.buf, x.sel ? x.sel.buf : null, x.buf, x.id ? x.id.buf : null]));
    addon.grandProd(desc, four.concat([out.buf]), ew);
    copyBack(out.buf, outIn.buf);
    return outIn;
}
const grandProduct = (terms, alpha, beta, gamma, out, n, opts) => grandProd(false, terms, alpha, beta, gamma, out, n, opts);
const grandProductDev = (terms, alpha, beta, gamma, out, n, opts) => grandProd(true, terms, alpha, beta, gamma, out, n, opts);
const grandProductPlan = (n, nTerms, sumK, bn128) => addon.grandProdPlan(n, nTerms, sumK, bn128 ? 4 : 1);
// the term lists of the reference's two identities (grandProductPermutation.js, grandProductConnection.js); deltaKs[j] = delta ks'_j, made
// by the caller with its field (ks' = 1, ks[0], ks[1], ..)
const permutationTerms = (f, t) => [Object.assign({}, f, { den: 0 }), Object.assign({}, t, { den: 1 })];
const connectionTerms = (aCols, sCols, x, delta, deltaKs) => [].concat(...aCols.map((a, j) => [
    { buf: a.buf, stride: a.stride, cols: [a.col], den: 0, id: x, idCoef: deltaKs[j] },
    { buf: a.buf, stride: a.stride, cols: [a.col], den: 1, id: sCols[j], idCoef: delta }]));

// ---- plookup of pil1: the fold of F and T, and z from f, t, h1 and h2 ----
// f and t are sides { buf, stride, cols, sel } with their own column counts; h1, h2 and the outputs are columns { buf, stride, col } of hDim
// words an element (Goldilocks: opts.hDim, 3 by default; Fr: one element); the challenges are 3 or 4 words each.  z[n-1] is the hint's result.
function plookup(dev, prod, fIn, tIn, colsIn, chs, n, opts) {
    const bn = !!(opts && opts.bn128), ew = bn ? 4 : 1, cw = bn ? 4 : 3;
    const hDim = bn ? 1 : (opts && opts.hDim !== undefined ? opts.hDim : 3), hw = bn ? 1 : hDim, zw = bn ? 1 : 3;
    if (hDim !== 1 && hDim !== 3) throw new Error("hDim is 1 or 3");
    const elem = (v, what) => {
        const w = Array.from(stage.asWords(v));
        if (w.length !== cw) throw new Error(what + " must hold " + cw + " words");
        return w.concat([0n]).slice(0, 4);
    };
    const names = prod ? ["h1", "h2", "out"] : ["outF", "outT"], chNames = ["alpha", "beta", "gamma", "delta"];
    const f = side(fIn, "f", n, ew, dev), t = side(tIn, "t", n, ew, dev);
    for (const [x, what] of [[f, "f"], [t, "t"]]) if (x.cols.length < 1 || x.cols.length > 16) throw new Error(what + ": 1 .. 16 columns");
    const cols = colsIn.map((c, i) => {
        if (!c || !(c.stride > 0) || !(c.col >= 0)) throw new Error(names[i] + " must be { buf, stride, col }");
        return side({ buf: c.buf, stride: c.stride, cols: [c.col, c.col + (prod && i === 2 ? zw : hw) - 1] }, names[i], n, ew, dev);
    });
    if (!prod && colsIn[0].buf === colsIn[1].buf) cols[1].buf = cols[0].buf;      // one matrix for both outputs: one copy where asWords copied
    const ptr = (b) => dev && b ? b.ptr : 0n;
    const five = (x) => [ptr(x.buf), x.stride].concat(x.sel ? [ptr(x.sel.buf), x.sel.stride, x.sel.col] : [0n, 0, 0]);
    const four = [0, 1, 2, 3].map((i) => i < chs.length ? elem(chs[i], chNames[i]) : [0n, 0n, 0n, 0n]);
    const three = [0, 1, 2].map((i) => i < cols.length ? [ptr(cols[i].buf), cols[i].stride, colsIn[i].col] : [0n, 0, 0]);
    const slots = (x) => x.cols.concat(new Array(16 - x.cols.length).fill(0));
    const desc = BigUint64Array.from([n, f.cols.length, t.cols.length, hDim].concat(...four, five(f), five(t), ...three, slots(f), slots(t)).map((v) => BigInt(v)));
    const written = prod ? [colsIn[2]] : colsIn;
    if (dev) { (prod ? addon.plookupProdDev : addon.plookupFoldDev)(desc, ew, opts && opts.stream); return prod ? written[0] : written; }
    const mats = matrices([f, t]).concat(prod ? [cols[0].buf, null, cols[1].buf, null, cols[2].buf] : [cols[0].buf, null, cols[1].buf]);
    (prod ? addon.plookupProd : addon.plookupFold)(desc, mats, ew);
    (prod ? [cols[2]] : cols).forEach((c, i) => copyBack(c.buf, written[i].buf));
    return prod ? written[0] : written;
}
const plookupFold = (f, t, alpha, beta, outF, outT, n, opts) => plookup(false, false, f, t, [outF, outT], [alpha, beta], n, opts);
const plookupFoldDev = (f, t, alpha, beta, outF, outT, n, opts) => plookup(true, false, f, t, [outF, outT], [alpha, beta], n, opts);
const plookupProduct = (f, t, h1, h2, alpha, beta, gamma, delta, out, n, opts) => plookup(false, true, f, t, [h1, h2, out], [alpha, beta, gamma, delta], n, opts);
const plookupProductDev = (f, t, h1, h2, alpha, beta, gamma, delta, out, n, opts) => plookup(true, true, f, t, [h1, h2, out], [alpha, beta, gamma, delta], n, opts);
const plookupPlan = (n, kF, kT, bn128) => addon.plookupPlan(n, kF, kT, bn128 ? 4 : 1);

module.exports = { lookupMultiplicities, lookupMultiplicitiesDev, formatMissing, lookupMultProbe, rangeMultiplicities, rangeMultiplicitiesDev, rangeMultPlan, formatOutOfRange, LookupSession, RangeSession, lookupSessionPlan, rangeSessionPlan, logupSum, logupSumDev, logupSumPlan, rangeSum, rangeSumDev, rangeSumPlan, logupCluster, logupClusterDev, logupClusterPlan, DIRECT, grandProduct, grandProductDev, grandProductPlan, permutationTerms, connectionTerms, plookupFold, plookupFoldDev, plookupProduct, plookupProductDev, plookupPlan, checkLookup, checkPermutation, checkLookupDev, checkPermutationDev, formatReport, tupleHome, tupleCheckProbe, LOOKUP, PERMUTATION };
