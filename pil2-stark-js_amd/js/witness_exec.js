// The recursion witness on the device: the `*_exec` step of the reference with the witness in place of the wasm (the witness calculator
// is third-party and stays the caller's).  Names and shapes follow src/compressor/compressor_exec.js and src/final/exec_helpers.js /
// main_final_exec.js:50-67; the additions and the sMap gather run in csrc/wtns_exec.hip.
//   readExecFile(execFile, nCols)            compressor .exec (flat u64)  -> { nAdds, nSMap, addsBuff, sMapBuff }
//   readExecFile(Fr, execFile, nCols)        final .exec (binfile "exec") -> { nAdds, nSMap, addsBigInt, addsFr, sMap }; addsFr = the 2 nAdds
//                                            coefficients as section 4 holds them, Montgomery bytes (the reference turns them into BigInts)
//   readWtns(file)                           .wtns (binfile "wtns")       -> { n8, prime, nWitness, w: Uint8Array, normal form }
//   compressorExec(F, pil, w, exec)          w: BigUint64Array | BigInt[] -> cmPols-shaped { Compressor: { a: [nCols][N] BigInt }, trace }
//   finalExec(w, exec, nCols, opts)          w: Uint8Array of 32-byte normal-form values -> the N x nCols trace as bytes, Montgomery form
//                                            unless opts.montgomery === false (what writeToBigBufferFr leaves in cm1_n)
//   prepareExec(exec, nCols, nWitness)       once per setup -> { adds, coefs, sMap, levelStart, ... } with the tables as DevBuffers
//   execDev(prepared, wDev, dst, opts)       per proof: wDev = DevBuffer of nW elements whose first nWitness hold the witness; dst = DevBuffer
//                                            of nRows x (opts.dstCols || nCols) elements, made when absent; opts.check: throw on a bad index
//   connectionPols(F, sMap, N, ks, { w })    the setups' two S loops (compressor12_setup.js:470-500 and siblings; csrc/conn_pols.hip): sMap = the
//                                            setups' own array of nCols Uint32Array(N), ks = getKs(F, nCols - 1), w = F.w[log2 N] unless given
//                                            -> S[j][i]: BigInts over Goldilocks, 32-byte Montgomery Uint8Arrays over curve.Fr, so that a
//                                            setup says constPols.Compressor.S = connectionPols(F, sMap, N, ks)
//   connectionPolsDev(prepared, dConst, { N, ks, w, stride, offset, check })   the same from prepareExec's resident sMap into columns
//                                            [offset, offset + nCols) of dConst, a DevBuffer of N rows of `stride` elements (made when
//                                            absent, stride = nCols); nothing is copied to the host; check: throw on a bad index
//   checkConnections(F, a, S, N, ks, { w })  does the trace meet `{a} connect {S}`, the connection half of pilcom's verifyPil
//                                            (main_compressor_pil_verify.js:36; csrc/conn_check.hip): a, S = [nCols][N] arrays (BigInts, 32-byte
//                                            Montgomery Uint8Arrays) or the flat N x nCols matrices -> null when clean, else
//                                            { row, col, toRow, toCol, kind, message() } of the first failing cell
//   checkConnectionsDev(aCol, SCol, { N, ks, w })   the same on resident columns { buf, stride, offset }: where execDev wrote the trace
//                                            and connectionPolsDev the constants; message() reads two elements back
// Node 12: no optional chaining.
"use strict";
const fs = require("fs");
const { addon, DevBuffer, isDev } = require("./native.js");
const stage = require("./bn128_stage.js");

function short(file, found, expected) { return new Error(file + ": " + found + " bytes found, " + expected + " expected"); }
function readAt(fd, file, size, at, n) {
    if (at + n > size) throw short(file, size, at + n);
    const b = new Uint8Array(n);
    let got = 0;
    while (got < n) { const k = fs.readSync(fd, b, got, n - got, at + got); if (k <= 0) throw short(file, at + got, at + n); got += k; }
    return b;
}
const u32 = (b, o) => new DataView(b.buffer, b.byteOffset, b.byteLength).getUint32(o, true);
const u64n = (b, o) => Number(new DataView(b.buffer, b.byteOffset, b.byteLength).getBigUint64(o, true));

// the minimal iden3 binfile reader: 4-byte type, u32 version, u32 section count, then (u32 id, u64 size, payload) until the file ends
function withSections(file, type, fn) {
    const fd = fs.openSync(file, "r");
    try {
        const size = fs.fstatSync(fd).size;
        const head = readAt(fd, file, size, 0, 12);
        if (Buffer.from(head.subarray(0, 4)).toString("latin1") !== type) throw new Error(file + ": not a " + type + " file");
        const version = u32(head, 4), count = u32(head, 8), secs = {};
        for (let at = 12, k = 0; at < size && k < count; k++) {
            const h = readAt(fd, file, size, at, 12), n = u64n(h, 4);
            if (at + 12 + n > size) throw short(file, size, at + 12 + n);
            secs[u32(h, 0)] = { at: at + 12, n };
            at += 12 + n;
        }
        const section = (id, bytes) => {
            if (!secs[id]) throw new Error(file + ": no section " + id);
            if (secs[id].n < bytes) throw short(file, size, size + bytes - secs[id].n);
            return readAt(fd, file, size, secs[id].at, bytes);
        };
        return fn(version, section);
    } finally { fs.closeSync(fd); }
}

function readCompressorExec(file, nCols) {
    const fd = fs.openSync(file, "r");
    try {
        const size = fs.fstatSync(fd).size;
        const h = readAt(fd, file, size, 0, 16), nAdds = u64n(h, 0), nSMap = u64n(h, 8);
        const want = 8 * (2 + 4 * nAdds + nSMap * nCols);
        if (size < want) throw short(file, size, want);
        const addsBuff = stage.asWords(readAt(fd, file, size, 16, 32 * nAdds));
        const sMapBuff = stage.asWords(readAt(fd, file, size, 16 + 32 * nAdds, 8 * nSMap * nCols));
        return { nAdds, nSMap, addsBuff, sMapBuff };
    } finally { fs.closeSync(fd); }
}
function readFinalExec(file, nCols) {
    return withSections(file, "exec", (version, section) => {
        if (version !== 1) throw new Error(file + ": exec version " + version + ", 1 expected");
        const info = section(2, 16), nAdds = u64n(info, 0), nSMap = u64n(info, 8);
        return { nAdds, nSMap, addsBigInt: stage.asWords(section(3, 16 * nAdds)), addsFr: section(4, 64 * nAdds), sMap: stage.asWords(section(5, 8 * nSMap * nCols)) };
    });
}
// both of the reference's shapes: (execFile, nCols) and (F, execFile, nCols[, logger])
async function readExecFile(a, b, c) {
    return typeof a === "string" ? readCompressorExec(a, b) : readFinalExec(b, c);
}
function readWtns(file) {
    return withSections(file, "wtns", (version, section) => {
        const n8 = u32(section(1, 4), 0), head = section(1, 8 + n8), nWitness = u32(head, 4 + n8);
        let prime = 0n;
        for (let i = n8 - 1; i >= 0; i--) prime = (prime << 8n) | BigInt(head[4 + i]);
        return { n8, prime, nWitness, w: section(2, nWitness * n8) };
    });
}

const isFinal = (exec) => exec.addsFr !== undefined;
function words(x) { return x instanceof BigUint64Array ? x : x instanceof Uint8Array ? stage.asWords(x) : BigUint64Array.from(Array.from(x, (v) => BigInt(v))); }

async function compressorExec(F, pil, w, exec) {
    const refs = pil.references, N = Object.values(refs)[0].polDeg;
    const a = refs["Compressor.a"], nCols = a && a.len ? a.len : exec.sMapBuff.length / exec.nSMap;
    const wW = words(w), trace = new BigUint64Array(exec.nSMap * nCols);
    addon.wtnsExec(wW, wW.length, exec.addsBuff, exec.nAdds, exec.sMapBuff, exec.nSMap, nCols, trace);
    const cols = [];
    for (let j = 0; j < nCols; j++) { const col = new Array(N).fill(0n); for (let i = 0; i < exec.nSMap; i++) col[i] = trace[i * nCols + j]; cols.push(col); }
    return { Compressor: { a: cols }, trace };
}
function finalExec(w, exec, nCols, opts) {
    const wW = words(w), out = new Uint8Array(32 * exec.nSMap * nCols);
    addon.bn128WtnsExec(wW, wW.length / 4, exec.addsBigInt, words(exec.addsFr), exec.nAdds, exec.sMap, exec.nSMap, nCols, stage.asWords(out),
        !(opts && opts.montgomery === false));
    return out;
}

function prepareExec(exec, nCols, nWitness) {
    const bn128 = isFinal(exec), nAdds = exec.nAdds, nRows = exec.nSMap, nW = nWitness + nAdds;
    const idx = bn128 ? exec.addsBigInt : exec.addsBuff, coef = bn128 ? words(exec.addsFr) : exec.addsBuff;
    const plan = bn128 ? addon.wtnsAddsPlan(idx, 0, 2, nAdds, nWitness, coef, 0, 8, 4) : addon.wtnsAddsPlan(idx, 0, 4, nAdds, nWitness, coef, 2, 4, 1);
    const sMap64 = bn128 ? exec.sMap : exec.sMapBuff, cells = nRows * nCols;
    if (sMap64.length < cells) throw new Error("sMap holds " + sMap64.length + " entries, " + nRows + " x " + nCols + " expected");
    // narrow and validate over the 32-bit halves of the file's words (little-endian: low half first): no BigInt per cell
    const packed = new BigUint64Array(Math.ceil(cells / 2)), sMap32 = new Uint32Array(packed.buffer);
    const halves = new Uint32Array(sMap64.buffer, sMap64.byteOffset, 2 * cells);
    for (let k = 0; k < cells; k++) {
        const lo = halves[2 * k];
        if (halves[2 * k + 1] !== 0 || lo >= nW) throw new Error("sMap[" + k + "] = " + sMap64[k] + " names no signal (nWitness + nAdds = " + nW + ")");
        sMap32[k] = lo;
    }
    return { bn128, nWitness, nAdds, nW, nRows, nCols, nLevels: plan.nLevels, levelStart: plan.levelStart,
        adds: DevBuffer.from(plan.adds), coefs: DevBuffer.from(plan.coefs), sMap: DevBuffer.from(packed),
        free() { this.adds.free(); this.coefs.free(); this.sMap.free(); } };
}
function execDev(p, wDev, dst, opts) {
    opts = opts || {};
    const wordsPer = p.bn128 ? 4 : 1, dstCols = opts.dstCols || p.nCols;
    if (!isDev(wDev) || wDev.length < p.nW * wordsPer) throw new Error("execDev: w must be a DevBuffer of nW = " + p.nW + " elements");
    if (!dst) dst = new DevBuffer(p.nRows * dstCols * wordsPer);
    if (dst.length < p.nRows * dstCols * wordsPer) throw new Error("execDev: dst holds " + dst.length + " words");
    addon.wtnsAddsDev(wDev.ptr, p.nWitness, p.adds.ptr, p.coefs.ptr, p.nAdds, p.levelStart, p.nLevels, p.bn128);
    const bad = addon.wtnsGatherDev(wDev.ptr, p.nW, p.sMap.ptr, p.nRows, p.nCols, dst.ptr, dstCols, p.bn128, opts.montgomery !== false, !!opts.check);
    if (opts.check && bad !== 0xFFFFFFFFFFFFFFFFn) throw new Error("sMap cell " + bad + " names no signal");
    return dst;
}

// ---- connection polynomials ----
const FR_ONE = (() => {       // 2^256 mod r: one in Montgomery form, as bytes
    const v = (1n << 256n) % 21888242871839275222246405745257275088548364400416034343698204186575808495617n, b = new Uint8Array(32);
    for (let i = 0; i < 32; i++) b[i] = Number((v >> BigInt(8 * i)) & 0xFFn);
    return b;
})();
// w, then ks1 = one and the caller's nCols - 1 elements, as the library reads them
function connConsts(bn128, nCols, w, one, ks) {
    if (!ks || ks.length !== Math.max(nCols - 1, 0)) throw new Error("connectionPols: ks must hold nCols - 1 = " + (nCols - 1) + " elements");
    if (w === undefined) throw new Error("connectionPols: no root of unity w");
    const ew = bn128 ? 4 : 1, c = new BigUint64Array(ew * (1 + nCols));
    [w, one].concat(Array.from(ks)).slice(0, 1 + nCols).forEach((v, k) => { if (bn128) c.set(stage.asWords(v), 4 * k); else c[k] = BigInt(v); });
    return c;
}
function connectionPols(F, sMap, N, ks, opts) {
    const bn128 = F.n8 === 32, ew = bn128 ? 4 : 1, nCols = sMap.length;
    const consts = connConsts(bn128, nCols, opts && opts.w !== undefined ? opts.w : F.w[Math.log2(N)], F.one, ks);
    const packed = new BigUint64Array(Math.ceil(nCols * N / 2)), flat = new Uint32Array(packed.buffer);
    let top = 0;
    for (let j = 0; j < nCols; j++) {
        if (sMap[j].length !== N) throw new Error("connectionPols: sMap[" + j + "] holds " + sMap[j].length + " entries, N = " + N + " expected");
        flat.set(sMap[j], j * N);
        for (let i = 0; i < N; i++) if (sMap[j][i] > top) top = sMap[j][i];
    }
    const out = new BigUint64Array(ew * N * nCols);
    (bn128 ? addon.bn128ConnPols : addon.connPols)(packed, 1, N, nCols, top + 1, N, consts, out);
    const bytes = new Uint8Array(out.buffer), S = [];
    for (let j = 0; j < nCols; j++) {
        const col = new Array(N);
        for (let i = 0; i < N; i++) col[i] = bn128 ? bytes.subarray(32 * (i * nCols + j), 32 * (i * nCols + j + 1)) : out[i * nCols + j];
        S.push(col);
    }
    return S;
}
function connectionPolsDev(p, dConst, opts) {
    opts = opts || {};
    const ew = p.bn128 ? 4 : 1, N = opts.N, offset = opts.offset || 0, stride = opts.stride || p.nCols + offset;
    const consts = connConsts(p.bn128, p.nCols, opts.w, p.bn128 ? FR_ONE : 1n, opts.ks);
    const plan = addon.connPlan(p.nRows, p.nCols, p.nW, N, ew);
    if (!dConst) dConst = new DevBuffer(N * stride * ew);
    if (!isDev(dConst) || dConst.length < ((N - 1) * stride + offset + p.nCols) * ew) throw new Error("connectionPolsDev: dConst must be a DevBuffer of N = " + N + " rows of " + stride + " elements");
    const work = new DevBuffer(plan.scratchBytes / 8);
    try {
        const bad = (p.bn128 ? addon.bn128ConnPolsDev : addon.connPolsDev)(p.sMap.ptr, p.nRows, p.nCols, p.nW, N, consts, dConst.ptr, stride, offset, work.ptr,
            plan.scratchBytes, !!opts.check);
        if (opts.check && bad !== 0xFFFFFFFFFFFFFFFFn) throw new Error("sMap cell " + bad + " names no signal");
    } finally { work.free(); }                       // releasing device memory waits for the work enqueued on it
    return dConst;
}

// ---- connection check ----
const GL_P = 0xFFFFFFFF00000001n;
const FR = 21888242871839275222246405745257275088548364400416034343698204186575808495617n;
const FR_R_INV = 9915499612839321149637521777990102151350674507940716049588462388200839649614n;       // (2^256)^-1 mod r
const NONE = 0xFFFFFFFFFFFFFFFFn;
// an element's words as the decimal the reference's F.toString prints: the value mod p, the normal form of Montgomery words
function decimalOf(wordsOfElem) {
    if (wordsOfElem.length === 1) return (wordsOfElem[0] % GL_P).toString();
    let v = 0n;
    for (let k = 3; k >= 0; k--) v = (v << 64n) | wordsOfElem[k];
    return (v % FR * FR_R_INV % FR).toString();
}
// the library's three words and a reader of element (cell) of a or S -> null when clean, else the failing cell with a message().
// The wording, once (INTEGRATION.md): kind 2 "connect: a[col][row] = X differs from a[toCol][toRow] = Y, the cell S[col][row] names";
// kind 1 "connect: S[col][row] = X names no cell (a[col][row] = Y)"; kind 3 "connect: the identities of row, column and toRow, toCol are
// equal (w or ks is wrong)".  Two elements are read, and only when message() is called.
function connReport(rep, nCols, read) {
    const kind = Number(rep[2]);
    if (!kind) return null;
    const cell = Number(rep[0]), named = rep[1] !== NONE, to = named ? Number(rep[1]) : null;
    const r = { row: Math.floor(cell / nCols), col: cell % nCols, toRow: named ? Math.floor(to / nCols) : null, toCol: named ? to % nCols : null, kind };
    const at = "[" + r.col + "][" + r.row + "]";
    r.message = () => {
        if (kind === 3) return "connect: the identities of row " + r.row + ", column " + r.col + " and row " + r.toRow + ", column " + r.toCol + " are equal (w or ks is wrong)";
        if (kind === 1) return "connect: S" + at + " = " + decimalOf(read("S", cell)) + " names no cell (a" + at + " = " + decimalOf(read("a", cell)) + ")";
        return "connect: a" + at + " = " + decimalOf(read("a", cell)) + " differs from a[" + r.toCol + "][" + r.toRow + "] = " + decimalOf(read("a", to)) + ", the cell S" + at + " names";
    };
    return r;
}
// a or S of the host form as N x nCols row-major words: the cmPols shape [nCols][N] (BigInts, 32-byte Uint8Arrays) or the flat matrix itself
function connMatrix(x, N, nCols, ew, what) {
    if (x instanceof BigUint64Array || x instanceof Uint8Array) {
        const m = words(x);
        if (m.length !== N * nCols * ew) throw new Error("checkConnections: " + what + " holds " + m.length + " words, " + N + " x " + nCols + " elements expected");
        return m;
    }
    if (!Array.isArray(x) || x.length !== nCols) throw new Error("checkConnections: " + what + " must hold nCols = " + nCols + " columns");
    const m = new BigUint64Array(N * nCols * ew), bytes = new Uint8Array(m.buffer);
    for (let j = 0; j < nCols; j++) {
        if (x[j].length !== N) throw new Error("checkConnections: " + what + "[" + j + "] holds " + x[j].length + " entries, N = " + N + " expected");
        for (let i = 0; i < N; i++) { if (ew === 4) bytes.set(x[j][i], 32 * (i * nCols + j)); else m[i * nCols + j] = BigInt(x[j][i]); }
    }
    return m;
}
function checkConnections(F, a, S, N, ks, opts) {
    const bn128 = F.n8 === 32, ew = bn128 ? 4 : 1, nCols = ks.length + 1;
    const consts = connConsts(bn128, nCols, opts && opts.w !== undefined ? opts.w : F.w[Math.log2(N)], F.one, ks);
    const ma = connMatrix(a, N, nCols, ew, "a"), mS = connMatrix(S, N, nCols, ew, "S"), rep = new BigUint64Array(3);
    (bn128 ? addon.bn128ConnCheck : addon.connCheck)(ma, mS, N, nCols, consts, rep);
    return connReport(rep, nCols, (which, cell) => (which === "a" ? ma : mS).subarray(cell * ew, (cell + 1) * ew));
}
// aCol, SCol: { buf: DevBuffer, stride, offset }, nCols adjacent columns from `offset` on of a matrix of N rows of `stride` elements (the
// columns polutils_bn128.js takes, stride defaulting to offset + nCols here); the field is Fr when w is a Uint8Array, or as opts.bn128 says
function checkConnectionsDev(aCol, SCol, opts) {
    const bn128 = opts.bn128 !== undefined ? !!opts.bn128 : opts.w instanceof Uint8Array, ew = bn128 ? 4 : 1, N = opts.N, nCols = opts.ks.length + 1;
    const col = (c, what) => {
        if (!c || !isDev(c.buf)) throw new Error("checkConnectionsDev: " + what + " must be { buf: DevBuffer, stride, offset }");
        const offset = c.offset || 0, stride = c.stride === undefined ? offset + nCols : c.stride;
        if (c.buf.length < ((N - 1) * stride + offset + nCols) * ew) throw new Error("checkConnectionsDev: " + what + " holds " + c.buf.length + " words, N = " + N + " rows of " + stride + " elements need more");
        return { buf: c.buf, stride, offset };
    };
    const A = col(aCol, "a"), Sc = col(SCol, "S");
    const consts = connConsts(bn128, nCols, opts.w, bn128 ? FR_ONE : 1n, opts.ks);
    const plan = addon.connCheckPlan(N, nCols, ew), rep = new BigUint64Array(3);
    const work = new DevBuffer(plan.scratchBytes / 8);
    try {
        (bn128 ? addon.bn128ConnCheckDev : addon.connCheckDev)(A.buf.ptr, A.stride, A.offset, Sc.buf.ptr, Sc.stride, Sc.offset, N, nCols, consts, work.ptr, plan.scratchBytes, rep);
    } finally { work.free(); }
    return connReport(rep, nCols, (which, cell) => {
        const c = which === "a" ? A : Sc, at = (Math.floor(cell / nCols) * c.stride + c.offset + cell % nCols) * ew;
        return c.buf.slice(at, at + ew);
    });
}

module.exports = { readExecFile, readWtns, compressorExec, finalExec, prepareExec, execDev, connectionPols, connectionPolsDev, checkConnections, checkConnectionsDev };
