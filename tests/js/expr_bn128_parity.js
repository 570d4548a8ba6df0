// calculateExps over Fr (pil2-stark-js_amd/js/prover_helpers_bn128.js) on DevBuffer sections against BigInt arithmetic computed here:
// an intermediate polynomial on domain "n", a quotient-like expression on domain "ext" with ret, and the debug path's first failing row.
// usage: node expr_bn128_parity.js; exits non-zero on the first difference.
"use strict";
const path = require("path");
const m = require(path.join(__dirname, "..", "..", "pil2-stark-js_amd", "js", "index.js"));
const { calculateExps, callCalculateExps } = m.prover_helpers_bn128;

const R = 21888242871839275222246405745257275088548364400416034343698204186575808495617n;
const MONT = (1n << 256n) % R;
const mod = (v) => ((v % R) + R) % R;
function inv(a) { let [r0, r1, s0, s1] = [R, mod(a), 0n, 1n]; while (r1) { const q = r0 / r1; [r0, r1] = [r1, r0 - q * r1]; [s0, s1] = [s1, s0 - q * s1]; } return mod(s0); }
const MONT_INV = inv(MONT);
const fmul = (a, b) => a * b * MONT_INV % R;                 // F.mul on the integers F keeps in memory
const toBytes = (v) => { const u = new Uint8Array(32); for (let k = 0; k < 32; k++) u[k] = Number((v >> BigInt(8 * k)) & 0xFFn); return u; };
const fromBytes = (u) => { let v = 0n; for (let k = 31; k >= 0; k--) v = (v << 8n) | BigInt(u[k]); return v; };
const F = { e: (v) => toBytes(mod(BigInt(v)) * MONT % R), toString: (u) => (fromBytes(u) * MONT_INV % R).toString(10) };

let seed = 12345n;
const rnd = () => { let v = 0n; for (let k = 0; k < 5; k++) { seed = (seed * 6364136223846793005n + 1442695040888963407n) & 0xFFFFFFFFFFFFFFFFn; v = (v << 64n) | seed; } return v % R; };
const matrix = (rows, width) => Array.from({ length: rows }, () => Array.from({ length: width }, rnd));
function toDev(rows) {
    const flat = new BigUint64Array(rows.length * rows[0].length * 4);
    let o = 0;
    for (const row of rows) for (const v of row) for (let k = 0; k < 4; k++) flat[o++] = (v >> BigInt(64 * k)) & 0xFFFFFFFFFFFFFFFFn;
    return m.DevBuffer.from(flat);
}
function fromDev(buf, rows, width) {
    const flat = buf.toHost(), out = [];
    for (let r = 0; r < rows; r++) { const row = []; for (let c = 0; c < width; c++) { let v = 0n; for (let k = 3; k >= 0; k--) v = (v << 64n) | flat[(r * width + c) * 4 + k]; row.push(v); } out.push(row); }
    return out;
}
function same(what, got, want) {
    for (let r = 0; r < want.length; r++) for (let c = 0; c < want[r].length; c++)
        if (got[r][c] !== want[r][c]) throw new Error(what + ": row " + r + " column " + c + " differs");
}

async function main() {
    const nBits = 4, nBitsExt = 6, N = 16, extN = 64, extendBits = 2;
    const T = (id) => ({ type: "tmp", id, dim: 1 });
    const h = { const_n: matrix(N, 2), cm1_n: matrix(N, 2), cm2_n: matrix(N, 1), const_ext: matrix(extN, 2), cm1_ext: matrix(extN, 2), x_ext: matrix(extN, 1),
                Zi_ext: matrix(2 * extN, 1), q_ext: matrix(extN, 1) };
    const pub = rnd(), chal = rnd();
    const ctx = {
        F, nBits, nBitsExt, extendBits, N, extN, prover: "fflonk",
        pilInfo: { nConstants: 2, mapSectionsN: { cm1: 2, cm2: 1 }, cmPolsMap: [{ stage: 1, stagePos: 0, dim: 1 }, { stage: 1, stagePos: 1, dim: 1 }, { stage: 2, stagePos: 0, dim: 1 }],
                   boundaries: [{ name: "everyRow" }, { name: "lastRow" }] },
        publics: [toBytes(pub)], challenges: [[], [toBytes(chal)]], subproofValues: [],
    };
    for (const k of Object.keys(h)) ctx[k] = toDev(h[k]);

    // ---- domain n: an intermediate polynomial, cm2 = cm1_0 * cm1_1' + const_1[-1] - challenge * public + (-3)
    const imPol = { tmpUsed: 4, code: [
        { op: "mul", dest: T(0), src: [{ type: "cm", id: 0, prime: 0 }, { type: "cm", id: 1, prime: 1 }] },
        { op: "add", dest: T(1), src: [T(0), { type: "const", id: 1, prime: -1 }] },
        { op: "mul", dest: T(2), src: [{ type: "challenge", stage: 2, stageId: 0 }, { type: "public", id: 0 }] },
        { op: "sub", dest: T(3), src: [T(1), T(2)] },
        { op: "add", dest: { type: "cm", id: 2, prime: 0 }, src: [T(3), { type: "number", value: "-3" }] },
    ] };
    await callCalculateExps("stage2", imPol, "n", ctx, false, false, false);
    const minus3 = mod(-3n) * MONT % R;
    const wantCm2 = h.cm1_n.map((row, i) => [mod(fmul(row[0], h.cm1_n[(i + 1) % N][1]) + h.const_n[(i + N - 1) % N][1] - fmul(chal, pub) + minus3)]);
    same("domain n", fromDev(ctx.cm2_n, N, 1), wantCm2);
    same("domain n left cm1 alone", fromDev(ctx.cm1_n, N, 2), h.cm1_n);

    // ---- domain ext with ret: q = (cm1_0[-1] * x - const_0[+1]) * Zi(lastRow); prime -1 / +1 are 4 rows back / ahead.  The value returned is
    // the last op's, a temporary (the reference's getRef has no "q": compileCode could not return one)
    const qCode = { tmpUsed: 3, code: [
        { op: "mul", dest: T(0), src: [{ type: "cm", id: 0, prime: -1 }, { type: "x" }] },
        { op: "sub", dest: T(1), src: [T(0), { type: "const", id: 0, prime: 1 }] },
        { op: "mul", dest: { type: "q", dim: 1 }, src: [T(1), { type: "Zi", boundaryId: 1 }] },
        { op: "add", dest: T(2), src: [T(1), { type: "x" }] },
    ] };
    const res = calculateExps(ctx, qCode, "ext", false, true);
    const wantQ = h.x_ext.map((x, i) => [fmul(mod(fmul(h.cm1_ext[(i + extN - 4) % extN][0], x[0]) - h.const_ext[(i + 4) % extN][0]), h.Zi_ext[extN + i][0])]);
    same("domain ext q_ext", fromDev(ctx.q_ext, extN, 1), wantQ);
    if (res.length !== extN) throw new Error("ret: expected " + extN + " values");
    for (let i = 0; i < extN; i++) {
        const want = mod(fmul(h.cm1_ext[(i + extN - 4) % extN][0], h.x_ext[i][0]) - h.const_ext[(i + 4) % extN][0] + h.x_ext[i][0]);
        if (!(res[i] instanceof Uint8Array) || res[i].length !== 32 || fromBytes(res[i]) !== want) throw new Error("ret: row " + i + " differs");
    }

    // ---- debug: the constraint cm2 - (what the first program computed) holds on every row until row 11 is spoilt
    const cons = { boundary: "everyRow", line: "test.pil:7", tmpUsed: 5, code: imPol.code.slice(0, 4).concat([
        { op: "add", dest: T(4), src: [T(3), { type: "number", value: "-3" }] },
        { op: "sub", dest: T(0), src: [{ type: "cm", id: 2, prime: 0 }, T(4)] }]) };
    calculateExps(ctx, cons, "n", true, false);
    if (ctx.errors.length) throw new Error("a constraint that holds was reported: " + ctx.errors[0]);
    for (const row of [13, 11]) {
        const off = row * 4, w = ctx.cm2_n.slice(off, off + 4);
        w[0] = w[0] ^ 1n;                                      // some other canonical value: the low bit flipped
        ctx.cm2_n.set(w, off);
    }
    calculateExps(ctx, cons, "n", true, false);
    const bad = mod((wantCm2[11][0] ^ 1n) - wantCm2[11][0]);
    const wantMsg = "test.pil:7: identity does not match w=11 val=" + (bad * MONT_INV % R).toString(10) + " ";
    if (ctx.errors.length !== 1 || ctx.errors[0] !== wantMsg) throw new Error("debug path: got " + JSON.stringify(ctx.errors) + ", want " + wantMsg);
    ctx.errors = [];
    calculateExps(ctx, Object.assign({}, cons, { boundary: "everyFrame", offsetMin: 12, offsetMax: 3 }), "n", true, false);      // rows [12, 13): neither spoilt row
    if (ctx.errors.length) throw new Error("a row outside the boundary was reported");

    let threw = false;
    try { calculateExps(ctx, { code: [{ op: "copy", dest: { type: "q", dim: 1 }, src: [T(0)] }] }, "n", false, false); } catch (e) { threw = /Accessing q in domain n/.test(e.message); }
    if (!threw) throw new Error("q on domain n was accepted");
    for (const k of Object.keys(h)) ctx[k].free();
    console.log("expr bn128 parity OK");
}
main().catch((e) => { console.error(e && e.stack || e); process.exit(1); });
