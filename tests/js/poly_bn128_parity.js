// js/polynomial_bn128.js from Node: divZh on a DevBuffer (divisible, and not: the reference's message), divByXNSubValue on a DevBuffer
// column and on a staged Uint8Array, evaluate -- against a job file the Python test wrote with its checker's expectations.  Then the
// write-back in several pieces: a strided division staged in 1024-byte pieces leaves the bytes it leaves in one piece.
// usage: node poly_bn128_parity.js job.json; exits non-zero on the first difference.
"use strict";
const fs = require("fs");
const path = require("path");
const m = require(path.join(__dirname, "..", "..", "pil2-stark-js_amd", "js", "index.js"));
const P = m.polynomial_bn128;
const stage = require(path.join(__dirname, "..", "..", "pil2-stark-js_amd", "js", "bn128_stage.js"));

const bytes = (hex) => Uint8Array.from(Buffer.from(hex, "hex"));
const hexOf = (u8) => Buffer.from(u8.buffer, u8.byteOffset, u8.byteLength).toString("hex");
const toDev = (u8) => m.DevBuffer.from(new BigUint64Array(u8.buffer.slice(u8.byteOffset, u8.byteOffset + u8.byteLength)));
const fromDev = (d) => { const w = d.toHost(); return new Uint8Array(w.buffer, w.byteOffset, w.byteLength); };
function same(what, got, wantHex) { if (hexOf(got) !== wantHex) throw new Error(what + " differs"); }

function main() {
    const job = JSON.parse(fs.readFileSync(process.argv[2], "utf8"));

    // divZh, divisible: the quotient from domainSize on, zeros below
    let d = toDev(bytes(job.divzh.c));
    if (P.divZh(d, job.divzh.N) !== d) throw new Error("divZh must return its buffer");
    same("divZh", fromDev(d), job.divzh.want);
    d.free();

    // not divisible: the reference's message
    d = toDev(bytes(job.divzh.spoilt));
    let msg = null;
    try { P.divZh(d, job.divzh.N); } catch (e) { msg = e.message; }
    if (msg !== "Polynomial is not divisible") throw new Error("divZh of a non-multiple: got " + JSON.stringify(msg));
    d.free();

    // divByXNSubValue: one column of a resident matrix, then a staged Uint8Array
    for (const c of job.div) {
        d = toDev(bytes(c.m));
        const col = d.view(4 * c.col, d.length - 4 * c.col);
        if (P.divByXNSubValue(col, c.k, bytes(c.beta), { n: c.n, stride: c.stride }) !== col) throw new Error("divByXNSubValue must return its buffer");
        same("divByXNSubValue (DevBuffer) k = " + c.k, fromDev(d), c.want);
        d.free();
        const u8 = bytes(c.m).subarray(32 * c.col);
        P.divByXNSubValue(u8, c.k, bytes(c.beta), { n: c.n, stride: c.stride });
        same("divByXNSubValue (Uint8Array) k = " + c.k, u8, c.want.slice(64 * c.col));
    }

    // the same division staged in 1024-byte pieces: n = 100 at stride 3 is 9536 bytes, up and back in ten pieces
    {
        const c = job.div.find((x) => x.k === 5 && x.stride === 3), n = 100, staged = ((n - 1) * c.stride + 1) * 32;
        const orig = bytes(c.m).subarray(32 * c.col), one = Uint8Array.from(orig), many = Uint8Array.from(orig);
        P.divByXNSubValue(one, c.k, bytes(c.beta), { n, stride: c.stride });
        const was = stage.setPieceBytes(1024);
        try { P.divByXNSubValue(many, c.k, bytes(c.beta), { n, stride: c.stride }); } finally { stage.setPieceBytes(was); }
        same("divByXNSubValue in 1024-byte pieces", many, hexOf(one));
        if (hexOf(one.subarray(0, staged)) === hexOf(orig.subarray(0, staged))) throw new Error("the division changed nothing");
        for (let e = 0; 32 * e < many.length; e++)           // the elements between the column's, and everything past what was staged
            if (e % c.stride !== 0 || 32 * e >= staged) same("element " + e + " outside the column", many.subarray(32 * e, 32 * e + 32), hexOf(orig.subarray(32 * e, 32 * e + 32)));
    }

    // evaluate: resident and staged; the coefficients stay as they were
    d = toDev(bytes(job.eval.c));
    const pts = job.eval.points.map(bytes);
    for (const buf of [d, bytes(job.eval.c)]) {
        const got = P.evaluate(buf, pts);
        if (got.length !== pts.length) throw new Error("evaluate: " + got.length + " values");
        got.forEach((v, i) => same("evaluate point " + i, v, job.eval.want[i]));
    }
    same("evaluate left the coefficients alone", fromDev(d), job.eval.c);
    d.free();
    console.log("poly bn128 parity OK");
}
try { main(); } catch (e) { console.error(e && e.stack || e); process.exit(1); }
