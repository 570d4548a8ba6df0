// js/polutils_bn128.js from Node: the array forms of calculateZ / calculateS / batchInverse and the resident DevBuffer column forms,
// against a job file the Python test wrote with its checker's expectations (Montgomery bytes, hex).
// usage: node hints_bn128_parity.js job.json; exits non-zero on the first difference.
"use strict";
const fs = require("fs");
const path = require("path");
const m = require(path.join(__dirname, "..", "..", "pil2-stark-js_amd", "js", "index.js"));
const P = m.polutils_bn128;

const bytes = (hex) => Uint8Array.from(Buffer.from(hex, "hex"));
const hexOf = (u8) => Buffer.from(u8.buffer, u8.byteOffset, u8.byteLength).toString("hex");
const elems = (hex) => { const b = bytes(hex), out = []; for (let o = 0; o < b.length; o += 32) out.push(b.slice(o, o + 32)); return out; };
const join = (arr) => arr.map(hexOf).join("");
const toDev = (u8) => m.DevBuffer.from(new BigUint64Array(u8.buffer.slice(u8.byteOffset, u8.byteOffset + u8.byteLength)));
const fromDev = (d) => { const w = d.toHost(); return new Uint8Array(w.buffer, w.byteOffset, w.byteLength); };
function same(what, gotHex, wantHex) { if (gotHex !== wantHex) throw new Error(what + " differs"); }

async function main() {
    const job = JSON.parse(fs.readFileSync(process.argv[2], "utf8"));
    for (const c of job.arrays) {
        const num = elems(c.num), den = elems(c.den);
        const z = await P.calculateZ(null, num, den);
        if (z.length !== c.n || !(z[0] instanceof Uint8Array) || z[0].byteLength !== 32) throw new Error("calculateZ: shape");
        same("calculateZ n = " + c.n, join(z), c.z);
        same("calculateS n = " + c.n, join(await P.calculateS(null, num[0], den)), c.s);
        same("batchInverse n = " + c.n, join(P.batchInverse(null, den)), c.inv);
        same("the inputs", join(num) + join(den), c.num + c.den);
    }
    // resident: num and den are columns of one section, z and s go to columns of another, the inverse in place
    const r = job.resident;
    const sec = toDev(bytes(r.section)), dst = toDev(bytes(r.dst));
    const num = { buf: sec, stride: r.width, offset: r.numCol }, den = { buf: sec, stride: r.width, offset: r.denCol };
    const zc = { buf: dst, stride: r.dstWidth, offset: r.zCol }, sc = { buf: dst, stride: r.dstWidth, offset: r.sCol };
    if (P.calculateZDev(num, den, r.n, zc) !== zc) throw new Error("calculateZDev must return its out column");
    P.calculateSDev(bytes(r.numElem), den, r.n, sc);
    same("resident z and s", hexOf(fromDev(dst)), r.wantDst);
    same("the result field", hexOf(P.lastElement(zc, r.n)), r.wantResult);
    same("the section after the hints", hexOf(fromDev(sec)), r.section);
    P.batchInverseDev(den, r.n, den);
    same("resident inverse in place", hexOf(fromDev(sec)), r.wantSection);
    let msg = null;
    try { P.calculateZDev(num, den, r.n, den); } catch (e) { msg = e.message; }
    if (!msg || !/overlaps/.test(msg)) throw new Error("a hint over its own input: got " + JSON.stringify(msg));
    sec.free(); dst.free();
    console.log("hints bn128 parity OK");
}
main().catch((e) => { console.error(e && e.stack || e); process.exit(1); });
