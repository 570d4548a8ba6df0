// js/polynomial_bn128.js from Node: add, sub, mulScalar, byXSubValue, byXNSubValue, mulSparse and degree on DevBuffers (resident) and on
// staged Uint8Arrays, zerofierTerms, and the overlap refusal's message -- against a job file the Python test wrote with its checker's
// expectations.  usage: node polymul_bn128_parity.js job.json; exits non-zero on the first difference.
"use strict";
const fs = require("fs");
const path = require("path");
const m = require(path.join(__dirname, "..", "..", "pil2-stark-js_amd", "js", "index.js"));
const P = m.polynomial_bn128;

const bytes = (hex) => Uint8Array.from(Buffer.from(hex, "hex"));
const hexOf = (u8) => Buffer.from(u8.buffer, u8.byteOffset, u8.byteLength).toString("hex");
const toDev = (u8) => m.DevBuffer.from(new BigUint64Array(u8.buffer.slice(u8.byteOffset, u8.byteOffset + u8.byteLength)));
const fromDev = (d) => { const w = d.toHost(); return new Uint8Array(w.buffer, w.byteOffset, w.byteLength); };
function same(what, got, wantHex) { if (hexOf(got) !== wantHex) throw new Error(what + " differs"); }
const poison = (n) => new Uint8Array(32 * n).fill(0xFF);

// fn(acc, src) -> the buffer holding the result; run resident and staged
function both(what, accHex, srcHex, wantHex, fn) {
    const dA = toDev(bytes(accHex)), dS = toDev(bytes(srcHex));
    const r = fn(dA, dS);
    if (r !== dA) throw new Error(what + " must return its destination");
    same(what + " (DevBuffer)", fromDev(dA), wantHex);
    same(what + " left src alone", fromDev(dS), srcHex);
    dA.free(); dS.free();
    const a = bytes(accHex), s = bytes(srcHex);
    fn(a, s);
    same(what + " (Uint8Array)", a, wantHex);
    same(what + " left src alone (Uint8Array)", s, srcHex);
}

function main() {
    const job = JSON.parse(fs.readFileSync(process.argv[2], "utf8"));
    const value = bytes(job.value);
    const poisonHex = (n) => hexOf(poison(n));

    both("add", job.acc, job.src, job.add, (a, s) => P.add(a, s));
    both("sub", job.acc, job.src, job.sub, (a, s) => P.sub(a, s));
    both("byXSubValue", poisonHex(job.nSrc + 1), job.src, job.byXSubValue, (d, s) => P.byXSubValue(s, value, d));
    both("byXNSubValue", poisonHex(job.nSrc + job.xn), job.src, job.byXNSubValue, (d, s) => P.byXNSubValue(s, job.xn, value, d));

    // mulScalar: in place, resident and staged
    let d = toDev(bytes(job.src));
    if (P.mulScalar(d, value) !== d) throw new Error("mulScalar must return its buffer");
    same("mulScalar (DevBuffer)", fromDev(d), job.mulScalar);
    d.free();
    let u8 = bytes(job.src);
    P.mulScalar(u8, value);
    same("mulScalar (Uint8Array)", u8, job.mulScalar);

    // columns of sections: src column 1 of width 3 into column 0 of a section 2 wide
    const st = job.strided;
    for (const resident of [true, false]) {
        const src = resident ? toDev(bytes(st.src)) : bytes(st.src), dst = resident ? toDev(bytes(st.dst)) : bytes(st.dst);
        const col = resident ? src.view(4, src.length - 4) : src.subarray(32);
        P.byXSubValue(col, value, dst, { n: st.n, stride: 3, dstStride: 2 });
        same("byXSubValue on columns, resident = " + resident, resident ? fromDev(dst) : dst, st.want);
        if (resident) { src.free(); dst.free(); }
    }

    // zerofierTerms against the checker, and its product in one sweep
    const z = job.zerofier;
    const terms = P.zerofierTerms(z.factors.map((f) => ({ k: f.k, beta: bytes(f.beta) })));
    if (terms.length !== z.terms.length) throw new Error("zerofierTerms: " + terms.length + " terms, want " + z.terms.length);
    terms.forEach((t, i) => { if (t.exp !== z.terms[i].exp) throw new Error("zerofierTerms: exponent " + i); same("zerofierTerms coefficient " + i, t.coef, z.terms[i].coef); });
    const cancel = P.zerofierTerms(z.cancel.factors.map((f) => ({ k: f.k, beta: bytes(f.beta) })));
    if (cancel.length !== 2) throw new Error("zerofierTerms keeps a cancelled coefficient");
    cancel.forEach((t, i) => { if (t.exp !== z.cancel.terms[i].exp) throw new Error("zerofierTerms (cancel): exponent " + i); same("zerofierTerms (cancel) coefficient " + i, t.coef, z.cancel.terms[i].coef); });
    let msg = null;
    try { P.zerofierTerms(z.tooMany.map((f) => ({ k: f.k, beta: bytes(f.beta) }))); } catch (e) { msg = e.message; }
    if (msg === null || !/at most 64/.test(msg)) throw new Error("zerofierTerms of 128 terms: got " + JSON.stringify(msg));
    const top = terms[terms.length - 1].exp;
    both("mulSparse", poisonHex(job.nSrc + top), job.src, z.mulSparse, (dd, s) => P.mulSparse(s, terms, dd));

    // a shifted product in place: the library's refusal, its message kept
    d = toDev(bytes(job.src));
    msg = null;
    try { P.fma(d, d, terms.slice(0, 2), { nAcc: job.nSrc, nSrc: job.nSrc - terms[1].exp }); } catch (e) { msg = e.message; }
    if (msg === null || !/acc overlaps src/.test(msg)) throw new Error("a shifted product in place: got " + JSON.stringify(msg));
    same("the refused call left the buffer alone", fromDev(d), job.src);
    d.free();

    // degree: resident and staged
    for (const c of job.degree) {
        d = toDev(bytes(c.c));
        if (P.degree(d) !== c.want) throw new Error("degree (DevBuffer): got " + P.degree(d) + ", want " + c.want);
        d.free();
        if (P.degree(bytes(c.c)) !== c.want) throw new Error("degree (Uint8Array): want " + c.want);
    }
    console.log("polymul bn128 parity OK");
}
try { main(); } catch (e) { console.error(e && e.stack || e); process.exit(1); }
