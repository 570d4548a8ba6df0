// js/pil_checks.js rangeSum (host matrices as words and as bytes) and rangeSumDev (DevBuffer sections), and calculateSRange /
// calculateSRangeDev of js/polutils.js and js/polutils_bn128.js, from Node against what the Python checker says: every word of every matrix
// after the call (the column written, everything else untouched).  A name used twice in a case is ONE buffer, so that out can be spare
// columns of m's matrix.  usage: node range_sum_parity.js job.json; exits non-zero on the first difference.
"use strict";
const fs = require("fs");
const path = require("path");
const m = require(path.join(__dirname, "..", "..", "pil2-stark-js_amd", "js", "index.js"));
const C = m.pil_checks;

const bytes = (hex) => Uint8Array.from(Buffer.from(hex, "hex"));
const asWords = (u8) => new BigUint64Array(u8.buffer);
function same(what, got, want) { if (got !== want) throw new Error(what + ": got " + String(got).slice(0, 400) + ", expected " + String(want).slice(0, 400)); }
const hexOf = (words) => Buffer.from(words.buffer, words.byteOffset, words.byteLength).toString("hex");

function main() {
    const job = JSON.parse(fs.readFileSync(process.argv[2], "utf8"));
    for (const c of job.cases) {
        const bn = c.field === "bn128", opts = { bn128: bn }, P = bn ? m.polutils_bn128 : m.polutils;
        const elem = (hex) => bn ? asWords(bytes(hex)) : asWords(bytes(hex))[0];
        const dev = (u8) => m.DevBuffer.from(asWords(u8));
        const forms = [["words", asWords, (t, r, a, b, o, n) => C.rangeSum(t, r, a, b, o, n, opts)], ["bytes", (u8) => u8, (t, r, a, b, o, n) => C.rangeSum(t, r, a, b, o, n, opts)],
                       ["resident", dev, (t, r, a, b, o, n) => C.rangeSumDev(t, r, a, b, o, n, opts)], ["polutils", asWords, P.calculateSRange],
                       ["polutils resident", dev, P.calculateSRangeDev]];
        for (const [name, wrap, fn] of forms) {
            const bufs = {}, resident = name.endsWith("resident");
            for (const k of Object.keys(c.mats)) bufs[k] = wrap(bytes(c.mats[k].words));
            const term = (s) => ({ buf: bufs[s.mat], stride: c.mats[s.mat].stride, cols: s.cols, coef: elem(s.coef), busId: elem(s.busId),
                                   sel: s.sel ? { buf: bufs[s.sel.mat], stride: c.mats[s.sel.mat].stride, col: s.sel.col } : undefined });
            const range = (r) => ({ m: { buf: bufs[r.mat], stride: c.mats[r.mat].stride, col: r.col }, lo: BigInt(r.lo), size: r.size, row0: r.row0, coef: elem(r.coef), busId: elem(r.busId) });
            fn(c.terms.map(term), c.ranges.map(range), asWords(bytes(c.alpha)), name === "bytes" && bn ? bytes(c.beta) : asWords(bytes(c.beta)),
               { buf: bufs[c.out.mat], stride: c.mats[c.out.mat].stride, col: c.out.col }, c.n);
            for (const k of Object.keys(c.mats)) {
                const b = bufs[k], after = resident ? b.slice(0, b.length) : name === "bytes" ? asWords(Uint8Array.from(b)) : b;
                same(c.name + ", " + name + ", matrix " + k, hexOf(after), c.after[k]);
            }
            if (resident) Object.keys(bufs).forEach((k) => bufs[k].free());
        }
        const plan = C.rangeSumPlan(c.n, c.terms.length, c.ranges.length, bn);
        same(c.name + ", plan", JSON.stringify([plan.launches, plan.outWidth]), JSON.stringify(c.plan));
    }
    console.log("range sum parity OK");
}
try { main(); process.exit(0); } catch (e) { console.error(e.stack || e); process.exit(1); }
