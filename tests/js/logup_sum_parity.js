// js/pil_checks.js logupSum (host matrices as words and as bytes) and logupSumDev (DevBuffer sections), and the column-numerator grand sum of
// js/polutils.js and js/polutils_bn128.js (array and resident forms), from Node against what the Python checker says: every word of every
// matrix after the call (the column written, everything else untouched).  A name used twice in a case is ONE buffer, so that out can be spare
// columns of t's matrix.  usage: node logup_sum_parity.js job.json; exits non-zero on the first difference.
"use strict";
const fs = require("fs");
const path = require("path");
const m = require(path.join(__dirname, "..", "..", "pil2-stark-js_amd", "js", "index.js"));
const C = m.pil_checks;

const bytes = (hex) => Uint8Array.from(Buffer.from(hex, "hex"));
const asWords = (u8) => new BigUint64Array(u8.buffer);
function same(what, got, want) { if (got !== want) throw new Error(what + ": got " + String(got).slice(0, 400) + ", expected " + String(want).slice(0, 400)); }
const hexOf = (words) => Buffer.from(words.buffer, words.byteOffset, words.byteLength).toString("hex");

async function main() {
    const job = JSON.parse(fs.readFileSync(process.argv[2], "utf8"));
    for (const c of job.cases) {
        const bn = c.field === "bn128", opts = { bn128: bn };
        const elem = (hex) => bn ? asWords(bytes(hex)) : asWords(bytes(hex))[0];
        const dev = (u8) => m.DevBuffer.from(asWords(u8));
        for (const [name, wrap, fn] of [["words", asWords, C.logupSum], ["bytes", (u8) => u8, C.logupSum], ["resident", dev, C.logupSumDev]]) {
            const bufs = {};
            for (const k of Object.keys(c.mats)) bufs[k] = wrap(bytes(c.mats[k].words));
            const term = (s) => ({ buf: bufs[s.mat], stride: c.mats[s.mat].stride, cols: s.cols, coef: elem(s.coef), busId: elem(s.busId),
                                   sel: s.sel ? { buf: bufs[s.sel.mat], stride: c.mats[s.sel.mat].stride, col: s.sel.col } : undefined });
            fn(c.terms.map(term), asWords(bytes(c.alpha)), name === "bytes" && bn ? bytes(c.beta) : asWords(bytes(c.beta)),
               { buf: bufs[c.out.mat], stride: c.mats[c.out.mat].stride, col: c.out.col }, c.n, opts);
            for (const k of Object.keys(c.mats)) {
                const b = bufs[k], after = name === "resident" ? b.slice(0, b.length) : name === "bytes" ? asWords(Uint8Array.from(b)) : b;
                same(c.name + ", " + name + ", matrix " + k, hexOf(after), c.after[k]);
            }
            if (name === "resident") Object.keys(bufs).forEach((k) => bufs[k].free());
        }
        const plan = C.logupSumPlan(c.n, c.terms.length, bn);
        same(c.name + ", plan", JSON.stringify([plan.launches, plan.outWidth]), JSON.stringify(c.plan));
    }
    for (const g of job.gsumCol) {
        if (g.field === "gl") {
            const rows = (hex, dim) => { const w = asWords(bytes(hex)), out = []; for (let i = 0; i < w.length / dim; i++) out.push(dim === 1 ? w[i] : [w[3 * i], w[3 * i + 1], w[3 * i + 2]]); return out; };
            const flat = (col) => hexOf(BigUint64Array.from([].concat(...col.map((e) => Array.isArray(e) ? e : [e]))));
            same(g.name + ", arrays", flat(await m.polutils.calculateSCol(null, rows(g.num, g.dimNum), rows(g.den, g.dimDen))), g.want);
            const dn = m.DevBuffer.from(asWords(bytes(g.num))), dd = m.DevBuffer.from(asWords(bytes(g.den))), out = new m.DevBuffer(g.n * Math.max(g.dimNum, g.dimDen));
            m.polutils.calculateSColDev(dn, g.dimNum, dd, g.dimDen, g.n, out);
            same(g.name + ", resident", hexOf(out.slice(0, out.length)), g.want);
            [dn, dd, out].forEach((b) => b.free());
        } else {
            const rows = (hex) => { const u = bytes(hex), out = []; for (let i = 0; i < u.length / 32; i++) out.push(u.slice(32 * i, 32 * i + 32)); return out; };
            const got = await m.polutils_bn128.calculateSCol(null, rows(g.num), rows(g.den));
            same(g.name + ", arrays", Buffer.concat(got.map((e) => Buffer.from(e))).toString("hex"), g.want);
            // resident: num and den as two columns of one section of stride 3, the result in the third
            const sec = new BigUint64Array(12 * g.n), nu = asWords(bytes(g.num)), de = asWords(bytes(g.den));
            for (let i = 0; i < g.n; i++) { sec.set(nu.subarray(4 * i, 4 * i + 4), 12 * i); sec.set(de.subarray(4 * i, 4 * i + 4), 12 * i + 4); }
            const d = m.DevBuffer.from(sec);
            m.polutils_bn128.calculateSColDev({ buf: d, stride: 3, offset: 0 }, { buf: d, stride: 3, offset: 1 }, g.n, { buf: d, stride: 3, offset: 2 });
            const after = d.slice(0, d.length), col = new BigUint64Array(4 * g.n);
            for (let i = 0; i < g.n; i++) {
                col.set(after.subarray(12 * i + 8, 12 * i + 12), 4 * i);
                same(g.name + ", resident, the inputs of row " + i, hexOf(after.subarray(12 * i, 12 * i + 8)), hexOf(sec.subarray(12 * i, 12 * i + 8)));
            }
            same(g.name + ", resident", hexOf(col), g.want);
            same(g.name + ", the hint's result", Buffer.from(m.polutils_bn128.lastElement({ buf: d, stride: 3, offset: 2 }, g.n)).toString("hex"), g.want.slice(-64));
            d.free();
        }
    }
    console.log("logup sum parity OK");
}
main().then(() => process.exit(0), (e) => { console.error(e.stack || e); process.exit(1); });
