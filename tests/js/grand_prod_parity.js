// js/pil_checks.js grandProduct (host matrices as words and as bytes) and grandProductDev (DevBuffer sections), and the two spellings of
// js/polutils.js and js/polutils_bn128.js (calculateZPermutation[Dev], calculateZConnection[Dev]), from Node against what the Python checker
// says: every word of every matrix after the call (the column written, everything else untouched).  A name used twice in a case is ONE
// buffer.  usage: node grand_prod_parity.js job.json; exits non-zero on the first difference.
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
        const dev = (u8) => m.DevBuffer.from(asWords(u8));
        const ch = (hex) => asWords(bytes(hex));
        for (const [name, wrap, resident] of [["words", asWords, false], ["bytes", (u8) => u8, false], ["resident", dev, true], ["spelling", asWords, false],
                                              ["resident spelling", dev, true]]) {
            const bufs = {};
            for (const k of Object.keys(c.mats)) bufs[k] = wrap(bytes(c.mats[k].words));
            const col = (s) => s ? { buf: bufs[s.mat], stride: c.mats[s.mat].stride, col: s.col } : undefined;
            const out = col(c.out);
            if (name.endsWith("spelling")) {
                if (c.perm) {
                    const sd = (s) => ({ buf: bufs[s.mat], stride: c.mats[s.mat].stride, cols: s.cols, sel: col(s.sel) });
                    (resident ? P.calculateZPermutationDev : P.calculateZPermutation)(sd(c.perm.f), sd(c.perm.t), ch(c.alpha), ch(c.beta), ch(c.gamma), out, c.n);
                } else {
                    (resident ? P.calculateZConnectionDev : P.calculateZConnection)(c.conn.a.map(col), c.conn.S.map(col), col(c.conn.x), ch(c.gamma), ch(c.conn.delta),
                                                                                      c.conn.deltaKs.map(ch), out, c.n);
                }
            } else {
                const term = (s) => ({ buf: bufs[s.mat], stride: c.mats[s.mat].stride, cols: s.cols, den: s.den, sel: col(s.sel), id: col(s.id),
                                       idCoef: s.id ? (name === "bytes" && bn ? bytes(s.idCoef) : ch(s.idCoef)) : undefined });
                (resident ? C.grandProductDev : C.grandProduct)(c.terms.map(term), ch(c.alpha), ch(c.beta), ch(c.gamma), out, c.n, opts);
            }
            for (const k of Object.keys(c.mats)) {
                const b = bufs[k], after = resident ? b.slice(0, b.length) : name === "bytes" ? asWords(Uint8Array.from(b)) : b;
                same(c.name + ", " + name + ", matrix " + k, hexOf(after), c.after[k]);
            }
            if (resident) Object.keys(bufs).forEach((k) => bufs[k].free());
        }
        const plan = C.grandProductPlan(c.n, c.terms.length, c.sumK, bn);
        same(c.name + ", plan", JSON.stringify([plan.launches, plan.outWidth]), JSON.stringify(c.plan));
    }
    console.log("grand product parity OK");
}
try { main(); process.exit(0); } catch (e) { console.error(e.stack || e); process.exit(1); }
