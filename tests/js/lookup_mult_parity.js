// js/pil_checks.js from Node: lookupMultiplicities on host matrices (words and bytes) and lookupMultiplicitiesDev on DevBuffer sections,
// against what the Python checker says: `matched`, the missing pair with the formatter's message, and every word of m's matrix after the
// call (m written, its other columns untouched).  A name used twice in a case is ONE buffer, so that m can be a spare column of t's or of
// an f's matrix.  usage: node lookup_mult_parity.js job.json; exits non-zero on the first difference.
"use strict";
const fs = require("fs");
const path = require("path");
const m = require(path.join(__dirname, "..", "..", "pil2-stark-js_amd", "js", "index.js"));
const C = m.pil_checks;

const bytes = (hex) => Uint8Array.from(Buffer.from(hex, "hex"));
function same(what, got, want) { if (JSON.stringify(got) !== JSON.stringify(want)) throw new Error(what + ": got " + JSON.stringify(got) + ", expected " + JSON.stringify(want)); }
const plain = (r) => ({ matched: r.matched, missing: r.missing === null ? null : { side: r.missing.side, row: r.missing.row, message: r.missing.message() } });
const hexOf = (words) => Buffer.from(words.buffer, words.byteOffset, words.byteLength).toString("hex");

function main() {
    const job = JSON.parse(fs.readFileSync(process.argv[2], "utf8"));
    for (const c of job.cases) {
        const opts = { bn128: c.field === "bn128" };
        const asWords = (u8) => new BigUint64Array(u8.buffer), asBytes = (u8) => u8, dev = (u8) => m.DevBuffer.from(asWords(u8));
        for (const [name, wrap, fn] of [["words", asWords, C.lookupMultiplicities], ["bytes", asBytes, C.lookupMultiplicities], ["resident", dev, C.lookupMultiplicitiesDev]]) {
            const bufs = {};
            for (const k of Object.keys(c.mats)) bufs[k] = wrap(bytes(c.mats[k].words));
            const side = (s) => ({ buf: bufs[s.mat], stride: c.mats[s.mat].stride, cols: s.cols, sel: s.sel ? { buf: bufs[s.sel.mat], stride: c.mats[s.sel.mat].stride, col: s.sel.col } : undefined });
            const got = fn(c.fs.map(side), side(c.t), { buf: bufs[c.m.mat], stride: c.mats[c.m.mat].stride, col: c.m.col }, c.n, opts);
            same(c.name + ", " + name, plain(got), c.want);
            for (const k of Object.keys(c.mats)) {
                const b = bufs[k], after = name === "resident" ? b.slice(0, b.length) : name === "bytes" ? asWords(Uint8Array.from(b)) : b;
                same(c.name + ", " + name + ", matrix " + k, hexOf(after), c.after[k]);
            }
            if (name === "resident") Object.keys(bufs).forEach((k) => bufs[k].free());
        }
    }
    if (!(C.lookupMultProbe() >= 0)) throw new Error("lookupMultProbe");
    console.log("lookup mult parity OK");
}
try { main(); process.exit(0); } catch (e) { console.error(e.stack || e); process.exit(1); }
