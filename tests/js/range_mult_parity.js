// js/pil_checks.js from Node: rangeMultiplicities on host matrices (words and bytes) and rangeMultiplicitiesDev on DevBuffer sections,
// against what the Python checker says: `matched`, the missing pair with the formatter's message, and every word of every matrix after the
// call (m written, everything else untouched).  A name used twice in a case is ONE buffer, so that m can be a spare column of an f's
// matrix.  usage: node range_mult_parity.js job.json; exits non-zero on the first difference.
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
        const bn128 = c.field === "bn128", opts = { bn128, row0: c.row0 };
        const asWords = (u8) => new BigUint64Array(u8.buffer), asBytes = (u8) => u8, dev = (u8) => m.DevBuffer.from(asWords(u8));
        for (const [name, wrap, fn] of [["words", asWords, C.rangeMultiplicities], ["bytes", asBytes, C.rangeMultiplicities], ["resident", dev, C.rangeMultiplicitiesDev]]) {
            const bufs = {};
            for (const k of Object.keys(c.mats)) bufs[k] = wrap(bytes(c.mats[k].words));
            const side = (s) => ({ buf: bufs[s.mat], stride: c.mats[s.mat].stride, cols: s.cols, sel: s.sel ? { buf: bufs[s.sel.mat], stride: c.mats[s.sel.mat].stride, col: s.sel.col } : undefined });
            const lo = name === "bytes" && Number.isSafeInteger(Number(c.lo)) ? Number(c.lo) : BigInt(c.lo);      // a plain integer where it is one
            const got = fn(c.fs.map(side), lo, c.size, { buf: bufs[c.m.mat], stride: c.mats[c.m.mat].stride, col: c.m.col }, c.n, opts);
            same(c.name + ", " + name, plain(got), c.want);
            for (const k of Object.keys(c.mats)) {
                const b = bufs[k], after = name === "resident" ? b.slice(0, b.length) : name === "bytes" ? asWords(Uint8Array.from(b)) : b;
                same(c.name + ", " + name + ", matrix " + k, hexOf(after), c.after[k]);
            }
            if (name === "resident") Object.keys(bufs).forEach((k) => bufs[k].free());
        }
        const plan = C.rangeMultPlan(c.n, c.size, c.fs.length, bn128);
        same(c.name + ", plan", [plan.launches, plan.headerBytes, plan.scratchBytes], [2 + c.fs.length, 64, Math.ceil((64 + 4 * c.size) / 16) * 16]);
    }
    console.log("range mult parity OK");
}
try { main(); process.exit(0); } catch (e) { console.error(e.stack || e); process.exit(1); }
