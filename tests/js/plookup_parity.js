// The plookup argument from Node against what the Python checker says: js/pil_checks.js plookupFold / plookupProduct (host matrices as words
// and as bytes) and their Dev forms (DevBuffer sections), and the spellings of js/polutils.js and js/polutils_bn128.js --
// calculateH1H2Plookup[Dev] and calculateZPlookup[Dev].  Every word of the matrix after a call (the columns written, everything else
// untouched), h1 and h2 word for word, and the h1h2 error for a value of f that t lacks.  usage: node plookup_parity.js job.json; exits
// non-zero on the first difference.
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
        const bn = c.field === "bn128", opts = { bn128: bn, hDim: c.hDim }, P = bn ? m.polutils_bn128 : m.polutils, ew = bn ? 4 : 1;
        const dev = (u8) => m.DevBuffer.from(asWords(u8));
        const ch = (hex) => asWords(bytes(hex));
        const chs = [c.alpha, c.beta, c.gamma, c.delta].map(ch);
        const tail = bn ? [] : [c.hDim];
        const sides = (buf) => {
            const col = (k) => k === null ? undefined : { buf, stride: c.stride, col: k };
            return { f: { buf, stride: c.stride, cols: c.f.cols, sel: col(c.f.sel) }, t: { buf, stride: c.stride, cols: c.t.cols, sel: col(c.t.sel) }, col };
        };
        const read = (buf, resident, asBytes) => resident ? buf.slice(0, buf.length) : asBytes ? asWords(Uint8Array.from(buf)) : buf;
        // the product: z into its column of the one matrix
        for (const [name, wrap, resident] of [["words", asWords, false], ["bytes", (u8) => u8, false], ["resident", dev, true], ["spelling", asWords, false],
                                              ["resident spelling", dev, true]]) {
            const buf = wrap(bytes(c.mat)), s = sides(buf);
            const args = [s.f, s.t, s.col(c.h1), s.col(c.h2)].concat(chs, [s.col(c.z), c.n]);
            if (name.endsWith("spelling")) (resident ? P.calculateZPlookupDev : P.calculateZPlookup)(...args, ...tail);
            else (resident ? C.plookupProductDev : C.plookupProduct)(...args, opts);
            same(c.name + ", product, " + name, hexOf(read(buf, resident, name === "bytes")), c.afterProd);
            if (resident) buf.free();
        }
        // the fold: F and T where h1 and h2 will lie
        for (const [name, wrap, resident] of [["words", asWords, false], ["bytes", (u8) => u8, false], ["resident", dev, true]]) {
            const buf = wrap(bytes(c.mat)), s = sides(buf);
            (resident ? C.plookupFoldDev : C.plookupFold)(s.f, s.t, chs[0], chs[1], s.col(c.h1), s.col(c.h2), c.n, opts);
            same(c.name + ", fold, " + name, hexOf(read(buf, resident, name === "bytes")), c.afterFold);
            if (resident) buf.free();
        }
        // h1 and h2 from the trace columns
        {
            const s = sides(asWords(bytes(c.mat)));
            const [h1, h2] = P.calculateH1H2Plookup(s.f, s.t, chs[0], chs[1], c.n, ...tail);
            const hex = (h) => bn ? h.map((e) => Buffer.from(e).toString("hex")).join("") : hexOf(h);
            same(c.name + ", h1", hex(h1), c.h1Words);
            same(c.name + ", h2", hex(h2), c.h2Words);
            const d = dev(bytes(c.mat)), sd = sides(d);
            const [d1, d2] = P.calculateH1H2PlookupDev(sd.f, sd.t, chs[0], chs[1], c.n, ...tail);
            if (bn) {
                const all = d1.buf.slice(0, d1.buf.length);
                const pick = (o) => { const w = new BigUint64Array(4 * c.n); for (let i = 0; i < c.n; i++) w.set(all.subarray(8 * i + 4 * o, 8 * i + 4 * o + 4), 4 * i); return w; };
                same(c.name + ", resident h1", hexOf(pick(d1.offset)), c.h1Words);
                same(c.name + ", resident h2", hexOf(pick(d2.offset)), c.h2Words);
                d1.buf.free();
            } else {
                same(c.name + ", resident h1", hexOf(d1.slice(0, d1.length)), c.h1Words);
                same(c.name + ", resident h2", hexOf(d2.slice(0, d2.length)), c.h2Words);
                d1.free(); d2.free();
            }
            d.free();
            // a value of f that t lacks
            for (const resident of [false, true]) {
                const b = resident ? dev(bytes(c.badMat)) : asWords(bytes(c.badMat)), sb = sides(b);
                let msg = "";
                try { (resident ? P.calculateH1H2PlookupDev : P.calculateH1H2Plookup)(sb.f, sb.t, chs[0], chs[1], c.n, ...tail); } catch (e) { msg = String(e.message); }
                if (!msg.includes("Number not included: w:" + c.badRow)) throw new Error(c.name + ", missing value" + (resident ? ", resident" : "") + ": got '" + msg + "'");
                if (resident) b.free();
            }
        }
        const plan = C.plookupPlan(c.n, c.f.cols.length, c.t.cols.length, bn);
        same(c.name + ", plan", JSON.stringify([plan.launches, plan.outWidth]), JSON.stringify(c.plan));
        void ew;
    }
    console.log("plookup parity OK");
}
try { main(); process.exit(0); } catch (e) { console.error(e.stack || e); process.exit(1); }
