// js/pil_checks.js logupCluster (host matrices as words and as bytes) and logupClusterDev (DevBuffer sections), and calculateSClustered /
// calculateSClusteredDev of js/polutils.js and js/polutils_bn128.js, from Node against what the Python checker says: every word of every
// matrix after the call (s and the im columns written, everything else untouched).  A name used twice in a case is ONE buffer, so that s and
// the im columns can be columns of one matrix, or spare columns of a matrix that is read.  usage: node logup_cluster_parity.js job.json;
// exits non-zero on the first difference.
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
    same("the addon's layout of pil2gl_logup_im_col", JSON.stringify(m.native.logupImColLayout()), JSON.stringify(job.layout));
    for (const c of job.cases) {
        const bn = c.field === "bn128", opts = { bn128: bn }, P = bn ? m.polutils_bn128 : m.polutils;
        const elem = (hex) => bn ? asWords(bytes(hex)) : asWords(bytes(hex))[0];
        const dev = (u8) => m.DevBuffer.from(asWords(u8));
        const host = (t, r, cl, im, a, b, o, n) => C.logupCluster(t, r, cl, im, a, b, o, n, opts);
        const forms = [["words", asWords, host], ["bytes", (u8) => u8, host], ["resident", dev, (t, r, cl, im, a, b, o, n) => C.logupClusterDev(t, r, cl, im, a, b, o, n, opts)],
                       ["polutils", asWords, P.calculateSClustered], ["polutils resident", dev, P.calculateSClusteredDev]];
        for (const [name, wrap, fn] of forms) {
            const bufs = {}, resident = name.endsWith("resident");
            for (const k of Object.keys(c.mats)) bufs[k] = wrap(bytes(c.mats[k].words));
            const term = (s) => ({ buf: bufs[s.mat], stride: c.mats[s.mat].stride, cols: s.cols, coef: elem(s.coef), busId: elem(s.busId),
                                   sel: s.sel ? { buf: bufs[s.sel.mat], stride: c.mats[s.sel.mat].stride, col: s.sel.col } : undefined });
            const range = (r) => ({ m: { buf: bufs[r.mat], stride: c.mats[r.mat].stride, col: r.col }, lo: BigInt(r.lo), size: r.size, row0: r.row0, coef: elem(r.coef), busId: elem(r.busId) });
            const column = (o) => ({ buf: bufs[o.mat], stride: c.mats[o.mat].stride, col: o.col });
            fn(c.terms.map(term), c.ranges.map(range), c.cluster.map((g) => g === "D" ? C.DIRECT : g), c.im.map(column), asWords(bytes(c.alpha)),
               name === "bytes" && bn ? bytes(c.beta) : asWords(bytes(c.beta)), column(c.out), c.n);
            for (const k of Object.keys(c.mats)) {
                const b = bufs[k], after = resident ? b.slice(0, b.length) : name === "bytes" ? asWords(Uint8Array.from(b)) : b;
                same(c.name + ", " + name + ", matrix " + k, hexOf(after), c.after[k]);
            }
            if (resident) Object.keys(bufs).forEach((k) => bufs[k].free());
        }
        const plan = C.logupClusterPlan(c.n, c.terms.length, c.ranges.length, c.im.length, bn);
        same(c.name + ", plan", JSON.stringify([plan.launches, plan.outWidth]), JSON.stringify(c.plan));
    }
    console.log("logup cluster parity OK");
}
try { main(); process.exit(0); } catch (e) { console.error(e.stack || e); process.exit(1); }
