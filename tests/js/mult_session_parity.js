// js/pil_checks.js from Node: one LookupSession and one RangeSession per case, fed the adds of the job on DevBuffer matrices, against what
// pilcheck's sessions gave on the same words: every add's report, the total, and every byte of m's matrix after the write.
// usage: node mult_session_parity.js job.json; exits non-zero on the first difference.
"use strict";
const fs = require("fs");
const path = require("path");
const m = require(path.join(__dirname, "..", "..", "pil2-stark-js_amd", "js", "index.js"));
const C = m.pil_checks;

const dev = (hex) => m.DevBuffer.from(new BigUint64Array(Uint8Array.from(Buffer.from(hex, "hex")).buffer));
function same(what, got, want) { if (JSON.stringify(got) !== JSON.stringify(want)) throw new Error(what + ": got " + JSON.stringify(got) + ", expected " + JSON.stringify(want)); }
const hexOf = (words) => Buffer.from(words.buffer, words.byteOffset, words.byteLength).toString("hex");

function main() {
    const job = JSON.parse(fs.readFileSync(process.argv[2], "utf8"));
    for (const c of job.cases) {
        const opts = { bn128: c.field === "bn128" };
        const bufs = {};
        for (const k of Object.keys(c.mats)) bufs[k] = dev(c.mats[k].words);
        const side = (s) => ({ buf: bufs[s.mat], stride: c.mats[s.mat].stride, cols: s.cols, sel: s.sel ? { buf: bufs[s.sel.mat], stride: c.mats[s.sel.mat].stride, col: s.sel.col } : undefined });
        const s = c.kind === "lookup" ? new C.LookupSession(side(c.t), c.nT, opts) : new C.RangeSession(BigInt(c.lo), c.size, opts);
        same(c.name + ", plan", s.plan, c.kind === "lookup" ? C.lookupSessionPlan(c.nT, c.t.cols.length, opts.bn128) : C.rangeSessionPlan(c.size, opts.bn128));
        same(c.name + ", scratch", s.plan.scratchBytes, c.scratchBytes);
        c.adds.forEach((a, i) => {
            const got = s.add(a.fs.map(side), a.rows);
            same(c.name + ", add " + i, { matched: typeof got.matched + " " + got.matched, missing: got.missing }, { matched: "bigint " + a.want.matched, missing: a.want.missing });
        });
        const out = { buf: bufs[c.m.mat], stride: c.mats[c.m.mat].stride, col: c.m.col };
        const total = c.kind === "lookup" ? s.write(out) : s.write(out, c.nM, c.row0);
        same(c.name + ", total", typeof total + " " + total, "bigint " + c.total);
        for (const k of Object.keys(c.mats)) same(c.name + ", matrix " + k, hexOf(bufs[k].slice(0, bufs[k].length)), c.after[k]);
        s.free();
        Object.keys(bufs).forEach((k) => bufs[k].free());
    }
    console.log("mult session parity OK");
}
try { main(); process.exit(0); } catch (e) { console.error(e.stack || e); process.exit(1); }
