// js/pil_checks.js from Node: checkLookup / checkPermutation on host matrices (words and bytes) and checkLookupDev / checkPermutationDev
// on DevBuffer sections with column lists, against what the Python checker says: null for a clean trace, else the five words and the
// formatter's message.  usage: node tuple_check_parity.js job.json; exits non-zero on the first difference.
"use strict";
const fs = require("fs");
const path = require("path");
const m = require(path.join(__dirname, "..", "..", "pil2-stark-js_amd", "js", "index.js"));
const C = m.pil_checks;

const bytes = (hex) => Uint8Array.from(Buffer.from(hex, "hex"));
function same(what, got, want) { if (JSON.stringify(got) !== JSON.stringify(want)) throw new Error(what + ": got " + JSON.stringify(got) + ", expected " + JSON.stringify(want)); }
const plain = (r) => r === null ? null : { kind: r.kind, row: r.row, partner: r.partner, cntF: r.cntF, cntT: r.cntT, side: r.side, message: r.message() };

function main() {
    const job = JSON.parse(fs.readFileSync(process.argv[2], "utf8"));
    for (const c of job.cases) {
        const opts = { bn128: c.field === "bn128" };
        const host = (s, wrap) => s === null ? undefined : { buf: wrap(bytes(s.words)), stride: s.stride, cols: s.cols, col: s.col };
        const asWords = (u8) => new BigUint64Array(u8.buffer), asBytes = (u8) => u8;
        const devs = [];
        const dev = (u8) => { const d = m.DevBuffer.from(asWords(u8)); devs.push(d); return d; };
        for (const [name, wrap, lookup, perm] of [["words", asWords, C.checkLookup, C.checkPermutation], ["bytes", asBytes, C.checkLookup, C.checkPermutation],
                                                   ["resident", dev, C.checkLookupDev, C.checkPermutationDev]]) {
            const side = (s, sel) => Object.assign(host(s, wrap), { sel: host(sel, wrap) });
            const got = (c.mode === C.LOOKUP ? lookup : perm)(side(c.f, c.selF), side(c.t, c.selT), c.n, opts);
            same(c.name + ", " + name, plain(got), c.want);
        }
        if (c.one) {                                  // f and t as column sets of ONE resident matrix
            const d = dev(bytes(c.f.words));
            const got = (c.mode === C.LOOKUP ? C.checkLookupDev : C.checkPermutationDev)({ buf: d, stride: c.f.stride, cols: c.f.cols }, { buf: d, stride: c.t.stride, cols: c.t.cols }, c.n, opts);
            same(c.name + ", one matrix", plain(got), c.want);
        }
        devs.forEach((d) => d.free());
    }
    for (const h of job.homes) same("tupleHome " + JSON.stringify(h.words), C.tupleHome(BigUint64Array.from(h.words.map(BigInt)), h.k, h.capacity, h.bn128), h.home);
    if (!(C.tupleCheckProbe() >= 0)) throw new Error("tupleCheckProbe");
    console.log("tuple check parity OK");
}
try { main(); process.exit(0); } catch (e) { console.error(e.stack || e); process.exit(1); }
