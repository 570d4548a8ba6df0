// js/witness_exec.js from Node: connectionPols on a setup-shaped sMap (an array of nCols Uint32Array(N)) and connectionPolsDev on the
// resident sMap that prepareExec leaves in HBM, for both fields, against the words the Python checker's sequential swaps give.
// usage: node conn_pols_parity.js job.json; exits non-zero on the first difference.
"use strict";
const fs = require("fs");
const path = require("path");
const m = require(path.join(__dirname, "..", "..", "pil2-stark-js_amd", "js", "index.js"));
const W = m.witness_exec;

const bytes = (hex) => Uint8Array.from(Buffer.from(hex, "hex"));
const hexOf = (t) => Buffer.from(t.buffer, t.byteOffset, t.byteLength).toString("hex");
function same(what, got, want) { if (got !== want) throw new Error(what + " differs: " + String(got).slice(0, 200)); }

async function main() {
    const job = JSON.parse(fs.readFileSync(process.argv[2], "utf8"));
    for (const name of ["gl", "bn128"]) {
        const c = job[name], bn = name === "bn128", ew = bn ? 4 : 1, N = c.N, nCols = c.nCols;
        const elem = (x) => bn ? bytes(x) : BigInt(x);
        const w = elem(c.w), ks = c.ks.map(elem);
        // the field object the setups hold: F3g / curve.Fr as far as the call reads them
        const F = { n8: bn ? 32 : 8, one: elem(c.one), w: { [Math.log2(N)]: w } };
        const sMap = c.sMap.map((col) => Uint32Array.from(col));
        const S = W.connectionPols(F, sMap, N, ks);
        if (S.length !== nCols || S[0].length !== N) throw new Error(name + ": S is not [nCols][N]");
        if (bn ? !(S[1][2] instanceof Uint8Array && S[1][2].length === 32) : typeof S[1][2] !== "bigint") throw new Error(name + ": element type");
        const rows = new BigUint64Array(ew * N * nCols), rb = new Uint8Array(rows.buffer);
        for (let i = 0; i < N; i++) for (let j = 0; j < nCols; j++) { if (bn) rb.set(S[j][i], 32 * (i * nCols + j)); else rows[i * nCols + j] = S[j][i]; }
        same(name + " connectionPols", hexOf(rows), c.S);
        same(name + " connectionPols with w given", hexOf(rowsOf(W.connectionPols({ n8: F.n8, one: F.one, w: {} }, sMap, N, ks, { w }), bn, N, nCols)), c.S);
        // resident: prepareExec once, then the S columns without a host copy
        const exec = bn ? await W.readExecFile(null, c.exec, nCols) : await W.readExecFile(c.exec, nCols);
        const prep = W.prepareExec(exec, nCols, c.nW);
        const d = W.connectionPolsDev(prep, null, { N, ks, w, check: true });
        same(name + " connectionPolsDev", hexOf(d.toHost()), c.S);
        // into columns [2, 2 + nCols) of a wider matrix whose other columns keep their contents
        const stride = nCols + 3, wide = new m.DevBuffer(N * stride * ew);
        wide.set(new BigUint64Array(N * stride * ew).fill(0x1122334455667788n));
        W.connectionPolsDev(prep, wide, { N, ks, w, stride, offset: 2 });
        const got = wide.toHost(), want = new BigUint64Array(rows.buffer);
        for (let i = 0; i < N; i++) for (let j = 0; j < stride; j++) for (let k = 0; k < ew; k++) {
            const v = got[(i * stride + j) * ew + k], inside = j >= 2 && j < 2 + nCols;
            if (v !== (inside ? want[(i * nCols + j - 2) * ew + k] : 0x1122334455667788n)) throw new Error(name + ": wide matrix differs at row " + i + " column " + j);
        }
        d.free(); wide.free(); prep.free();
    }
    console.log("conn pols parity OK");
}
function rowsOf(S, bn, N, nCols) {
    const rows = new BigUint64Array((bn ? 4 : 1) * N * nCols), rb = new Uint8Array(rows.buffer);
    for (let i = 0; i < N; i++) for (let j = 0; j < nCols; j++) { if (bn) rb.set(S[j][i], 32 * (i * nCols + j)); else rows[i * nCols + j] = S[j][i]; }
    return rows;
}
main().then(() => process.exit(0), (e) => { console.error(e.stack || e); process.exit(1); });
