// js/witness_exec.js from Node: checkConnections on host matrices (flat and in the cmPols shape [nCols][N]) and checkConnectionsDev on
// resident columns of a wider matrix, against what the Python checker says: null for a clean trace, the failing cell and the message
// for an altered one.  usage: node conn_check_parity.js job.json; exits non-zero on the first difference.
"use strict";
const fs = require("fs");
const path = require("path");
const m = require(path.join(__dirname, "..", "..", "pil2-stark-js_amd", "js", "index.js"));
const W = m.witness_exec;

const bytes = (hex) => Uint8Array.from(Buffer.from(hex, "hex"));
function same(what, got, want) { if (JSON.stringify(got) !== JSON.stringify(want)) throw new Error(what + ": got " + JSON.stringify(got) + ", expected " + JSON.stringify(want)); }
const plain = (r) => r === null ? null : { row: r.row, col: r.col, toRow: r.toRow, toCol: r.toCol, kind: r.kind, message: r.message() };

function main() {
    const job = JSON.parse(fs.readFileSync(process.argv[2], "utf8"));
    for (const c of job.cases) {
        const bn = c.field === "bn128", ew = bn ? 4 : 1, N = c.N, nCols = c.nCols;
        const elem = (x) => bn ? bytes(x) : BigInt(x);
        const w = elem(c.w), ks = c.ks.map(elem);
        const F = { n8: bn ? 32 : 8, one: elem(c.one), w: { [Math.log2(N)]: w } };
        const S = new BigUint64Array(bytes(c.S).buffer);
        for (const t of c.traces) {
            const a = new BigUint64Array(bytes(t.a).buffer);
            same(c.name + " checkConnections, flat words", plain(W.checkConnections(F, a, S, N, ks)), t.want);
            same(c.name + " checkConnections, flat bytes, w given", plain(W.checkConnections({ n8: F.n8, one: F.one, w: {} }, new Uint8Array(a.buffer), new Uint8Array(S.buffer), N, ks, { w })), t.want);
            const cols = (x) => Array.from({ length: nCols }, (_, j) => Array.from({ length: N }, (_, i) =>
                bn ? new Uint8Array(x.buffer, 32 * (i * nCols + j), 32) : x[i * nCols + j]));
            same(c.name + " checkConnections, [nCols][N]", plain(W.checkConnections(F, cols(a), cols(S), N, ks)), t.want);
            // resident: a in columns [1, 1 + nCols) and S in [2 + nCols, 2 + 2 nCols) of one matrix 3 + 2 nCols elements wide
            const stride = 3 + 2 * nCols, host = new BigUint64Array(N * stride * ew).fill(0x1122334455667788n);
            for (let i = 0; i < N; i++) {
                host.set(a.subarray(i * nCols * ew, (i + 1) * nCols * ew), (i * stride + 1) * ew);
                host.set(S.subarray(i * nCols * ew, (i + 1) * nCols * ew), (i * stride + 2 + nCols) * ew);
            }
            const d = m.DevBuffer.from(host);
            same(c.name + " checkConnectionsDev", plain(W.checkConnectionsDev({ buf: d, stride, offset: 1 }, { buf: d, stride, offset: 2 + nCols }, { N, ks, w })), t.want);
            d.free();
        }
    }
    console.log("conn check parity OK");
}
try { main(); process.exit(0); } catch (e) { console.error(e.stack || e); process.exit(1); }
