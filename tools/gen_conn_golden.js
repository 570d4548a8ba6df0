// Writes tests/golden/conn_pols.json by RUNNING the reference's own pieces of the setups' S loops: `connect` of src/helpers/polutils.js:166
// and F.w, F.k, F.mul of src/helpers/f3g.js, in the loop of src/compressor/compressor12_setup.js:470-500.  getKs is pilcom's and is not
// part of the reference tree, so ks[i] = k^(i + 1) is formed here and recorded.  Numbers only, as decimal strings.
//   PIL2_REFERENCE=<reference checkout> node tools/gen_conn_golden.js
"use strict";
const fs = require("fs");
const path = require("path");
const ref = process.env.PIL2_REFERENCE || process.argv[2];
if (!ref) { console.error("set PIL2_REFERENCE to the reference checkout"); process.exit(2); }
const F3g = require(path.join(ref, "src/helpers/f3g.js"));
const { connect } = require(path.join(ref, "src/helpers/polutils.js"));
const F = new F3g();

function run(name, nBits, nCols, r, cell) {
    const N = 1 << nBits;
    const sMap = [];
    for (let j = 0; j < nCols; j++) { sMap[j] = new Uint32Array(N); for (let i = 0; i < r; i++) sMap[j][i] = cell(i, j); }
    const ks = [];
    for (let i = 0, k = F.k; i < nCols - 1; i++, k = F.mul(k, F.k)) ks.push(k);
    const S = [];
    for (let j = 0; j < nCols; j++) S[j] = new Array(N);
    // compressor12_setup.js:470-500
    let w = F.one;
    for (let i = 0; i < N; i++) {
        S[0][i] = w;
        for (let j = 1; j < nCols; j++) S[j][i] = F.mul(w, ks[j - 1]);
        w = F.mul(w, F.w[nBits]);
    }
    const lastSignal = {};
    for (let i = 0; i < r; i++) {
        for (let j = 0; j < nCols; j++) {
            if (sMap[j][i]) {
                if (typeof lastSignal[sMap[j][i]] !== "undefined") {
                    const ls = lastSignal[sMap[j][i]];
                    connect(S[ls.col], ls.row, S[j], i);
                } else {
                    lastSignal[sMap[j][i]] = { col: j, row: i };
                }
            }
        }
    }
    return { name, nBits, nCols, nRows: r, w: F.w[nBits].toString(), ks: ks.map(String), sMap: sMap.map((c) => Array.from(c.subarray(0, r))), S: S.map((c) => c.map(String)) };
}

// 2^3 rows x 3 columns: zeros, a singleton (9), signal 1 in every cell of row 2, signals 2 and 3 spread over rows and columns
const small = [[1, 2, 0], [2, 0, 3], [1, 1, 1], [0, 9, 2], [3, 3, 1], [0, 0, 0]];
// 2^5 rows x 12 columns: five signals from a fixed recurrence, zeros, a singleton (77), signal 4 in every cell of row 7, rows 27.. beyond the table
function wide(i, j) {
    if (i === 7) return 4;
    if (i === 3 && j === 5) return 77;
    const v = (i * 31 + j * 17 + ((i * j) % 7)) % 9;
    return v < 6 ? v : 0;
}
const out = { source: "polutils.js connect, f3g.js F.w F.k F.mul; loop of compressor12_setup.js:470-500; ks[i] = k^(i+1)", k: F.k.toString(),
    cases: [run("8x3", 3, 3, small.length, (i, j) => small[i][j]), run("32x12", 5, 12, 27, wide)] };
const file = path.join(__dirname, "..", "tests", "golden", "conn_pols.json");
fs.writeFileSync(file, JSON.stringify(out) + "\n");
console.log("wrote " + file + " (" + fs.statSync(file).size + " bytes)");
