// js/witness_exec.js from Node: the files the Python test wrote (a compressor .exec, a final .exec, a .wtns) read with readExecFile /
// readWtns, the array drop-ins (compressorExec, finalExec) and the resident forms (prepareExec once, execDev per witness) for both
// fields, against the Python checker's trace bytes.
// usage: node wtns_exec_parity.js job.json; exits non-zero on the first difference.
"use strict";
const fs = require("fs");
const path = require("path");
const m = require(path.join(__dirname, "..", "..", "pil2-stark-js_amd", "js", "index.js"));
const W = m.witness_exec;

const bytes = (hex) => Uint8Array.from(Buffer.from(hex, "hex"));
const hexOf = (t) => Buffer.from(t.buffer, t.byteOffset, t.byteLength).toString("hex");
const wordsOf = (u8) => new BigUint64Array(u8.buffer.slice(u8.byteOffset, u8.byteOffset + u8.byteLength));
function same(what, got, want) { if (got !== want) throw new Error(what + " differs: " + String(got).slice(0, 200)); }
async function thrown(fn) { try { await fn(); } catch (e) { return e.message; } return null; }

async function main() {
    const job = JSON.parse(fs.readFileSync(process.argv[2], "utf8"));
    // Goldilocks: the compressor shape
    const g = job.gl;
    const exec = await W.readExecFile(g.exec, g.nCols);
    if (exec.nAdds !== g.nAdds || exec.nSMap !== g.nRows || !(exec.addsBuff instanceof BigUint64Array) || exec.sMapBuff.length !== g.nRows * g.nCols) throw new Error("readExecFile: compressor shape");
    const w = wordsOf(bytes(g.w));
    const pil = { references: { "Compressor.a": { polDeg: g.nRows, len: g.nCols } } };
    const cm = await W.compressorExec(null, pil, w, exec);
    same("compressorExec trace", hexOf(cm.trace), g.trace);
    if (cm.Compressor.a.length !== g.nCols || cm.Compressor.a[1][3] !== cm.trace[3 * g.nCols + 1]) throw new Error("compressorExec: cmPols shape");
    const prep = W.prepareExec(exec, g.nCols, g.nWitness);
    if (prep.nLevels !== g.nLevels) throw new Error("prepareExec: " + prep.nLevels + " levels, " + g.nLevels + " expected");
    const wDev = new m.DevBuffer(prep.nW); wDev.zero(); wDev.set(w);
    const dst = W.execDev(prep, wDev, null, { check: true });
    same("execDev trace", hexOf(dst.toHost()), g.trace);
    const wide = W.execDev(prep, wDev, null, { dstCols: g.nCols + 3 });
    same("execDev widened", hexOf(wide.toHost()), g.wide);
    dst.free(); wide.free(); wDev.free(); prep.free();
    const msg = await thrown(() => W.readExecFile(g.truncated, g.nCols));
    if (!msg || msg.indexOf(g.truncated) < 0 || msg.indexOf(g.truncatedMessage) < 0) throw new Error("truncated file: got " + JSON.stringify(msg));

    // BN254 Fr: the final shape, the witness from a .wtns
    const f = job.bn128;
    const fx = await W.readExecFile({}, f.exec, f.nCols);
    if (fx.nAdds !== f.nAdds || fx.nSMap !== f.nRows || fx.addsFr.byteLength !== 64 * f.nAdds) throw new Error("readExecFile: final shape");
    const wt = W.readWtns(f.wtns);
    if (wt.n8 !== 32 || wt.nWitness !== f.nWitness || wt.prime.toString() !== f.prime) throw new Error("readWtns: header");
    same("finalExec trace, Montgomery", hexOf(W.finalExec(wt.w, fx, f.nCols)), f.mont);
    same("finalExec trace, normal", hexOf(W.finalExec(wt.w, fx, f.nCols, { montgomery: false })), f.normal);
    const fp = W.prepareExec(fx, f.nCols, f.nWitness);
    const fw = new m.DevBuffer(4 * fp.nW); fw.zero(); fw.set(wordsOf(wt.w));
    const fd = W.execDev(fp, fw, null, { check: true });
    same("execDev trace, Montgomery", hexOf(fd.toHost()), f.mont);
    W.execDev(fp, fw, fd, { montgomery: false });
    same("execDev trace, normal", hexOf(fd.toHost()), f.normal);
    fd.free(); fw.free(); fp.free();
    console.log("wtns exec parity OK");
}
main().catch((e) => { console.error(e && e.stack || e); process.exit(1); });
