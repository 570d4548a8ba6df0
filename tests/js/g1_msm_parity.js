// multiExpAffine (pil2-stark-js_amd/js/g1_msm.js) against expected bytes a Python checker wrote: every case of the job runs over
// Uint8Arrays and over DevBuffers.  Then staging in several pieces: 40 points at stride 2, the scalars a view at byteOffset 4, in 1024-byte
// pieces give the point the same call gives in one piece.  usage: node g1_msm_parity.js <job.json>; exits non-zero on the first difference.
"use strict";
const fs = require("fs");
const path = require("path");
const m = require(path.join(__dirname, "..", "..", "pil2-stark-js_amd", "js", "index.js"));
const { multiExpAffine } = m.g1_msm;
const stage = require(path.join(__dirname, "..", "..", "pil2-stark-js_amd", "js", "bn128_stage.js"));

function check(what, got, wantHex) {
    const want = Buffer.from(wantHex, "hex");
    if (!(got instanceof Uint8Array) || got.length !== 64) throw new Error(what + ": expected a Uint8Array of 64 bytes");
    for (let i = 0; i < 64; i++) if (got[i] !== want[i]) throw new Error(what + ": byte " + i + " differs");
}
const toDev = (u8) => m.DevBuffer.from(new BigUint64Array(Uint8Array.from(u8).buffer));

async function main() {
    const job = JSON.parse(fs.readFileSync(process.argv[2], "utf8"));
    let n = 0;
    for (const c of job.cases) {
        const bases = Uint8Array.from(Buffer.from(c.bases, "hex")), scalars = Uint8Array.from(Buffer.from(c.scalars, "hex"));
        const opts = { stride: c.stride, montgomery: c.montgomery, n: c.n };
        const what = "n = " + c.n + ", stride " + c.stride + (c.montgomery ? "" : ", normal form");
        check(what + " Uint8Array", await multiExpAffine(bases, scalars, opts), c.expected);
        const dB = toDev(bases), dS = toDev(scalars);
        check(what + " DevBuffer", await multiExpAffine(dB, dS, opts), c.expected);
        check(what + " mixed", await multiExpAffine(dB, scalars, opts), c.expected);
        dB.free(); dS.free();
        n += 3;
    }
    const first = job.cases[0];
    if (first.stride === 1 && first.montgomery)          // the defaults: stride 1, Montgomery scalars, n from the bases
        check("defaults", await multiExpAffine(Uint8Array.from(Buffer.from(first.bases, "hex")), Uint8Array.from(Buffer.from(first.scalars, "hex"))), first.expected);
    {
        const c = job.cases.find((x) => x.stride === 2 && x.montgomery), opts = { n: 40, stride: 2, montgomery: true };
        const bases = Uint8Array.from(Buffer.from(c.bases, "hex")).subarray(0, 40 * 64), scalars = Uint8Array.from(Buffer.from(c.scalars, "hex")).subarray(0, (39 * 2 + 1) * 32);
        const one = await multiExpAffine(bases, scalars, opts);
        const parent = new Uint8Array(4 + scalars.length), view = parent.subarray(4);
        view.set(scalars);
        if (view.byteOffset % 8 === 0) throw new Error("the view is aligned");
        const was = stage.setPieceBytes(1024);
        let many;
        try { many = await multiExpAffine(bases, view, opts); } finally { stage.setPieceBytes(was); }
        check("1024-byte pieces, scalars at byteOffset 4", many, Buffer.from(one).toString("hex"));
        check("one piece, scalars at byteOffset 4", await multiExpAffine(bases, view, opts), Buffer.from(one).toString("hex"));
    }
    let threw = false;
    try { await multiExpAffine(new Uint8Array(128), new Uint8Array(32)); } catch (e) { threw = true; }
    if (!threw) throw new Error("too few scalar bytes were accepted");
    console.log("g1 msm parity OK (" + n + " runs)");
}
main().catch((e) => { console.error(e && e.stack || e); process.exit(1); });
