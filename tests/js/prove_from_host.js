// Proofs DRIVEN FROM NODE whose witness starts in HOST memory, as the reference's does (witnessCalculator.js:145-214, prover.js:24):
// the stage order of tests/js/prove_flow.js over the JS drop-in modules, the witness in a PinnedBuffer -- read there from a `.commit`
// file, or downloaded from the job's generator -- and proofs back to back over two device witness buffers: while proof k runs on
// the NULL stream, witness k + 1 goes up on the library's copy stream (copyAfter: not before proof k - 1 has let go of that buffer;
// copyFence: proof k + 1 not before the upload is done).  Two witnesses alternate, so a proof that read a stale or half-uploaded
// buffer cannot have the digest the caller expects for it.
//   node tests/js/prove_from_host.js job.json
// job: { pilInfo, expressionsInfo, constRoot, witnesses: [{ start, publics, queries }, x2], proofs, commitDir | null }
"use strict";
const fs = require("fs");
const path = require("path");
const crypto = require("crypto");
const root = path.join(__dirname, "..", "..");
const { prove, freeCtx } = require("./prove_flow.js");
const { addon, DevBuffer, PinnedBuffer, copyAfter, copyFence, copySync } = require(path.join(root, "pil2-stark-js_amd/js/native.js"));

function canon(v) {
    if (Array.isArray(v)) return "[" + v.map(canon).join(",") + "]";
    if (v && typeof v === "object") return "{" + Object.keys(v).map((k) => '"' + k + '":' + canon(v[k])).join(",") + "}";
    return '"' + BigInt(v).toString() + '"';
}
const now = () => Number(process.hrtime.bigint()) / 1e9;
const median = (a) => { const s = a.slice().sort((x, y) => x - y); return s.length % 2 ? s[(s.length - 1) / 2] : (s[s.length / 2 - 1] + s[s.length / 2]) / 2; };

(async () => {
    const g = JSON.parse(fs.readFileSync(process.argv[2]));
    const nBits = g.pilInfo.starkStruct.nBits, N = 2 ** nBits, cols = g.witnesses[0].start.length, K = cols / 2, nWords = N * cols;
    const consts = new BigUint64Array(N * 2); consts[0] = 1n; consts[(N - 1) * 2 + 1] = 1n;
    const dConsts = DevBuffer.from(consts);

    // the two witnesses (K Fibonacci machines, sm_fibonacci.js:12-23) into pinned host memory
    const pinned = [];
    for (let w = 0; w < 2; w++) {
        const gen = new DevBuffer(nWords), pb = new PinnedBuffer(nWords, undefined, false);
        addon.synthFibonacciDev(nBits, K, BigUint64Array.from(g.witnesses[w].start, BigInt), gen.ptr);
        if (g.commitDir) {          // through a `.commit` file: written from HBM, read by Node into the pinned chunks
            const f = path.join(g.commitDir, "witness" + w + ".commit");
            gen.toFile(f);
            const fd = fs.openSync(f, "r");
            let pos = 0;
            for (const c of pb.chunks) {
                const b8 = new Uint8Array(c.buffer, c.byteOffset, c.byteLength);
                for (let o = 0; o < b8.length;) { const got = fs.readSync(fd, b8, o, Math.min(1 << 28, b8.length - o), pos + o); if (got <= 0) throw new Error(f + " is short"); o += got; }
                pos += b8.length;
            }
            fs.closeSync(fd);
        } else {
            copyAfter(); gen.downloadAsync(pb); copySync();
        }
        gen.free();
        pinned.push(pb);
    }
    const B = [new DevBuffer(nWords), new DevBuffer(nWords)];
    const GB = nWords * 8 / 1e9;

    // host -> HBM rates, alone on the device: pinned asynchronous; the same followed by the landing pass (check of every word); pageable
    // pil2gl_dev_upload of the same bytes (one typed array's worth at a time through a pageable copy of each pinned chunk)
    const timed = (fn) => { addon.sync(); copySync(); const t0 = now(); fn(); return now() - t0; };
    const tPinned = median([0, 1, 2].map(() => timed(() => { B[0].uploadAsync(pinned[0]); copySync(); })));
    let firstBad;
    const tLanded = median([0, 1, 2].map(() => timed(() => { B[0].uploadAsync(pinned[0]); copyFence(); firstBad = addon.landRowsDev(B[0].ptr, cols, B[0].ptr, cols, N, true); })));
    if (firstBad !== 0xFFFFFFFFFFFFFFFFn) throw new Error("the witness has a non-canonical word at " + firstBad);
    let tPageable = 0;
    {
        let o = 0;
        for (const c of pinned[0].chunks) { const pageable = new BigUint64Array(c); tPageable += timed(() => addon.devUpload(B[1].ptr, o, pageable)); o += c.length; }
    }

    const jobFor = (k, cm1) => { const w = g.witnesses[k % 2]; return { pilInfo: g.pilInfo, expressionsInfo: g.expressionsInfo, cm1, consts: dConsts, publics: w.publics, constRoot: g.constRoot, queries: w.queries }; };
    const keep = [B[0], B[1], dConsts];
    const digests = [], walls = [], inner = [];
    // the same proof from a witness already in HBM (B[0] holds witness 0): one run to warm up (kernel compilation, scratch), then three
    const resident = [], residentInner = [];
    for (let it = 0; it < 4; it++) {
        addon.sync(); const t0 = now();
        const res = await prove(jobFor(0, B[0]), true);
        if (it) { resident.push(now() - t0); residentInner.push(res.seconds); }
        freeCtx(res.ctx, keep);
    }
    // prove() builds its tables and allocates before it starts its clock (the addon.sync() in front of tStart, tests/js/prove_flow.js);
    // the next upload is enqueued AT that point, so that it runs under the timed proof and not under the untimed preparation
    const realSync = addon.sync;
    let atProofStart = null, tHook = 0;
    addon.sync = function () { realSync(); if (atProofStart) { const f = atProofStart; atProofStart = null; f(); tHook = now(); } };
    // first proof from the host: upload, then proof, nothing under anything
    const tUploadFirst = timed(() => { copyAfter(); B[0].uploadAsync(pinned[0]); copySync(); });
    for (let k = 0; k < g.proofs; k++) {
        const t0 = now();
        copyFence();                                                                                 // proof k starts behind upload k
        atProofStart = () => { copyAfter(); B[(k + 1) & 1].uploadAsync(pinned[(k + 1) % 2]); };   // upload k + 1 behind proof k - 1, which read that buffer (the last proof has one under it too)
        const res = await prove(jobFor(k, B[k & 1]), true);
        const tEnd = now();
        // the hook must have fired right in front of prove()'s clock: from the hook to prove()'s return is the timed proof and nothing else.
        // (Were a sync added earlier in prove(), the upload would run under the preparation and the comparison below would mean nothing.)
        if (atProofStart !== null) throw new Error("prove() never reached the sync in front of its clock");
        const gap = (tEnd - tHook) - res.seconds;
        if (!(gap > -1e-3 && gap < 0.005 + 0.02 * res.seconds)) throw new Error("the upload was not enqueued at the start of the timed proof: " + gap + " s between the hook and prove()'s clock");
        walls.push(tEnd - t0); inner.push(res.seconds);
        digests.push(crypto.createHash("sha256").update(canon(res.proof)).digest("hex"));
        freeCtx(res.ctx, keep);
    }
    addon.sync = realSync;
    copySync();
    // seconds are prove()'s own clock (what tests/js/prove_c3.js reports); *_wall_seconds add its preparation (tables, ~200 GB of allocations at config 3)
    const line = {
        config: "2^" + nBits + " x " + cols + ", blow-up 8, Node-driven, witness from " + (g.commitDir ? "a .commit file through " : "") + "pinned host memory",
        proofSha256: digests,
        first_proof_seconds: tUploadFirst + inner[0],
        steady_seconds: median(inner.slice(1)), resident_seconds: median(residentInner),
        steady_wall_seconds: median(walls.slice(1)), resident_wall_seconds: median(resident),
        h2d_GBps: GB / tPinned, h2d_landed_GBps: GB / tLanded, h2d_pageable_GBps: GB / tPageable,
        witness_GB: GB, proof_seconds: inner,
    };
    console.log(JSON.stringify(line));
    for (const b of [...B, dConsts]) b.free();
    for (const p of pinned) p.free();
    console.log("prove from host OK");
})().catch((e) => { console.error(e); process.exit(1); });
