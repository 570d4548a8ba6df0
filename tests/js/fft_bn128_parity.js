// The BN254 Fr drop-in (pil2-stark-js_amd/js/fft_p_bn128.js) against expected bytes a Python checker wrote: every case of the job runs
// over a Uint8Array, over a chunked object with ffjavascript BigBuffer's surface (4096-byte chunks: staging crosses them) and over
// DevBuffers.  Then staging in several pieces: 3 columns of 64 rows (6144 bytes) with the piece size lowered to 1024 bytes give the bytes
// the same calls give in one piece.  usage: node fft_bn128_parity.js <job.json>; exits non-zero on the first difference.
"use strict";
const fs = require("fs");
const path = require("path");
const m = require(path.join(__dirname, "..", "..", "pil2-stark-js_amd", "js", "index.js"));
const { fft, ifft, interpolate } = m.fft_p_bn128;
const stage = require(path.join(__dirname, "..", "..", "pil2-stark-js_amd", "js", "bn128_stage.js"));
const Fr = { n8: 32 };

class Chunked {              // { byteLength, slice(a, b) -> Uint8Array, set(arr, off) } over 4096-byte pieces
    constructor(nBytes) { this.byteLength = nBytes; this.chunks = []; for (let o = 0; o < nBytes; o += 4096) this.chunks.push(new Uint8Array(Math.min(4096, nBytes - o))); }
    slice(a = 0, b = this.byteLength) {
        const out = new Uint8Array(Math.max(0, b - a));
        for (let o = a; o < b;) { const k = Math.floor(o / 4096), at = o % 4096, n = Math.min(b - o, 4096 - at); out.set(this.chunks[k].subarray(at, at + n), o - a); o += n; }
        return out;
    }
    set(arr, off = 0) {
        for (let o = 0; o < arr.length;) { const k = Math.floor((off + o) / 4096), at = (off + o) % 4096, n = Math.min(arr.length - o, 4096 - at); this.chunks[k].set(arr.subarray(o, o + n), at); o += n; }
    }
    static from(u8) { const c = new Chunked(u8.length); c.set(u8, 0); return c; }
}
const kinds = {
    flat: { make: (u8) => Uint8Array.from(u8), empty: (n) => new Uint8Array(n), bytes: (b) => b, free: () => {} },
    chunked: { make: (u8) => Chunked.from(u8), empty: (n) => new Chunked(n), bytes: (b) => b.slice(0, b.byteLength), free: () => {} },
    dev: { make: (u8) => m.DevBuffer.from(new BigUint64Array(Uint8Array.from(u8).buffer)), empty: (n) => new m.DevBuffer(n / 8),
        bytes: (b) => new Uint8Array(b.toHost().buffer), free: (b) => b.free() },
};
function check(what, got, wantHex) {
    const want = Buffer.from(wantHex, "hex");
    if (got.length !== want.length) throw new Error(what + ": " + got.length + " bytes, expected " + want.length);
    for (let i = 0; i < want.length; i++) if (got[i] !== want[i]) throw new Error(what + ": byte " + i + " (element " + Math.floor(i / 32) + ") differs");
}

// fft out of place and in place (buffDst === buffSrc), interpolate with buffDstCoefs given, over Uint8Arrays -> every buffer the calls touch
async function stagedRuns(input, nPols, nBits, nBitsExt) {
    const src = Uint8Array.from(input), dst = new Uint8Array(input.length), inPlace = Uint8Array.from(input);
    const coefs = new Uint8Array(input.length), ext = new Uint8Array(nPols * 2 ** nBitsExt * 32);
    await fft(src, nPols, nBits, dst, Fr);
    await fft(inPlace, nPols, nBits, inPlace, Fr);
    await interpolate(src, nPols, nBits, coefs, ext, nBitsExt, Fr);
    return { src, dst, inPlace, coefs, ext };
}
async function piecewise(job) {
    const nPols = 3, nBits = 6, bytes = nPols * 2 ** nBits * 32;
    const input = Buffer.from(job.cases[job.cases.length - 1].input, "hex").subarray(0, bytes);       // any run of field elements serves
    if (input.length !== bytes) throw new Error("the last case holds fewer than " + bytes + " bytes");
    const one = await stagedRuns(input, nPols, nBits, nBits + 1);
    const was = stage.setPieceBytes(1024);
    let many;
    try { many = await stagedRuns(input, nPols, nBits, nBits + 1); } finally { stage.setPieceBytes(was); }
    for (const k of Object.keys(one)) check("1024-byte pieces: " + k, many[k], Buffer.from(one[k]).toString("hex"));
    check("1024-byte pieces: in place and out of place agree", many.inPlace, Buffer.from(one.dst).toString("hex"));
    check("1024-byte pieces: source untouched", many.src, Buffer.from(input).toString("hex"));
}

async function main() {
    const job = JSON.parse(fs.readFileSync(process.argv[2], "utf8"));
    let n = 0;
    for (const c of job.cases) {
        const input = Buffer.from(c.input, "hex");
        for (const [kind, K] of Object.entries(kinds)) {
            const what = c.op + " (" + c.nBits + ", " + c.nPols + ") " + kind;
            const src = K.make(input);
            if (c.op === "interpolate") {
                const coefs = K.empty(input.length), dst = K.empty(c.nPols * 2 ** c.nBitsExt * 32);
                await interpolate(src, c.nPols, c.nBits, coefs, dst, c.nBitsExt, Fr);
                check(what + " coefs", K.bytes(coefs), c.coefs); check(what + " dst", K.bytes(dst), c.expected);
                const dst2 = K.empty(c.nPols * 2 ** c.nBitsExt * 32);
                await interpolate(src, c.nPols, c.nBits, null, dst2, c.nBitsExt, Fr);
                check(what + " dst without coefs", K.bytes(dst2), c.expected);
                K.free(coefs); K.free(dst); K.free(dst2);
            } else {
                const dst = K.empty(input.length);
                await (c.op === "fft" ? fft : ifft)(src, c.nPols, c.nBits, dst, Fr);
                check(what, K.bytes(dst), c.expected);
                check(what + " (source untouched)", K.bytes(src), c.input);
                await (c.op === "fft" ? fft : ifft)(src, c.nPols, c.nBits, src, Fr);      // in place
                check(what + " in place", K.bytes(src), c.expected);
                K.free(dst);
            }
            K.free(src);
            n++;
        }
    }
    await piecewise(job);
    let threw = false;
    try { await fft(new Uint8Array(64), 1, 1, new Uint8Array(64), { n8: 8 }); } catch (e) { threw = true; }
    if (!threw) throw new Error("a field with n8 != 32 was accepted");
    console.log("fft bn128 parity OK (" + n + " runs)");
}
main().catch((e) => { console.error(e && e.stack || e); process.exit(1); });
