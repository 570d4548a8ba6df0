// Drop-in for src/helpers/fft/fft_p.bn128.js of pil2-stark-js: same exports, same signatures, the trailing Fr included
// (fft / ifft(buffSrc, nPols, nBits, buffDst, Fr), interpolate(buffSrc, nPols, nBits, buffDstCoefs, buffDst, nBitsExt, Fr) -> Promise<void>,
// fft_p.bn128.js:178-285), computed by libpil2gl on the MI355X instead of one JavaScript thread over the WASM field.
// Buffers hold 32 bytes per element, the Montgomery bytes ffjavascript's Fr keeps (Fr.n8 === 32 is all that is read of Fr).  A buffer is
//   a DevBuffer                      resident: nothing is staged;
//   a Uint8Array                     staged whole;
//   anything with ffjavascript BigBuffer's surface { byteLength, slice(a, b) -> Uint8Array, set(arr, off) }: staged in 256 MB pieces.
"use strict";
const { addon, isDev } = require("./native.js");

const CHUNK_BYTES = 1 << 28;

function checkFr(Fr) { if (!Fr || Fr.n8 !== 32) throw new Error("fft_p_bn128: expected the BN254 scalar field (Fr.n8 === 32)"); }

function asWords(u8) {       // a BigUint64Array over the same bytes where alignment allows, over a copy otherwise
    if (u8.byteOffset % 8 === 0) return new BigUint64Array(u8.buffer, u8.byteOffset, u8.byteLength / 8);
    const c = new Uint8Array(u8.byteLength); c.set(u8);
    return new BigUint64Array(c.buffer);
}
function uploadBytes(dptr, buf, nBytes) {
    for (let o = 0; o < nBytes; o += CHUNK_BYTES) {
        const e = Math.min(nBytes, o + CHUNK_BYTES);
        addon.devUpload(dptr, o / 8, asWords(buf instanceof Uint8Array ? buf.subarray(o, e) : buf.slice(o, e)));
    }
}
function downloadBytes(buf, dptr, nBytes) {
    for (let o = 0; o < nBytes; o += CHUNK_BYTES) {
        const tmp = new BigUint64Array((Math.min(nBytes, o + CHUNK_BYTES) - o) / 8);
        addon.devDownload(tmp, dptr, o / 8);
        buf.set(new Uint8Array(tmp.buffer), o);
    }
}
function checkBytes(buf, nBytes, what) {
    const have = isDev(buf) ? buf.length * 8 : buf.byteLength;
    if (!(have >= nBytes)) throw new Error("fft_p_bn128: " + what + " holds " + have + " bytes, needs " + nBytes);
}

// run fn(dIn, dOuts) on device copies: ins / outs are { buf, bytes }; a DevBuffer stands for itself, a null output stays null
function onDevice(inp, outs, fn) {
    const owned = [];
    const alloc = (bytes) => { const p = addon.devAlloc(Math.max(1, bytes / 8)); owned.push(p); return p; };
    try {
        let dIn;
        if (isDev(inp.buf)) dIn = inp.buf.ptr; else { dIn = alloc(inp.bytes); uploadBytes(dIn, inp.buf, inp.bytes); }
        const dOuts = outs.map((o) => (o.buf === null || o.buf === undefined) ? null : (o.buf === inp.buf ? dIn : isDev(o.buf) ? o.buf.ptr : alloc(o.bytes)));
        fn(dIn, dOuts);
        outs.forEach((o, i) => { if (dOuts[i] !== null && !isDev(o.buf)) downloadBytes(o.buf, dOuts[i], o.bytes); });
    } finally {
        for (const p of owned) addon.devFree(p);
    }
}

async function transform(inverse, buffSrc, nPols, nBits, buffDst, Fr) {
    checkFr(Fr);
    const bytes = nPols * 2 ** nBits * 32;
    checkBytes(buffSrc, bytes, "buffSrc"); checkBytes(buffDst, bytes, "buffDst");
    onDevice({ buf: buffSrc, bytes }, [{ buf: buffDst, bytes }],
        (dIn, [dOut]) => (inverse ? addon.bn128IfftDev : addon.bn128FftDev)(dIn, nPols, nBits, dOut));
}
async function fft(buffSrc, nPols, nBits, buffDst, Fr) { return transform(false, buffSrc, nPols, nBits, buffDst, Fr); }
async function ifft(buffSrc, nPols, nBits, buffDst, Fr) { return transform(true, buffSrc, nPols, nBits, buffDst, Fr); }

async function interpolate(buffSrc, nPols, nBits, buffDstCoefs, buffDst, nBitsExt, Fr) {
    checkFr(Fr);
    const nIn = nPols * 2 ** nBits * 32, nOut = nPols * 2 ** nBitsExt * 32;
    checkBytes(buffSrc, nIn, "buffSrc"); checkBytes(buffDst, nOut, "buffDst");
    if (buffDstCoefs) checkBytes(buffDstCoefs, nIn, "buffDstCoefs");
    onDevice({ buf: buffSrc, bytes: nIn }, [{ buf: buffDstCoefs || null, bytes: nIn }, { buf: buffDst, bytes: nOut }],
        (dIn, [dCoefs, dOut]) => addon.bn128InterpolateDev(dIn, nPols, nBits, dCoefs, dOut, nBitsExt));
}

module.exports.fft = fft;
module.exports.ifft = ifft;
module.exports.interpolate = interpolate;
