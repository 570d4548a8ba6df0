// Drop-in for src/helpers/fft/fft_p.bn128.js of pil2-stark-js: same exports, same signatures, the trailing Fr included
// (fft / ifft(buffSrc, nPols, nBits, buffDst, Fr), interpolate(buffSrc, nPols, nBits, buffDstCoefs, buffDst, nBitsExt, Fr) -> Promise<void>,
// fft_p.bn128.js:178-285), computed by libpil2gl on the MI355X instead of one JavaScript thread over the WASM field.
// Buffers hold 32 bytes per element, the Montgomery bytes ffjavascript's Fr keeps (Fr.n8 === 32 is all that is read of Fr).  A buffer is
//   a DevBuffer                      resident: nothing is staged;
//   a Uint8Array                     staged whole;
//   anything with ffjavascript BigBuffer's surface { byteLength, slice(a, b) -> Uint8Array, set(arr, off) }: staged in 256 MB pieces.
"use strict";
const { addon } = require("./native.js");
const { byteLength, scope, input, output } = require("./bn128_stage.js").native();

function checkFr(Fr) { if (!Fr || Fr.n8 !== 32) throw new Error("fft_p_bn128: expected the BN254 scalar field (Fr.n8 === 32)"); }
function checkBytes(buf, nBytes, what) {
    const have = byteLength(buf);
    if (!(have >= nBytes)) throw new Error("fft_p_bn128: " + what + " holds " + have + " bytes, needs " + nBytes);
}

async function transform(inverse, buffSrc, nPols, nBits, buffDst, Fr) {
    checkFr(Fr);
    const bytes = nPols * 2 ** nBits * 32;
    checkBytes(buffSrc, bytes, "buffSrc"); checkBytes(buffDst, bytes, "buffDst");
    scope([input(buffSrc, bytes), output(buffDst, bytes)],
        ([dIn, dOut]) => (inverse ? addon.bn128IfftDev : addon.bn128FftDev)(dIn, nPols, nBits, dOut));
}
async function fft(buffSrc, nPols, nBits, buffDst, Fr) { return transform(false, buffSrc, nPols, nBits, buffDst, Fr); }
async function ifft(buffSrc, nPols, nBits, buffDst, Fr) { return transform(true, buffSrc, nPols, nBits, buffDst, Fr); }

async function interpolate(buffSrc, nPols, nBits, buffDstCoefs, buffDst, nBitsExt, Fr) {
    checkFr(Fr);
    const nIn = nPols * 2 ** nBits * 32, nOut = nPols * 2 ** nBitsExt * 32;
    checkBytes(buffSrc, nIn, "buffSrc"); checkBytes(buffDst, nOut, "buffDst");
    if (buffDstCoefs) checkBytes(buffDstCoefs, nIn, "buffDstCoefs");
    scope([input(buffSrc, nIn), output(buffDstCoefs || null, nIn), output(buffDst, nOut)],
        ([dIn, dCoefs, dOut]) => addon.bn128InterpolateDev(dIn, nPols, nBits, dCoefs, dOut, nBitsExt));
}

module.exports.fft = fft;
module.exports.ifft = ifft;
module.exports.interpolate = interpolate;
