// Byte staging for the BN254 drop-ins (fft_p_bn128, g1_msm, polynomial_bn128, polutils_bn128): the one place where a host buffer of
// 32-byte elements becomes a device copy and comes back.  A host buffer is a Uint8Array or anything with ffjavascript BigBuffer's surface
// { byteLength, slice(a, b) -> Uint8Array, set(u8, byteOffset) }; it crosses in pieces of pieceBytes (2^28 = 256 MB unless a test lowers
// it).  A DevBuffer is resident and is never staged.
//   createStage({ devAlloc, devFree, devUpload, devDownload }, isDev) -> { byteLength, uploadBytes, downloadBytes, scope, input, output,
//              inout, asWords }: the staging calls over those four memory calls, so a test can drive them without the addon
//   native()   that stage over the addon of native.js, made once (this module itself loads without the addon)
//   scope(bufs, fn)   bufs = [input | output | inout (buf, bytes)]; fn([device address per entry]); returns what fn returns
//     kernels read   kernels write   DevBuffer         host buffer
//     yes            no              its own address   allocated, uploaded                      input
//     no             yes             its own address   allocated, downloaded after fn           output
//     yes            yes             its own address   allocated, uploaded, downloaded after fn inout
//   One host object named by several entries is one device copy of the largest byte count, read / written if any entry is.  A null or
//   undefined buf yields null.  Zero bytes yield an allocation of one word and no copies.  Everything allocated is freed when scope
//   returns or throws; nothing is downloaded after a throw.
"use strict";

const CHUNK_BYTES = 1 << 28;                                 // the default piece: 256 MB
let pieceBytes = CHUNK_BYTES;
// tests lower the piece size to cross piece boundaries with small buffers; returns the size it replaces
function setPieceBytes(n) {
    if (!Number.isInteger(n) || n < 32 || n % 32) throw new Error("bn128_stage: the piece size must be a positive multiple of 32 bytes");
    const was = pieceBytes;
    pieceBytes = n;
    return was;
}

function asWords(u8) {       // a BigUint64Array over the same bytes where alignment allows, over a copy otherwise
    if (u8.byteOffset % 8 === 0) return new BigUint64Array(u8.buffer, u8.byteOffset, u8.byteLength / 8);
    const c = new Uint8Array(u8.byteLength); c.set(u8);
    return new BigUint64Array(c.buffer);
}
const input = (buf, bytes) => ({ buf, bytes, read: true, write: false });
const output = (buf, bytes) => ({ buf, bytes, read: false, write: true });
const inout = (buf, bytes) => ({ buf, bytes, read: true, write: true });

function createStage(dev, isDev) {
    function byteLength(buf) { return isDev(buf) ? buf.length * 8 : buf.byteLength; }
    function uploadBytes(dptr, buf, nBytes) {
        for (let o = 0; o < nBytes; o += pieceBytes) {
            const e = Math.min(nBytes, o + pieceBytes);
            dev.devUpload(dptr, o / 8, asWords(buf instanceof Uint8Array ? buf.subarray(o, e) : buf.slice(o, e)));
        }
    }
    function downloadBytes(buf, dptr, nBytes) {
        for (let o = 0; o < nBytes; o += pieceBytes) {
            const tmp = new BigUint64Array((Math.min(nBytes, o + pieceBytes) - o) / 8);
            dev.devDownload(tmp, dptr, o / 8);               // a synchronous copy: ordered after the kernels
            buf.set(new Uint8Array(tmp.buffer), o);
        }
    }
    function scope(bufs, fn) {
        const copies = new Map();                            // host object -> { ptr, bytes, read, write }
        const absent = (b) => b.buf === null || b.buf === undefined;
        for (const b of bufs) {
            if (absent(b) || isDev(b.buf)) continue;
            const c = copies.get(b.buf) || { bytes: 0, read: false, write: false };
            copies.set(b.buf, { ptr: null, bytes: Math.max(c.bytes, b.bytes), read: c.read || b.read, write: c.write || b.write });
        }
        try {
            for (const c of copies.values()) c.ptr = dev.devAlloc(Math.max(1, c.bytes / 8));
            for (const [buf, c] of copies) if (c.read) uploadBytes(c.ptr, buf, c.bytes);
            const res = fn(bufs.map((b) => absent(b) ? null : isDev(b.buf) ? b.buf.ptr : copies.get(b.buf).ptr));
            for (const [buf, c] of copies) if (c.write) downloadBytes(buf, c.ptr, c.bytes);
            return res;
        } finally {
            for (const c of copies.values()) if (c.ptr !== null) dev.devFree(c.ptr);
        }
    }
    return { byteLength, uploadBytes, downloadBytes, scope, input, output, inout, asWords };
}

let bound = null;
function native() {
    if (!bound) { const { addon, isDev } = require("./native.js"); bound = createStage(addon, isDev); }
    return bound;
}

module.exports = { createStage, native, setPieceBytes, asWords, input, output, inout };
