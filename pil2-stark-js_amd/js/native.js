// Loads the N-API addon (../addon/pil2gl.node -> ../lib/libpil2gl.so).  No fallback: if the addon is
// not built or no MI355X is present, requiring this module / calling into it throws.
"use strict";
const path = require("path");
const addon = require(path.join(__dirname, "..", "addon", "pil2gl.node"));

const CHUNK = 1 << 24;          // words per staging transfer for chunked containers (pilcom BigBuffer)

function isFlat(b) { return b instanceof BigUint64Array; }

// A BigBuffer-shaped container that lives in HBM: hand one of these to any of the drop-in modules (as ctx.cm1_ext,
// tree.elements, a FRI polynomial ...) and that module works on it in place -- nothing is staged through the JS heap.
// It also answers the BigBuffer calls the reference makes (length, getElement, setElement, slice, set), each as a
// small transfer, so untouched reference code keeps working on it.
class DevBuffer {
    constructor(nWords, ptr) { this.length = nWords; this.owned = ptr === undefined; this.ptr = this.owned ? addon.devAlloc(Math.max(1, nWords)) : ptr; }
    static from(arr) { const d = new DevBuffer(arr.length); upload(d.ptr, arr, arr.length); return d; }
    addr(offWords = 0) { return this.ptr + 8n * BigInt(offWords); }
    view(offWords, nWords) { return new DevBuffer(nWords, this.addr(offWords)); }      // no ownership
    getElement(i) { const t = new BigUint64Array(1); addon.devDownload(t, this.ptr, i); return t[0]; }
    setElement(i, v) { addon.devUpload(this.ptr, i, BigUint64Array.of(BigInt(v))); }
    slice(a, b) { if (a < 0) a += this.length; if (b === undefined) b = this.length; const t = new BigUint64Array(Math.max(0, b - a)); if (t.length) addon.devDownload(t, this.ptr, a); return t; }
    set(arr, off = 0) { if (arr instanceof DevBuffer) arr = arr.slice(0, arr.length); addon.devUpload(this.ptr, off, arr); }
    zero() { addon.devZero(this.ptr, 0, this.length); }
    toHost() { return this.slice(0, this.length); }
    free() { if (this.owned && this.ptr !== null) { addon.devFree(this.ptr); this.ptr = null; } }

    // ---- the asynchronous leg: copies on the library's copy stream, ordered against the NULL stream by copyAfter / copyFence ----
    // uploadAsync / downloadAsync only enqueue; the PinnedBuffer must stay alive and untouched until copySync() or until work
    // fenced behind the copy has finished.
    uploadAsync(pinned, offWords = 0) { eachPinned(pinned, (arr, o) => addon.devUploadAsync(this.ptr, offWords + o, arr)); return this; }
    downloadAsync(pinned, offWords = 0) { eachPinned(pinned, (arr, o) => addon.devDownloadAsync(arr, this.ptr, offWords + o)); return this; }
    // a new device buffer filled from pinned memory; {after: true} first orders the copy after the work now on the NULL stream
    static fromHost(pinned, opts = {}) { const d = new DevBuffer(pinned.length); if (opts.after) addon.copyAfter(); return d.uploadAsync(pinned); }
    // nRows x nCols words of a `.commit` / `.const` file (raw little-endian u64, witnessCalculator.js:145-196) streamed into HBM through
    // the library's two pinned chunks; {dstCols} pads every row with zeros (writeToBigBuffer(buff, nCols), :198-214), {check} (default
    // true) throws when a word is not a canonical field element.  Blocks until the data is in HBM.
    static fromFile(fileName, nRows, nCols, opts = {}) {
        const dstCols = opts.dstCols === undefined ? nCols : opts.dstCols, check = opts.check === undefined ? true : !!opts.check;
        const d = new DevBuffer(nRows * dstCols);
        try {
            const bad = addon.devLoadFile(fileName, opts.byteOffset || 0, nRows, nCols, d.ptr, dstCols, opts.chunkWords || 0, check);
            if (check && bad !== NO_BAD) {
                const r = bad / BigInt(nCols), c = bad % BigInt(nCols);
                throw new Error(fileName + ": word " + bad + " is " + d.getElement(Number(r) * dstCols + Number(c)) + ", not a canonical field element");
            }
        } catch (e) { d.free(); throw e; }
        return d;
    }
    // the words are read on the copy stream: first behind whatever the NULL stream (or opts.stream) still has to write into them
    toFile(fileName, opts = {}) { addon.copyAfter(opts.stream); addon.devSaveFile(fileName, opts.byteOffset || 0, this.ptr, this.length, opts.chunkWords || 0); }
}
function isDev(b) { return b instanceof DevBuffer; }
const NO_BAD = 0xFFFFFFFFFFFFFFFFn;
function copyAfter(stream) { addon.copyAfter(stream); }      // copies enqueued from now on start after the work now on the stream (default: NULL)
function copyFence(stream) { addon.copyFence(stream); }      // work enqueued on the stream from now on starts after the copies so far
function copySync() { addon.copySync(); }

// A chunked host container with pilcom BigBuffer's surface {length, getElement, setElement, slice(a,b) -> BigUint64Array, set(arr, off)}:
// one typed array cannot hold more than require("buffer").kMaxLength bytes (2 GB on Node 12), a witness has 13 GB.
// chunkWords defaults to the largest power of two the running Node allows.
function maxChunkWords() { return 2 ** Math.floor(Math.log2(Math.floor(require("buffer").kMaxLength / 8))); }
class ChunkedBuffer {
    constructor(nWords, chunkWords, allocChunk = (n) => new BigUint64Array(n)) {
        this.length = nWords;
        this.chunkWords = chunkWords || maxChunkWords();
        this.chunks = [];
        for (let o = 0; o < nWords; o += this.chunkWords) this.chunks.push(allocChunk(Math.min(this.chunkWords, nWords - o)));
    }
    getElement(i) { return this.chunks[Math.floor(i / this.chunkWords)][i % this.chunkWords]; }
    setElement(i, v) { this.chunks[Math.floor(i / this.chunkWords)][i % this.chunkWords] = BigInt(v); }
    slice(a = 0, b = this.length) {
        if (a < 0) a += this.length;
        if (b < 0) b += this.length;
        b = Math.min(b, this.length);
        const out = new BigUint64Array(Math.max(0, b - a));
        for (let o = a; o < b;) {
            const k = Math.floor(o / this.chunkWords), at = o % this.chunkWords, m = Math.min(b - o, this.chunkWords - at);
            out.set(this.chunks[k].subarray(at, at + m), o - a);
            o += m;
        }
        return out;
    }
    set(arr, off = 0) {
        if (!isFlat(arr)) arr = arr.slice(0, arr.length);
        if (off + arr.length > this.length) throw new RangeError("offset is out of bounds");
        for (let o = 0; o < arr.length;) {
            const k = Math.floor((off + o) / this.chunkWords), at = (off + o) % this.chunkWords, m = Math.min(arr.length - o, this.chunkWords - at);
            this.chunks[k].set(arr.subarray(o, o + m), at);
            o += m;
        }
    }
}
// The same container on pinned host memory (pil2gl_host_alloc): what uploadAsync / downloadAsync / DevBuffer.fromHost take.  The
// reference's writeToBigBuffer(buff) (witnessCalculator.js:198-214) fills it unchanged -- it only calls setElement.  The memory goes
// back when the chunks are collected, or at free().  Zero-filled like a BigBuffer unless zero = false (pinned memory comes as it is; a
// buffer that is about to be overwritten whole need not pay for the pass).
class PinnedBuffer extends ChunkedBuffer {
    constructor(nWords, chunkWords, zero = true) { super(nWords, chunkWords, (n) => { const c = addon.hostAlloc(n); if (zero) c.fill(0n); return c; }); }
    free() { for (const c of this.chunks) addon.hostFree(c); this.chunks = []; this.length = 0; }
}
function eachPinned(pinned, fn) {
    if (!(pinned instanceof PinnedBuffer)) throw new TypeError("expected a PinnedBuffer (pageable containers go through upload() / DevBuffer.from())");
    let o = 0;
    for (const c of pinned.chunks) { fn(c, o); o += c.length; }
}

// Containers: BigUint64Array, or anything with pilcom.BigBuffer's surface {length, slice(a,b) -> BigUint64Array, set(arr, off)}
// (used by the reference at fft_p.js:28-29,89,116; merklehash_p.js:70; stark_gen_helpers.js:104-137).
function upload(dptr, buf, nWords) {
    if (isFlat(buf)) { addon.devUpload(dptr, 0, nWords === buf.length ? buf : buf.subarray(0, nWords)); return; }
    for (let o = 0; o < nWords; o += CHUNK) addon.devUpload(dptr, o, buf.slice(o, Math.min(nWords, o + CHUNK)));
}
function download(buf, dptr, nWords) {
    if (isFlat(buf)) { addon.devDownload(nWords === buf.length ? buf : buf.subarray(0, nWords), dptr, 0); return; }
    for (let o = 0; o < nWords; o += CHUNK) {
        const tmp = new BigUint64Array(Math.min(CHUNK, nWords - o));
        addon.devDownload(tmp, dptr, o);
        buf.set(tmp, o);
    }
}
// run fn(dIn, dOut) with device staging buffers for containers that are not one flat array
function staged(src, nIn, dst, nOut, fn) {
    const dIn = addon.devAlloc(nIn);
    let dOut;
    try {
        dOut = addon.devAlloc(nOut);
        upload(dIn, src, nIn);
        fn(dIn, dOut);
        download(dst, dOut, nOut);
    } finally {
        addon.devFree(dIn);
        if (dOut !== undefined) addon.devFree(dOut);
    }
}

// Compile at setup, prove many times (include/pil2gl.h, "code objects ... kept on disk"); none of the three needs a device.
// jitCacheSetDir(dir): where the evaluator's run-time compiled kernels are kept between processes; null / "" = nowhere, the default
// unless PIL2GL_JIT_CACHE_DIR is set.  The directory holds code that will run on the GPU: keep it private to the user.
function jitCacheSetDir(dir) { addon.jitCacheSetDir(dir ? String(dir) : null); }
// -> { memoryHits, diskHits, compiles, diskWrites, rejected, failedWrites, compileMs, diskLoadMs } since load or the last jitCacheSetDir
function jitCacheStats() { return addon.jitCacheStats(); }
// (ops, nOps, nTmp as prover_helpers.encode writes them; widths: columns of every section; nScalars: the scalar pool, or how many
// words it will hold -- then pairwise distinct placeholders stand in) -> { routed: "jit" | "interp", origin: "none" | "compiled" | "disk", codeBytes, slots }
function precompileProgram(ops, nOps, nTmp, nBits, primeShift, widths, nScalars) {
    const w = widths instanceof BigUint64Array ? widths : BigUint64Array.from(Array.from(widths, (x) => BigInt(x)));
    let sc = nScalars;
    if (!(sc instanceof BigUint64Array)) { sc = new BigUint64Array(Math.max(1, Number(nScalars))); for (let i = 0; i < sc.length; i++) sc[i] = 0x9E3779B97F4A7C15n * BigInt(i + 1) % 0xFFFFFFFF00000001n; }
    return addon.precompileProgram(ops, nOps, nTmp, nBits, primeShift, w, sc);
}
module.exports = { addon, isFlat, isDev, DevBuffer, PinnedBuffer, ChunkedBuffer, copyAfter, copyFence, copySync, upload, download, staged, CHUNK,
    jitCacheSetDir, jitCacheStats, precompileProgram };
