// The staging scope of pil2-stark-js_amd/js/bn128_stage.js without a GPU: a stand-in for the addon's four memory calls keeps "device
// memory" in a Map of BigUint64Arrays and logs every call; the piece size is 64 bytes, so a 200-byte buffer crosses three piece
// boundaries.  Asserts on the call log and on the bytes.  usage: node bn128_stage_unit.js; exits non-zero on the first failure.
"use strict";
const assert = require("assert");
const path = require("path");
const stage = require(path.join(__dirname, "..", "..", "pil2-stark-js_amd", "js", "bn128_stage.js"));

class FakeDev { constructor(ptr, nWords) { this.ptr = ptr; this.length = nWords; } }
function standIn(failAllocAt) {
    const mem = new Map(), log = [];
    let next = 0x1000n, allocs = 0;
    const dev = {
        devAlloc(nWords) {
            if (++allocs === failAllocAt) throw new Error("out of device memory");
            const p = next; next += 0x10000n;
            mem.set(p, new BigUint64Array(nWords)); log.push(["alloc", p, nWords]);
            return p;
        },
        devFree(p) { assert(mem.delete(p), "freed twice or never allocated: " + p); log.push(["free", p]); },
        devUpload(p, offWords, arr) { assert(arr instanceof BigUint64Array); mem.get(p).set(arr, offWords); log.push(["up", p, offWords, arr.length * 8]); },
        devDownload(arr, p, offWords) { arr.set(mem.get(p).subarray(offWords, offWords + arr.length)); log.push(["down", p, offWords, arr.length * 8]); },
    };
    const s = stage.createStage(dev, (b) => b instanceof FakeDev);
    return Object.assign({ mem, log, calls: (kind) => log.filter((c) => c[0] === kind) }, s);
}
class Chunked {              // { byteLength, slice(a, b) -> Uint8Array, set(u8, byteOffset) } over 48-byte chunks
    constructor(u8) { this.byteLength = u8.length; this.chunks = []; for (let o = 0; o < u8.length; o += 48) this.chunks.push(Uint8Array.from(u8.subarray(o, o + 48))); }
    slice(a = 0, b = this.byteLength) {
        const out = new Uint8Array(Math.max(0, b - a));
        for (let o = a; o < b;) { const k = Math.floor(o / 48), at = o % 48, n = Math.min(b - o, 48 - at); out.set(this.chunks[k].subarray(at, at + n), o - a); o += n; }
        return out;
    }
    set(arr, off = 0) {
        for (let o = 0; o < arr.length;) { const k = Math.floor((off + o) / 48), at = (off + o) % 48, n = Math.min(arr.length - o, 48 - at); this.chunks[k].set(arr.subarray(o, o + n), at); o += n; }
    }
}
const pattern = (n, seed) => Uint8Array.from({ length: n }, (_, i) => (i * 7 + seed) & 0xFF);
const deviceBytes = (s, p, n) => new Uint8Array(s.mem.get(p).buffer, 0, n);
const PIECES = [[0, 64], [8, 64], [16, 64], [24, 8]];          // word offset, bytes of each piece of 200 bytes
const pieces = (s, kind) => s.calls(kind).map((c) => [c[2], c[3]]);
// the "kernel": every staged byte b -> b ^ 0x5A, checked against what was uploaded
function flip(s, n, want) {
    return ([p]) => { const d = deviceBytes(s, p, n); assert.deepStrictEqual(Array.from(d), Array.from(want)); for (let i = 0; i < n; i++) d[i] ^= 0x5A; return "result"; };
}
const flipped = (u8) => Array.from(u8, (b) => b ^ 0x5A);

const was = stage.setPieceBytes(64);
assert.strictEqual(was, 1 << 28, "the default piece is 2^28 bytes");
assert.throws(() => stage.setPieceBytes(48), /multiple of 32/);

// read-write Uint8Array, 200 bytes: up and down in 64, 64, 64, 8 at words 0, 8, 16, 24; one alloc of 25 words, one free; fn's value returned
{
    const s = standIn(), data = pattern(200, 1), buf = Uint8Array.from(data);
    assert.strictEqual(s.scope([s.inout(buf, 200)], flip(s, 200, data)), "result");
    assert.deepStrictEqual(pieces(s, "up"), PIECES); assert.deepStrictEqual(pieces(s, "down"), PIECES);
    assert.deepStrictEqual(s.calls("alloc").map((c) => c[2]), [25]); assert.strictEqual(s.calls("free").length, 1); assert.strictEqual(s.mem.size, 0);
    assert.deepStrictEqual(Array.from(buf), flipped(data));
}
// the same over a BigBuffer-surface object of 48-byte chunks: staging pieces and container chunks do not line up
{
    const s = standIn(), data = pattern(200, 2), buf = new Chunked(data);
    s.scope([s.inout(buf, 200)], flip(s, 200, data));
    assert.deepStrictEqual(pieces(s, "up"), PIECES); assert.deepStrictEqual(pieces(s, "down"), PIECES);
    assert.deepStrictEqual(Array.from(buf.slice(0, 200)), flipped(data));
}
// a view at byteOffset 4: the right bytes go up, and the parent ArrayBuffer outside the view is untouched after write-back
{
    const s = standIn(), parent = pattern(4 + 200 + 12, 3), before = Uint8Array.from(parent), view = new Uint8Array(parent.buffer, 4, 200);
    s.scope([s.inout(view, 200)], flip(s, 200, before.subarray(4, 204)));
    assert.deepStrictEqual(pieces(s, "up"), PIECES);
    assert.deepStrictEqual(Array.from(parent.subarray(0, 4)), Array.from(before.subarray(0, 4)));
    assert.deepStrictEqual(Array.from(parent.subarray(204)), Array.from(before.subarray(204)));
    assert.deepStrictEqual(Array.from(view), flipped(before.subarray(4, 204)));
}
// read-only: never downloaded, and the host bytes stay; write-only: never uploaded, and the host bytes are replaced
{
    const s = standIn(), data = pattern(96, 4), src = Uint8Array.from(data), dst = new Uint8Array(96).fill(0xEE);
    s.scope([s.input(src, 96), s.output(dst, 96)], ([pi, po]) => { assert.notStrictEqual(pi, po); deviceBytes(s, pi, 96).fill(0); deviceBytes(s, po, 96).set(pattern(96, 5)); });
    assert.deepStrictEqual(s.calls("up").map((c) => c[1]), [s.calls("alloc")[0][1], s.calls("alloc")[0][1]], "only the input is uploaded");
    assert.deepStrictEqual(s.calls("down").map((c) => c[1]), [s.calls("alloc")[1][1], s.calls("alloc")[1][1]], "only the output is downloaded");
    assert.deepStrictEqual(Array.from(src), Array.from(data)); assert.deepStrictEqual(Array.from(dst), Array.from(pattern(96, 5)));
    assert.strictEqual(s.calls("free").length, 2);
}
// a resident buffer stands for itself: no call at all, in any role, and fn receives its ptr
{
    const s = standIn(), d = new FakeDev(0xABC0n, 25), e = new FakeDev(0xDEF0n, 25);
    s.scope([s.input(d, 200), s.output(e, 200), s.inout(d, 200)], (ptrs) => assert.deepStrictEqual(ptrs, [0xABC0n, 0xDEF0n, 0xABC0n]));
    assert.deepStrictEqual(s.log, []);
    assert.strictEqual(s.byteLength(d), 200); assert.strictEqual(s.byteLength(new Uint8Array(72)), 72);
}
// one host object as input and output: one allocation of the larger byte count, the same address twice, up and down once each
{
    const s = standIn(), data = pattern(128, 6), buf = Uint8Array.from(data);
    s.scope([s.input(buf, 64), s.output(buf, 128)], ([pi, po]) => { assert.strictEqual(pi, po); flip(s, 128, data)([pi]); });
    assert.deepStrictEqual(s.calls("alloc").map((c) => c[2]), [16]);
    assert.deepStrictEqual(pieces(s, "up"), [[0, 64], [8, 64]]); assert.deepStrictEqual(pieces(s, "down"), [[0, 64], [8, 64]]);
    assert.deepStrictEqual(Array.from(buf), flipped(data));
}
// an absent output stays null (and undefined counts as absent)
{
    const s = standIn(), buf = pattern(32, 7);
    s.scope([s.input(buf, 32), s.output(null, 32), s.output(undefined, 32)], ([p, a, b]) => { assert.strictEqual(typeof p, "bigint"); assert.strictEqual(a, null); assert.strictEqual(b, null); });
    assert.strictEqual(s.calls("alloc").length, 1);
}
// zero bytes: an allocation of one word, no copies
{
    const s = standIn();
    s.scope([s.inout(new Uint8Array(0), 0)], ([p]) => assert(s.mem.has(p)));
    assert.deepStrictEqual(s.calls("alloc").map((c) => c[2]), [1]);
    assert.strictEqual(s.calls("up").length + s.calls("down").length, 0); assert.strictEqual(s.calls("free").length, 1);
}
// fn throws: both allocations freed exactly once (devFree asserts on a second free), nothing downloaded, the error is fn's own
{
    const s = standIn(), boom = new Error("kernel failed"), a = pattern(64, 8), b = new Uint8Array(64);
    assert.throws(() => s.scope([s.inout(a, 64), s.output(b, 64)], () => { throw boom; }), (e) => e === boom);
    assert.deepStrictEqual(s.calls("free").map((c) => c[1]).sort(), s.calls("alloc").map((c) => c[1]).sort());
    assert.strictEqual(s.calls("alloc").length, 2); assert.strictEqual(s.calls("down").length, 0); assert.strictEqual(s.mem.size, 0);
    assert.deepStrictEqual(Array.from(a), Array.from(pattern(64, 8)));
}
// the second devAlloc throws: the first is freed exactly once, nothing is copied, fn never runs, the allocator's error propagates
{
    const s = standIn(2);
    let ran = false;
    assert.throws(() => s.scope([s.input(pattern(64, 9), 64), s.output(new Uint8Array(64), 64)], () => { ran = true; }), /out of device memory/);
    assert.strictEqual(ran, false);
    assert.deepStrictEqual(s.log.map((c) => c[0]), ["alloc", "free"]); assert.strictEqual(s.log[0][1], s.log[1][1]); assert.strictEqual(s.mem.size, 0);
}
// uploadBytes / downloadBytes on their own move exactly nBytes, piecewise
{
    const s = standIn(), p = 0x9000n, data = pattern(200, 10), back = new Uint8Array(200);
    s.mem.set(p, new BigUint64Array(25));
    s.uploadBytes(p, data, 200); s.downloadBytes(back, p, 200);
    assert.deepStrictEqual(Array.from(back), Array.from(data));
    assert.strictEqual(s.calls("up").reduce((t, c) => t + c[3], 0), 200); assert.strictEqual(s.calls("down").reduce((t, c) => t + c[3], 0), 200);
}
assert.strictEqual(stage.setPieceBytes(was), 64);
console.log("bn128 stage unit OK");
