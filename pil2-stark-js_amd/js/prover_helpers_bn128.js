// The evaluator entry points of src/prover/prover_helpers.js as the fflonk final prover uses them (ctx.F = curve.Fr, ctx.prover === "fflonk"):
//   calculateExps(ctx, code, dom, debug, ret)                                          (prover_helpers.js:31-72)
//   callCalculateExps(stage, code, dom, ctx, parallelExec, useThreads, debug, global)  (prover_helpers.js:23-29)
// The op-list `code.code` is encoded into the binary form of include/pil2gl_expr.h, operand resolution following getRef / setRef /
// evalMap (prover_helpers.js:109-259), and run for every row of the domain by pil2gl_bn128_eval_program_dev (csrc/bn_expr.hip).
//   sections  ctx.const_n / const_ext, cm{s}_n / cm{s}_ext, x_n / x_ext, Zi_ext, q_ext are DevBuffers of 32-byte elements (4 words each,
//             the Montgomery bytes ffjavascript's Fr keeps): resident, nothing is staged, destinations are written in place
//   scalars   ctx.publics[i], ctx.challenges[s][i], ctx.subproofValues[...] are Uint8Arrays of 32 Montgomery bytes, as ctx.F holds
//             them; number{value} is ctx.F.e(value) (pil2gl_bn128_convert when ctx has no F)
// No arithmetic happens here.
"use strict";
const { addon, isDev, DevBuffer } = require("./native.js");
const { asWords } = require("./bn128_stage.js");
const OP = { add: 0, sub: 1, mul: 2, copy: 3 };
const TMP = 0, SEC = 1, SCALAR = 2;
const R = 21888242871839275222246405745257275088548364400416034343698204186575808495617n;

function fe(ctx, value) {          // F.e(value) as 4 words
    let v = BigInt(value) % R; if (v < 0n) v += R;
    if (ctx.F && typeof ctx.F.e === "function") return words(ctx.F.e(v));
    const inp = new BigUint64Array(4), out = new BigUint64Array(4);
    for (let k = 0; k < 4; k++) inp[k] = (v >> BigInt(64 * k)) & 0xFFFFFFFFFFFFFFFFn;
    addon.bn128Convert(inp, 1, 1, out);
    return out;
}
function words(u8) {
    if (!(u8 instanceof Uint8Array) || u8.length !== 32) throw new Error("prover_helpers_bn128: a scalar must be a Uint8Array of 32 bytes");
    return asWords(u8);
}

function encode(code, dom, ctx, global) {
    const info = ctx.pilInfo;
    const sections = [], secIndex = new Map(), scalars = [], numbers = new Map();
    function section(name, width, zi) {
        const key = zi === undefined ? name : name + "#" + zi;
        if (!secIndex.has(key)) { secIndex.set(key, sections.length); sections.push({ name, width, zi }); }
        return secIndex.get(key);
    }
    const scalar = (w) => { scalars.push(w); return { kind: SCALAR, section: 0, prime: 0, index: scalars.length - 1 }; };
    function ref(r, isDest) {
        if ((r.dim || 1) !== 1) throw new Error("Invalid dom");                                     // prover_helpers.js:123: Fr elements have dim 1
        switch (r.type) {
            case "tmp": return { kind: TMP, section: 0, prime: 0, index: r.id };
            case "$ret": return { kind: SEC, section: section("$ret", 1), prime: 0, index: 0 };     // calculateExps(..., ret = true)
            case "cm": {                                                                            // evalMap, prover_helpers.js:220-259
                const p = info.cmPolsMap[r.id], st = "cm" + p.stage;
                return { kind: SEC, section: section(st + "_" + dom, info.mapSectionsN[st]), prime: r.prime || 0, index: p.stagePos };
            }
            case "q":
                if (!isDest) break;
                if (dom !== "ext") throw new Error("Accessing q in domain n");
                return { kind: SEC, section: section("q_ext", 1), prime: 0, index: 0 };
        }
        if (isDest) throw new Error("Invalid reference type set: " + r.type);
        switch (r.type) {
            case "const": return { kind: SEC, section: section("const_" + dom, info.nConstants), prime: r.prime || 0, index: r.id };
            case "x": return { kind: SEC, section: section("x_" + dom, 1), prime: 0, index: 0 };
            case "Zi": {
                const boundary = info.boundaries[r.boundaryId];
                let ziIndex;
                if (boundary.name === "everyFrame") ziIndex = info.boundaries.findIndex((b) => b.name === "everyFrame" && b.offsetMin === boundary.offsetMin && b.offsetMax === boundary.offsetMax);
                else if (["everyRow", "firstRow", "lastRow"].includes(boundary.name)) ziIndex = info.boundaries.findIndex((b) => b.name === boundary.name);
                else throw new Error("Invalid boundary: " + boundary.name);
                if (ziIndex === -1) throw new Error("Something went wrong");
                return { kind: SEC, section: section("Zi_ext", 1, ziIndex), prime: 0, index: 0 };
            }
            case "number": {
                const key = String(r.value);
                if (!numbers.has(key)) numbers.set(key, scalar(fe(ctx, r.value)));
                return numbers.get(key);
            }
            case "public": return scalar(words(ctx.publics[r.id]));
            case "challenge": return scalar(words(ctx.challenges[r.stage - 1][r.stageId]));
            case "subproofValue": return scalar(words(global ? ctx.subproofValues[r.subproofId][r.id] : ctx.subproofValues[r.id]));
            default: throw new Error("Invalid reference type get: " + r.type);
        }
    }
    let nTmp = 0;
    for (const c of code) for (const r of [c.dest, ...c.src]) if (r.type === "tmp") nTmp = Math.max(nTmp, r.id + 1);
    // glx_op: u32 op, u32 pad, 3 x glx_ref{u8 kind,u8 dim,u16 section,i32 prime,u32 index,u32 pad} = 56 bytes
    const buf = new ArrayBuffer(code.length * 56), dv = new DataView(buf);
    const put = (o, r) => { dv.setUint8(o, r.kind); dv.setUint8(o + 1, 1); dv.setUint16(o + 2, r.section, true); dv.setInt32(o + 4, r.prime, true); dv.setUint32(o + 8, r.index, true); };
    for (let j = 0; j < code.length; j++) {
        const c = code[j], o = j * 56;
        if (!(c.op in OP)) throw new Error("Invalid op:" + c.op);
        dv.setUint32(o, OP[c.op], true);
        put(o + 24, ref(c.src[0], false));
        if (c.op !== "copy") put(o + 40, ref(c.src[1], false));
        put(o + 8, ref(c.dest, true));
    }
    const pool = new BigUint64Array(4 * scalars.length);
    scalars.forEach((w, i) => pool.set(w, 4 * i));
    return { ops: new BigUint64Array(buf), nOps: code.length, nTmp, sections, scalars: pool };
}

// ret: the value the LAST op produced, for every row -- an array of 32-byte Uint8Arrays (compileCode returns getRef(dest), :102-104).
// ret === "dev": the column stays in HBM and onDev(devPtr, rows) reads what it needs of it (the debug path).
function run(code, dom, ctx, global, ret, onDev) {
    let ops = code.code;
    if (ret) {
        if (!ops.length) throw new Error("calculateExps: an empty program returns nothing");
        const last = ops[ops.length - 1];
        // a temporary is simply redirected; any other destination is written as the program says AND copied out
        if (last.dest.type === "tmp") ops = ops.slice(0, -1).concat([{ op: last.op, dest: { type: "$ret", dim: 1 }, src: last.src }]);
        else ops = ops.concat([{ op: "copy", dest: { type: "$ret", dim: 1 }, src: [last.dest] }]);
    }
    const enc = encode(ops, dom, ctx, global);
    const nBits = dom === "n" ? ctx.nBits : ctx.nBitsExt;
    const rows = 2 ** nBits;
    const ptrs = new BigUint64Array(enc.sections.length), widths = new BigUint64Array(enc.sections.length);
    let retBuf = null, out;
    try {
        enc.sections.forEach((s, i) => {
            widths[i] = BigInt(s.width);
            if (s.name === "$ret") { retBuf = new DevBuffer(rows * 4); ptrs[i] = retBuf.ptr; return; }
            const buf = ctx[s.name];
            if (!buf) throw new Error("ctx." + s.name + " is not allocated");
            if (!isDev(buf)) throw new Error("prover_helpers_bn128: ctx." + s.name + " must be a DevBuffer");
            const base = s.zi === undefined ? 0 : s.zi * rows * 4;                   // ctx.Zi_ext[ziIndex * extN + i]
            if (buf.length < base + rows * s.width * 4) throw new Error("ctx." + s.name + " holds " + buf.length + " words, needs " + (base + rows * s.width * 4));
            ptrs[i] = buf.addr(base);
        });
        addon.bn128EvalProgramDev(enc.ops, enc.nOps, enc.nTmp, nBits, dom === "n" ? 0 : ctx.extendBits, ptrs, widths, enc.scalars);
        if (ret === "dev") out = onDev(retBuf.ptr, rows);
        else if (ret) {
            const flat = new Uint8Array(retBuf.toHost().buffer);                      // a synchronous copy: ordered after the kernel
            out = new Array(rows);
            for (let r = 0; r < rows; r++) out[r] = flat.slice(32 * r, 32 * r + 32);
        }
    } finally {
        if (retBuf) retBuf.free();
    }
    return out;
}

// debug = true (prover_helpers.js:46-70, fflonk_prover_worker.js:19-26): `code` is one constraint with its boundary and source line.  The
// op-list runs on the whole domain and pil2gl_bn128_first_nonzero_row_dev finds the first row of the boundary whose value is not zero;
// only that row and its 32 bytes come back.  The message is the reference's, the value printed by ctx.F.toString where ctx has an F.
function checkConstraint(ctx, code, dom, global) {
    const N = dom === "n" ? 2 ** ctx.nBits : 2 ** ctx.nBitsExt;
    let first, last;
    if (code.boundary === "everyRow") { first = 0; last = N; }
    else if (code.boundary === "firstRow" || code.boundary === "finalProof") { first = 0; last = 1; }
    else if (code.boundary === "lastRow") { first = N - 1; last = N; }
    else if (code.boundary === "everyFrame") { first = code.offsetMin; last = N - code.offsetMax; }
    else throw new Error("Invalid boundary: " + code.boundary);
    if (!ctx.errors) ctx.errors = [];
    if (last <= first) return;
    const hit = run(code, dom, ctx, global, "dev", (dev) => {
        const [row, ...w] = addon.bn128FirstNonzeroRowDev(dev, 1, 0, first, last);
        return row === 0xFFFFFFFFFFFFFFFFn ? null : { row, val: new Uint8Array(BigUint64Array.from(w).buffer) };
    });
    if (!hit) return;
    const shown = ctx.F && typeof ctx.F.toString === "function" && ctx.F.toString !== Object.prototype.toString ? ctx.F.toString(hit.val) : "0x" + Buffer.from(hit.val).reverse().toString("hex");
    ctx.errors.push(`${code.line}: identity does not match w=${hit.row} val=${shown} `);
}

module.exports.calculateExps = function calculateExps(ctx, code, dom, debug, ret, global) {
    if (debug) return checkConstraint(ctx, code, dom, !!global);
    return run(code, dom, ctx, !!global, !!ret);
};
module.exports.callCalculateExps = async function callCalculateExps(stage, code, dom, ctx, parallelExec, useThreads, debug, global = false) {
    module.exports.calculateExps(ctx, code, dom, debug, false, global);               // prover_helpers.js:23-29 (no worker pool here)
};
module.exports.encode = encode;
