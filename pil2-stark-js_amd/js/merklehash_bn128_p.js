// Drop-in for src/helpers/hash/merklehash/merklehash_bn128_p.js: `await buildMerkleHash(arity, custom)` -> MH with
// merkelize / getElement / getGroupProof / calculateRootFromGroupProof / verifyGroupProof / eqRoot / root /
// writeToFile / readFromFile (merklehash_bn128_p.js:10-285).  tree.nodes is a BigUint64Array of Montgomery-form field
// elements (4 words each) laid out as the reference's (:31-45, :89-101); roots and siblings are BigInt in normal form.
// Handed a DevBuffer, merkelize builds the tree next to its leaves and leaves it in HBM (tree.nodes is a DevBuffer too), as the
// Goldilocks module does: openings are then one device call per tree (getGroupProofs), the root is the only node that is downloaded.
// The reference obtains its permutation from circomlibjs / wasmcurves; here it is libpil2gl's (csrc/bn128.hip).
"use strict";
const fs = require("fs");
const { addon, isFlat, isDev, DevBuffer, upload } = require("./native.js");

const R = 21888242871839275222246405745257275088548364400416034343698204186575808495617n;
const M64 = 0xFFFFFFFFFFFFFFFFn;

function toWords(vals) {
    const a = new BigUint64Array(4 * vals.length);
    for (let i = 0; i < vals.length; i++) {
        let v = BigInt(vals[i]) % R; if (v < 0n) v += R;
        for (let k = 0; k < 4; k++) a[4 * i + k] = (v >> BigInt(64 * k)) & M64;
    }
    return a;
}
function fromWords(a, i) { return a[4 * i] | (a[4 * i + 1] << 64n) | (a[4 * i + 2] << 128n) | (a[4 * i + 3] << 192n); }

// circomlibjs poseidon(inputs, initState, nOut) with BigInt in / out
function poseidon(inputs, initState, nOut) {
    nOut = nOut || 1;
    const out = new BigUint64Array(4 * nOut);
    addon.bn128Poseidon(toWords(inputs), toWords([initState || 0n]), 1, inputs.length, nOut, out);
    const res = [];
    for (let i = 0; i < nOut; i++) res.push(fromWords(out, i));
    return nOut === 1 ? res[0] : res;
}
// transcript.bn128.js:56-66 for a list: the full blocks of nIn elements in `flat` absorbed one after the other (each
// permutation's output 0 is the next one's state element 0) in one device call -> the nIn+1 outputs of the last one
poseidon.absorbChain = function (flat, initState, nIn) {
    const out = new BigUint64Array(4 * (nIn + 1));
    addon.bn128SpongeAbsorb(toWords(flat), flat.length / nIn, nIn, toWords([initState || 0n]), out);
    const res = [];
    for (let i = 0; i <= nIn; i++) res.push(fromWords(out, i));
    return res;
};
function fromMontgomery(words) {
    const n = words.length / 4, out = new BigUint64Array(words.length);
    addon.bn128Convert(words, n, 0, out);
    const res = [];
    for (let i = 0; i < n; i++) res.push(fromWords(out, i));
    return res;
}

class LinearHashBN {    // linearhash.bn128.js:4-62
    constructor(arity, custom) { this.arity = arity; this.custom = custom; }
    hash(vals) {
        const flat = [];
        for (let i = 0; i < vals.length; i++) {
            if (Array.isArray(vals[i])) for (let k = 0; k < vals[i].length; k++) flat.push(BigInt(vals[i][k])); else flat.push(BigInt(vals[i]));
        }
        const vals3 = [];
        for (let i = 0; i < flat.length; i += 3) {
            let acc = 0n;
            for (let k = 0; k < 3 && i + k < flat.length; k++) acc += flat[i + k] << BigInt(64 * k);
            vals3.push(acc % R);
        }
        if (vals3.length == 0) return 0n;
        if (vals3.length == 1) return vals3[0];
        let st = 0n, inHash = [];
        for (let i = 0; i < vals3.length; i++) {
            inHash.push(vals3[i]);
            if (inHash.length == this.arity) { st = poseidon(inHash, st); inHash = []; }
        }
        if (inHash.length > 0) {
            while (inHash.length % this.arity !== 0 && this.custom) inHash.push(0n);
            st = poseidon(inHash, st);
        }
        return st;
    }
}

class MerkleHash {
    constructor(arity, custom) {
        this.arity = arity; this.custom = custom;
        this.lh = new LinearHashBN(arity, custom);
        this.poseidon = poseidon;
    }

    _getNNodes(n) { return addon.bn128MerkleNumNodes(n, this.arity); }      // merklehash_bn128_p.js:31-45

    async merkelize(buff, width, height) {
        if (isDev(buff)) {          // resident: the tree is built next to its leaves and stays there
            const nodes = new DevBuffer(this._getNNodes(height) * 4);
            addon.bn128MerkelizeDev(buff.ptr, width, height, this.arity, this.custom ? 1 : 0, nodes.ptr);
            return { elements: buff, nodes, width, height };
        }
        const tree = { elements: buff, nodes: new BigUint64Array(this._getNNodes(height) * 4), width, height };
        if (isFlat(buff)) {
            addon.bn128Merkelize(buff, width, height, this.arity, this.custom ? 1 : 0, tree.nodes);
        } else {
            const dEl = addon.devAlloc(width * height);
            let dNodes;
            try {
                dNodes = addon.devAlloc(tree.nodes.length);
                upload(dEl, buff, width * height);
                addon.bn128MerkelizeDev(dEl, width, height, this.arity, this.custom ? 1 : 0, dNodes);
                addon.devDownload(tree.nodes, dNodes, 0);
            } finally {
                addon.devFree(dEl);
                if (dNodes !== undefined) addon.devFree(dNodes);
            }
        }
        return tree;
    }

    getElement(tree, idx, subIdx) {
        const e = tree.elements;
        return isFlat(e) ? e[tree.width * idx + subIdx] : e.getElement(tree.width * idx + subIdx);
    }

    _nLevels(height) { let nl = 0; for (let n = height; n > 1; n = Math.floor((n - 1) / this.arity) + 1) nl++; return nl; }
    // siblings: nLevels x arity field elements (4 words each, normal form) from word offset o -> the reference's array of levels
    _levels(sib, o, nl) {
        const mp = [];
        for (let l = 0; l < nl; l++) { const g = []; for (let i = 0; i < this.arity; i++) g.push(fromWords(sib, o / 4 + l * this.arity + i)); mp.push(g); }
        return mp;
    }

    getGroupProof(tree, idx) {          // merklehash_bn128_p.js:142-182
        if ((idx < 0) || (idx >= tree.height)) throw new Error("Out of range");
        if (isDev(tree.elements) && isDev(tree.nodes)) {        // only the opened row and its groups cross PCIe
            const nl = this._nLevels(tree.height), vals = new BigUint64Array(Math.max(1, tree.width)), sib = new BigUint64Array(Math.max(1, nl * this.arity * 4));
            addon.bn128GroupProofDev(tree.elements.ptr, tree.nodes.ptr, tree.width, tree.height, this.arity, idx, vals, sib);
            return [Array.from(vals.subarray(0, tree.width)), this._levels(sib, 0, nl)];
        }
        const v = new Array(tree.width);
        for (let i = 0; i < tree.width; i++) v[i] = this.getElement(tree, idx, i);
        const nBitsArity = Math.ceil(Math.log2(this.arity));
        const mp = [];
        let offset = 0, n = tree.height;
        while (n > 1) {
            const si = idx ^ (idx & (this.arity - 1));
            const grp = fromMontgomery(tree.nodes.slice((offset + si) * 4, (offset + si + this.arity) * 4));
            mp.push(grp.map((g, i) => (i < n ? g : 0n)));
            const nextN = Math.floor((n - 1) / this.arity) + 1;
            offset += nextN * this.arity; n = nextN; idx = idx >> nBitsArity;
        }
        return [v, mp];
    }

    // getGroupProof for every query of a tree (fri.js:83-105 opens each tree at all query rows): for a device-resident tree one gather
    // kernel and one copy back; host trees one by one.  Same values as getGroupProof: siblings in normal form, nodes beyond a level's count 0.
    getGroupProofs(tree, idxs) {
        if (!(isDev(tree.elements) && isDev(tree.nodes)) || idxs.length === 0) return idxs.map((i) => this.getGroupProof(tree, i));
        for (const idx of idxs) if ((idx < 0) || (idx >= tree.height)) throw new Error("Out of range");
        const nl = this._nLevels(tree.height), w = tree.width, per = nl * this.arity * 4, n = idxs.length;
        const vals = new BigUint64Array(Math.max(1, n * w)), sib = new BigUint64Array(Math.max(1, n * per));
        addon.bn128GroupProofsDev(tree.elements.ptr, tree.nodes.ptr, w, tree.height, this.arity, BigUint64Array.from(idxs, BigInt), vals, sib);
        return idxs.map((_, q) => [Array.from(vals.subarray(q * w, (q + 1) * w)), this._levels(sib, q * per, nl)]);
    }

    calculateRootFromGroupProof(mp, idx, vals) {    // merklehash_bn128_p.js:184-232
        let value = this.lh.hash(vals);
        const nBitsArity = Math.ceil(Math.log2(this.arity));
        for (let o = 0; o < mp.length; o++) {
            const curIdx = idx & (this.arity - 1);
            idx = idx >> nBitsArity;
            const group = mp[o].map((x) => BigInt(x));
            group[curIdx] = value;
            value = poseidon(group, 0n);
        }
        return value;
    }

    // batch form for the verifier's loops over queries (stark_verify.js:165-178, fri.js:140): proofs = [[vals, siblings], ...] of one tree ->
    // their roots; packing, leaf sponge and every level of every opening in ONE device call (a wave per opening walks its whole path)
    calculateRootsFromGroupProofs(proofs, idxs) {
        const n = proofs.length;
        if (n === 0) return [];
        const flatten = (vals) => { const f = []; for (const v of vals) { if (Array.isArray(v)) for (const x of v) f.push(BigInt(x)); else f.push(BigInt(v)); } return f; };
        const first = flatten(proofs[0][0]), width = first.length, nl = proofs[0][1].length, a = this.arity, per = nl * a * 4;
        const vals = new BigUint64Array(Math.max(1, n * width)), sib = new BigUint64Array(Math.max(1, n * per)), ii = new BigUint64Array(n), roots = new BigUint64Array(4 * n);
        for (let q = 0; q < n; q++) {
            const f = q === 0 ? first : flatten(proofs[q][0]), mp = proofs[q][1];
            if (f.length !== width || mp.length !== nl || mp.some((g) => g.length !== a)) throw new Error("openings of different shapes in one batch");
            for (let i = 0; i < width; i++) vals[q * width + i] = f[i];
            for (let l = 0; l < nl; l++) for (let i = 0; i < a; i++) {
                let v = BigInt(mp[l][i]); if (v < 0n || v >> 256n) { v %= R; if (v < 0n) v += R; }        // below 2^256 the library reduces
                const o = q * per + (l * a + i) * 4;
                for (let k = 0; k < 4; k++) sib[o + k] = (v >> BigInt(64 * k)) & M64;
            }
            ii[q] = BigInt(idxs[q]);
        }
        addon.bn128RootsFromGroupProofs(vals, sib, width, nl, a, this.custom ? 1 : 0, 0, ii, n, roots);
        const out = [];
        for (let q = 0; q < n; q++) out.push(fromWords(roots, q));
        return out;
    }
    verifyGroupProofs(root, proofs, idxs) { return this.calculateRootsFromGroupProofs(proofs, idxs).every((r) => this.eqRoot(r, root)); }

    eqRoot(r1, r2) { return BigInt(r1) === BigInt(r2); }

    verifyGroupProof(root, mp, idx, groupElements) {
        return this.eqRoot(this.calculateRootFromGroupProof(mp, idx, groupElements), root);
    }

    root(tree) { return fromMontgomery(tree.nodes.slice(tree.nodes.length - 4))[0]; }     // resident: the last 4 words are all that is downloaded

    async writeToFile(tree, fileName) {     // merklehash_bn128_p.js:243-263
        if (isDev(tree.elements) && isDev(tree.nodes)) {        // resident: HBM -> file through the library's pinned chunks, nothing on the JS heap
            await fs.promises.writeFile(fileName, new Uint8Array(BigUint64Array.from([BigInt(tree.width), BigInt(tree.height)]).buffer));
            tree.elements.view(0, tree.width * tree.height).toFile(fileName, { byteOffset: 16 });
            tree.nodes.toFile(fileName, { byteOffset: 16 + 8 * tree.width * tree.height });
            return;
        }
        const fd = await fs.promises.open(fileName, "w+");
        await fd.write(new Uint8Array(BigUint64Array.from([BigInt(tree.width), BigInt(tree.height)]).buffer));
        const el = tree.elements;
        const n = tree.width * tree.height;
        const chunk = 1 << 22;
        for (let i = 0; i < n; i += chunk) {
            const sb = isFlat(el) ? el.subarray(i, Math.min(n, i + chunk)) : el.slice(i, Math.min(n, i + chunk));
            await fd.write(new Uint8Array(sb.buffer, sb.byteOffset, sb.byteLength));
        }
        await fd.write(new Uint8Array(tree.nodes.buffer, tree.nodes.byteOffset, tree.nodes.byteLength));
        await fd.close();
    }

    // merklehash_bn128_p.js:265-285.  {device: true}: elements and nodes are DevBuffers streamed from the file into HBM by the library
    // (the elements checked canonical; the nodes are Montgomery-form BN254 words, which no Goldilocks bound applies to).  Without it, one
    // BigUint64Array each as before, or a chunked host container when the elements are larger than a typed array can be.
    async readFromFile(fileName, opts = {}) {
        const { hostContainer, readInto } = require("./merklehash_p.js");
        const fd = await fs.promises.open(fileName, "r");
        try {
            const header = new BigUint64Array(2);
            await fd.read(new Uint8Array(header.buffer), 0, 16, 0);
            const tree = { width: Number(header[0]), height: Number(header[1]) };
            const nEl = tree.width * tree.height, nNodes = this._getNNodes(tree.height) * 4;
            if (opts.device) {
                tree.elements = DevBuffer.fromFile(fileName, tree.height, tree.width, { byteOffset: 16, check: opts.check, chunkWords: opts.chunkWords });
                tree.nodes = DevBuffer.fromFile(fileName, 1, nNodes, { byteOffset: 16 + 8 * nEl, check: false, chunkWords: opts.chunkWords });
                return tree;
            }
            tree.elements = hostContainer(nEl, opts.chunkWords);
            tree.nodes = new BigUint64Array(nNodes);
            const pos = await readInto(fd, tree.elements, 16);
            await readInto(fd, tree.nodes, pos);
            return tree;
        } finally {
            await fd.close();
        }
    }
}

module.exports = async function buildMerkleHash(arity, custom) { return new MerkleHash(arity, !!custom); };
module.exports.poseidon = poseidon;
module.exports.LinearHashBN = LinearHashBN;
