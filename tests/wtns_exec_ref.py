"""The checker of the recursion witness expansion: a plain transcription of the two reference loops over Python integers -- the additions
`w.push(F.add(F.mul(w[a], ca), F.mul(w[b], cb)))` and the fill `a[j][i] = sMap[i nCols + j] ? w[sMap[i nCols + j]] : 0` of
src/compressor/compressor_exec.js:17-29 (mod p) and src/final/main_final_exec.js:55-67 (mod r) -- a second formulation of the additions
(by dependency level) that the CPU test holds against the serial one, and writers of the three file formats, restated from
compressor/exec_helpers.js:26-47 (writeExecFile), final/exec_helpers.js:93-187 (writeExecFile) and the .wtns layout of snarkjs'
wtns_utils (write).  Nothing here touches the library."""
import random
import struct

import numpy as np

P = 0xFFFFFFFF00000001
R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
MONT = (1 << 256) % R


def additions(w, adds, q):
    """the serial loop: adds = [(a, b, ca, cb)], values and coefficients as integers (any representative) -> the whole w, reduced mod q
    only where the reference's F.mul / F.add reduce: the derived signals"""
    w = list(w)
    for a, b, ca, cb in adds:
        w.append((w[a] * ca + w[b] * cb) % q)
    return w


def levels(adds, n_witness):
    lv = []
    for i, (a, b, _, _) in enumerate(adds):
        assert a < n_witness + i and b < n_witness + i, i
        lv.append(max([0] + [lv[s - n_witness] + 1 for s in (a, b) if s >= n_witness]))
    return lv


def additions_by_level(w, adds, q):
    """the second formulation: every addition of level 0 from the witness alone, then level 1, and so on; within a level in any order"""
    n = len(w)
    lv = levels(adds, n)
    out = list(w) + [None] * len(adds)
    for l in range(max(lv) + 1 if lv else 0):
        batch = [i for i in range(len(adds)) if lv[i] == l]
        vals = [(out[adds[i][0]] * adds[i][2] + out[adds[i][1]] * adds[i][3]) % q for i in reversed(batch)]      # all reads before all writes
        for i, v in zip(reversed(batch), vals):
            out[n + i] = v
    return out


def plan(adds, n_witness):
    """what pil2gl_wtns_adds_plan emits: records (a, b, dst, source position) sorted by level, stable; levelStart"""
    lv = levels(adds, n_witness)
    order = sorted(range(len(adds)), key=lambda i: lv[i])
    n_levels = max(lv) + 1 if lv else 0
    start = [sum(1 for x in lv if x < l) for l in range(n_levels + 1)]
    return [(adds[i][0], adds[i][1], n_witness + i, i) for i in order], start, order


def gather(w, s_map, n_rows, n_cols, dst_cols, q):
    """[n_rows][dst_cols] integers: the fill loop, widened with zero columns (land_rows' rule); canonical"""
    return [[(w[s_map[i * n_cols + j]] % q if s_map[i * n_cols + j] else 0) if j < n_cols else 0 for j in range(dst_cols)] for i in range(n_rows)]


def trace(w, adds, s_map, n_rows, n_cols, q, dst_cols=None):
    return gather(additions(w, adds, q), s_map, n_rows, n_cols, dst_cols or n_cols, q)


def random_dag(rng, n_witness, n_adds, q, back=0.5):
    """additions whose operands name earlier additions with probability `back`"""
    adds = []
    for i in range(n_adds):
        ops = [rng.randrange(n_witness, n_witness + i) if i and rng.random() < back else rng.randrange(n_witness) for _ in range(2)]
        adds.append((ops[0], ops[1], rng.randrange(q), rng.randrange(q)))
    return adds


def queue_reduction(terms, n_witness, first_add=0):
    """r1cs2plonk.js:49-67: a linear combination of `terms` signals reduced through a queue -- two off the front, their sum to the back"""
    queue = list(terms)
    adds = []
    while len(queue) > 1:
        a, b = queue.pop(0), queue.pop(0)
        queue.append(n_witness + first_add + len(adds))
        adds.append((a, b, 3 + len(adds), 5 + 2 * len(adds)))
    return adds


# ---- words ----
def fr_words(vals):
    """[n] integers below 2^256 -> (n, 4) uint64, as they are"""
    a = np.zeros((len(vals), 4), np.uint64)
    for i, v in enumerate(vals):
        for k in range(4):
            a[i, k] = (int(v) >> (64 * k)) & 0xFFFFFFFFFFFFFFFF
    return a


def fr_ints(words):
    return [sum(int(x) << (64 * k) for k, x in enumerate(r)) for r in np.asarray(words, np.uint64).reshape(-1, 4)]


def to_mont(v):
    return v % R * MONT % R


# ---- file writers ----
def write_compressor_exec(path, adds, s_map, n_rows, n_cols):
    """flat u64: nAdds, nSMap, adds[4 nAdds] (a, b, ca, cb), sMap[nSMap nCols] row-major"""
    assert len(s_map) == n_rows * n_cols
    words = [len(adds), n_rows] + [x for rec in adds for x in rec] + list(s_map)
    with open(path, "wb") as f:
        f.write(np.array(words, np.uint64).tobytes())


def _binfile(path, kind, version, sections, n_sections=None):
    with open(path, "wb") as f:
        f.write(kind.encode() + struct.pack("<II", version, n_sections if n_sections is not None else len(sections)))
        for sid, payload in sections:
            f.write(struct.pack("<IQ", sid, len(payload)) + payload)


def write_final_exec(path, adds, s_map, n_rows, n_cols):
    """iden3 binfile "exec" version 1; the header says 5 sections (EXEC_NSECTIONS) and four are written: 2 = nAdds, nSMap; 3 = 2 nAdds u64
    operand indices; 4 = 2 nAdds 32-byte Montgomery coefficients; 5 = nSMap nCols u64.  `adds` carries the coefficients as VALUES."""
    assert len(s_map) == n_rows * n_cols
    idx = np.array([x for a, b, _, _ in adds for x in (a, b)], np.uint64)
    coef = fr_words([to_mont(c) for _, _, ca, cb in adds for c in (ca, cb)])
    _binfile(path, "exec", 1, [(2, struct.pack("<QQ", len(adds), n_rows)), (3, idx.tobytes()), (4, coef.tobytes()),
                               (5, np.array(s_map, np.uint64).tobytes())], n_sections=5)


def write_wtns(path, w, q=R, n8=32):
    """binfile "wtns" version 2: section 1 = u32 n8, the prime (n8 bytes), u32 nWitness; section 2 = the values, n8 bytes each, normal form"""
    head = struct.pack("<I", n8) + int(q).to_bytes(n8, "little") + struct.pack("<I", len(w))
    _binfile(path, "wtns", 2, [(1, head), (2, b"".join(int(v).to_bytes(n8, "little") for v in w))])


def rng(seed):
    return random.Random(seed)
