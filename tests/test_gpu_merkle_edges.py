"""The Goldilocks hashing unit (csrc/merkle.hip) compared in whole: every digest of the leaf kernels, every op of the level kernel, every
node of a tree, every value and sibling of a batch of openings, every root of the batched path walk, at the launch edges (the 64-lane
wave, the 256-row plain and 512-row split workgroups, ragged last workgroups), at every shape the split form can take, on full-range
words and on words at or above p, into destinations that were dirty before and are guarded after, on a stream that is not the default.
Every comparison is exact equality of 64-bit words.  The reference is the C oracle on the same raw words (tests/test_merkle_ref_cpu.py
pins what it does with words at or above p and checks it against tests/merkle_ref.py); the shapes are merkle_ref's lists."""
import ctypes as C

import numpy as np
import pytest

import merkle_ref as mref
from merkle_ref import P

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from pil2gl import _lib  # noqa: E402

GUARD = 0xFFFFFFFFDEADBEEF                            # the sentinel of dirty destinations and guard words
NG = 64                                               # guard words behind an output
PU = np.uint64(P)


@pytest.fixture(scope="module")
def gl():
    import pil2gl
    pil2gl.init(0)
    yield pil2gl
    _TREES.clear()                                    # the shared trees leave the device with this module
    _SIDE.clear()
    torch.cuda.synchronize()


# ---- helpers ----
def to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).reshape(-1).view(np.int64)).cuda()


def to_host(d):
    return d.cpu().numpy().view(np.uint64)


def dirty(words):
    return to_dev(np.full(words + NG, GUARD, np.uint64))


def ptr(d):
    return C.c_void_p(d.data_ptr() if d.numel() else 0)


def cur_stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def first_bad(got, want, per):
    bad = np.flatnonzero((got != want).reshape(-1, per).any(axis=1))
    return "%d of %d differ, first %d" % (bad.size, got.size // per, bad[0]) if bad.size else ""


def check(buf, want, what, per=4):
    """the first want.size words of a dirty() buffer equal `want`, the guard words behind them were not written"""
    got = to_host(buf)
    assert got.size == want.size + NG
    assert np.array_equal(got[:want.size], want), "%s: %s" % (what, first_bad(got[:want.size], want, per))
    assert (got[want.size:] == GUARD).all(), what + ": a word past the output was written"


def make_rows(rng, h, w, kind, split):
    if kind == "canonical":
        return mref.full_range(rng, (h, w))
    return mref.noncanonical(rng, (h, w), mref.noncanonical_columns(w, split))


_SIDE = []


def on_side_stream(fn):
    """run fn(stream handle) on a stream that is not the default one, after everything queued so far, and wait for it"""
    if not _SIDE:
        _SIDE.append(torch.cuda.Stream())             # one stream for the whole module
    s = _SIDE[0]
    assert s.cuda_stream != torch.cuda.default_stream().cuda_stream
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        fn(C.c_void_p(s.cuda_stream))
    s.synchronize()


# ---- leaf kernels: every row ----
@pytest.mark.parametrize("kind", ["canonical", "noncanonical"])
@pytest.mark.parametrize("split", [False, True])
def test_leaf_kernels_every_row(gl, oracle, split, kind):
    rng = np.random.default_rng(100 + 2 * split + (kind != "canonical"))
    for w, h in mref.leaf_shapes():
        rows = make_rows(rng, h, w, kind, split)
        if kind != "canonical" and w:
            assert (rows >= PU).any()
        want = oracle.merkelize(rows, split)[:4 * h]
        d_in, out = to_dev(rows), dirty(4 * h)
        _lib.call("pil2gl_linear_hash_rows_dev", ptr(d_in), w, h, int(split), ptr(out), cur_stream())
        check(out, want, "leaves of %d x %d, split %d, %s" % (h, w, split, kind))
        assert np.array_equal(to_host(d_in), rows.reshape(-1)), "the input was written"
        if w > 4:
            assert (want < PU).all()
        elif w:
            assert np.array_equal(want.reshape(h, 4)[:, :w], rows) and not want.reshape(h, 4)[:, w:].any()


# ---- level kernel: every op ----
@pytest.mark.parametrize("kind", ["canonical", "noncanonical"])
def test_level_kernel_every_op(gl, oracle, kind):
    rng = np.random.default_rng(7 + (kind != "canonical"))
    for n_ops in (1, 255, 256, 257, 1000):
        a = mref.full_range(rng, (n_ops, 8)) if kind == "canonical" else mref.noncanonical(rng, (n_ops, 8))
        want = np.array([oracle.poseidon(r, None, 4) for r in a], dtype=np.uint64).reshape(-1)
        assert (want < PU).all()
        d_in, out = to_dev(a), dirty(4 * n_ops)
        _lib.call("pil2gl_merkelize_level_dev", ptr(d_in), n_ops, ptr(out), cur_stream())
        check(out, want, "%d ops, %s" % (n_ops, kind))
        assert np.array_equal(to_host(d_in), a.reshape(-1)), "the input was written"
        assert np.array_equal(gl.merkelizeLevel(a), want), "the host form differs"


# ---- trees: every node ----
def build_tree(rows, split, nodes):
    """pil2gl_merkelize_dev itself, on a side stream -> the rows on the device"""
    h, w = rows.shape
    d_in = to_dev(rows)
    on_side_stream(lambda s: _lib.call("pil2gl_merkelize_dev", ptr(d_in), w, h, int(split), ptr(nodes), s))
    return d_in


def level_offsets(h):
    off, out = 0, []
    for n in mref.level_sizes(h):
        out.append(off)
        off += 4 * (n + (n & 1))
    return out


TREE_CASES = [
    (9, False, "canonical", mref.TREE_HEIGHTS),
    (9, True, "canonical", mref.TREE_HEIGHTS),
    (33, True, "canonical", [1, 2, 3, 5, 12, 33, 257, 511, 513, 1000, 4097]),
    (3, False, "noncanonical", [1, 2, 3, 5, 12, 33, 257, 513, 1000, 1028, 4097]),
    (3, True, "noncanonical", [1, 5, 513, 4097]),
]


@pytest.mark.parametrize("w,split,kind,heights", TREE_CASES, ids=["w9-plain", "w9-split", "w33-split", "w3-plain-above-p", "w3-split-above-p"])
def test_tree_every_node_on_a_side_stream_into_a_dirty_buffer(gl, oracle, w, split, kind, heights):
    assert set(heights) <= set(mref.TREE_HEIGHTS)
    rng = np.random.default_rng(1000 + w + split)
    for h in heights:
        rows = make_rows(rng, h, w, kind, split)
        want = oracle.merkelize(rows, split)
        n = int(_lib.load().pil2gl_merkle_num_nodes(h))
        assert want.size == n == mref.num_nodes(h)
        nodes = dirty(n)
        d_in = build_tree(rows, split, nodes)
        check(nodes, want, "tree of %d x %d, split %d, %s" % (h, w, split, kind))
        assert np.array_equal(to_host(d_in), rows.reshape(-1)), "the input was written"
        for lv, sz in zip(level_offsets(h), mref.level_sizes(h)[:-1]):          # the padding of every odd level is zero (part of `want`; said aloud)
            if sz & 1:
                assert not want[lv + 4 * sz:lv + 4 * sz + 4].any(), (h, sz)


@pytest.mark.parametrize("split", [False, True])
def test_tree_built_again_into_the_same_buffer(gl, oracle, split):
    """one buffer, never cleared: each build leaves its own tree in the first num_nodes words -- odd-level padding that an earlier, other
    tree filled with digests is zero again -- and leaves every word past them as the build before left it"""
    rng = np.random.default_rng(31 + split)
    biggest = mref.num_nodes(1000)
    nodes = dirty(biggest)
    before = to_host(nodes).copy()
    for h in (1000, 1000, 513, 999, 33, 5, 1, 1000):
        rows = mref.full_range(rng, (h, 9))
        want = oracle.merkelize(rows, split)
        build_tree(rows, split, nodes)
        got = to_host(nodes)
        assert np.array_equal(got[:want.size], want), "tree of %d rows over an older one: %s" % (h, first_bad(got[:want.size], want, 4))
        assert np.array_equal(got[want.size:], before[want.size:]), "a word past the tree of %d rows was written" % h
        before = got.copy()


@pytest.mark.parametrize("kind", ["canonical", "noncanonical"])
def test_digest_trees_into_a_dirty_buffer(gl, oracle, kind):
    """pil2gl_merkelize_digests_dev: the leaves are the caller's; a width-4 tree of the oracle is the tree over such digests"""
    rng = np.random.default_rng(41 + (kind != "canonical"))
    for h in (1, 2, 3, 5, 12, 33, 257, 513, 1000, 1028, 4097):
        dig = mref.full_range(rng, (h, 4)) if kind == "canonical" else mref.noncanonical(rng, (h, 4))
        want = oracle.merkelize(dig, False)
        assert np.array_equal(want[:4 * h], dig.reshape(-1))
        nodes = dirty(want.size)
        nodes[:4 * h] = to_dev(dig)
        on_side_stream(lambda s: _lib.call("pil2gl_merkelize_digests_dev", ptr(nodes), h, s))
        check(nodes, want, "digest tree of %d, %s" % (h, kind))
        if h == 1028:                                         # and through the wrapper, twice from the same leaves
            MH = gl.buildMerkleHash(False)
            for _ in range(2):
                assert np.array_equal(to_host(MH.merkelizeDigests(to_dev(dig), h)), want)


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("w", [3, 9])
def test_one_row_tree_quirk(gl, oracle, w, split):
    """merklehash_p.js:28-42,87: 8 words, the leaf and four zero words that are read as the root; no siblings"""
    rows = mref.full_range(np.random.default_rng(w), (1, w))
    nodes = dirty(8)
    d_in = build_tree(rows, split, nodes)
    want = np.concatenate([oracle.linear_hash(rows[0], split), np.zeros(4, np.uint64)])
    check(nodes, want, "1-row tree")
    assert np.array_equal(want, oracle.merkelize(rows, split))
    MH = gl.buildMerkleHash(split)
    tree = {"elements": d_in, "nodes": nodes[:8], "width": w, "height": 1}
    assert MH.root(tree) == [0, 0, 0, 0]
    assert MH.getGroupProof(tree, 0) == (rows[0].tolist(), [])
    assert MH.getGroupProofs(tree, [0, 0]) == [(rows[0].tolist(), []), (rows[0].tolist(), [])]


# ---- openings ----
_TREES = {}


def resident_tree(gl, oracle, h, w, split, small=False):
    """a tree on the device and the oracle's tree over the same rows, built once and never written.  small: half of the words are below
    2^32 - 1, so that adding p to them stays below 2^64"""
    key = (h, w, split, small)
    if key not in _TREES:
        rng = np.random.default_rng(h * 131 + w * 2 + split)
        pols = mref.full_range(rng, (h, w))
        if small:
            pols = np.where(rng.random((h, w)) < 0.5, pols & np.uint64(0x7FFFFFFF), pols)
        MH = gl.buildMerkleHash(split)
        tree = MH.merkelize(to_dev(pols), w, h)
        torch.cuda.synchronize()
        nodes = oracle.merkelize(pols, split)
        assert np.array_equal(to_host(tree["nodes"]), nodes)
        levels = len(mref.level_sizes(h)) - 1
        sib = np.zeros((h, levels, 4), np.uint64)
        for i in range(h):
            sib[i] = oracle.group_proof(nodes, h, i)
        pols.setflags(write=False); nodes.setflags(write=False); sib.setflags(write=False)
        _TREES[key] = (MH, tree, pols, nodes, sib)
    return _TREES[key]


def shuffled_with_repeats(rng, h):
    """every row once, in shuffled order, then about an eighth of them again at random places, two of them next to themselves"""
    idx = list(rng.permutation(h))
    for r in rng.integers(0, h, max(2, h // 8)):
        idx.insert(int(rng.integers(0, len(idx) + 1)), int(r))
    idx.insert(3, idx[3])
    idx.append(idx[-1])
    return [int(i) for i in idx]


@pytest.mark.parametrize("w", [1, 63, 64, 65, 129])
@pytest.mark.parametrize("h", [1000, 4097])
def test_group_proofs_open_every_row(gl, oracle, h, w):
    MH, tree, pols, nodes, sib = resident_tree(gl, oracle, h, w, False)
    rng = np.random.default_rng(h + w)
    idx = shuffled_with_repeats(rng, h)
    assert set(idx) == set(range(h)) and len(idx) > h + 2

    def opened(ii):
        pr = MH.getGroupProofs(tree, ii)
        assert len(pr) == len(ii)
        return np.array([v for v, _ in pr], dtype=np.uint64).reshape(len(ii), w), np.array([s for _, s in pr], dtype=np.uint64).reshape(len(ii), -1, 4)
    vals, sibs = opened(idx)
    assert np.array_equal(vals, pols[idx]), "values: " + first_bad(vals, pols[idx], w)
    assert np.array_equal(sibs, sib[idx]), "siblings: " + first_bad(sibs, sib[idx], sib.shape[1] * 4)
    few = [h - 1, 0, h - 1, 1, h // 2, 0, h - 2]                     # a smaller call into the same working buffer, then the large one again
    v2, s2 = opened(few)
    assert np.array_equal(v2, pols[few]) and np.array_equal(s2, sib[few])
    v3, s3 = opened(idx)
    assert np.array_equal(v3, vals) and np.array_equal(s3, sibs)
    assert np.array_equal(to_host(tree["nodes"]), nodes) and np.array_equal(to_host(tree["elements"]), pols.reshape(-1)), "the tree was written"
    i = idx[5]
    assert MH.getGroupProof(tree, i) == (pols[i].tolist(), sib[i].tolist())


# ---- the batched path walk ----
PATH_TREES = [(3, False), (9, True), (33, True)]
H_PATH = 4097


def packed_openings(pols, sib, idx):
    idx = np.asarray(idx)
    return np.ascontiguousarray(np.concatenate([pols[idx], sib[idx].reshape(len(idx), -1)], axis=1))


def walk(packed, w, levels, idx, split):
    ii = np.array(idx, dtype=np.uint64)
    roots = np.full((len(idx), 4), GUARD, np.uint64)
    _lib.call("pil2gl_roots_from_group_proofs", C.c_void_p(packed.ctypes.data), w, levels, C.c_void_p(ii.ctypes.data), len(idx), int(split),
              C.c_void_p(roots.ctypes.data))
    return roots


@pytest.mark.parametrize("w,split", PATH_TREES)
def test_path_walk_every_root(gl, oracle, w, split):
    MH, tree, pols, nodes, sib = resident_tree(gl, oracle, H_PATH, w, split, small=True)
    root = nodes[-4:]
    assert MH.root(tree) == root.tolist()
    order = [int(i) for i in np.random.default_rng(w).permutation(H_PATH)]
    ref = np.array([oracle.root_from_proof(pols[i], i, sib[i], split) for i in order], dtype=np.uint64)
    assert (ref == root).all()
    for count in (1, 255, 256, 257, H_PATH):
        idx = order[:count]
        proofs = [(pols[i].tolist(), sib[i].tolist()) for i in idx]
        roots = np.array(MH.calculateRootsFromGroupProofs(proofs, idx), dtype=np.uint64)
        assert roots.shape == (count, 4)
        assert np.array_equal(roots, ref[:count]), "%d openings: %s" % (count, first_bad(roots, ref[:count], 4))
        assert MH.verifyGroupProofs(root.tolist(), proofs, idx)
        assert np.array_equal(walk(packed_openings(pols, sib, idx), w, sib.shape[1], idx, split), roots)


@pytest.mark.parametrize("w,split", PATH_TREES)
def test_path_walk_one_flipped_bit_changes_one_root(gl, oracle, w, split):
    MH, tree, pols, nodes, sib = resident_tree(gl, oracle, H_PATH, w, split, small=True)
    levels = sib.shape[1]
    rng = np.random.default_rng(50 + w)
    order = [int(i) for i in rng.permutation(H_PATH)]
    for count, qs in ((257, (0, 255, 256)), (H_PATH, (0, 63, 64, 2047, 4095, 4096))):
        idx = order[:count]
        good = packed_openings(pols, sib, idx)
        base = walk(good, w, levels, idx, split)
        assert (base == nodes[-4:]).all()
        for k, q in enumerate(qs):
            col = int(rng.integers(0, w)) if k % 2 == 0 else w + int(rng.integers(0, 4 * levels))     # a value, or a word of a sibling
            if k == len(qs) - 1:
                col = w + 4 * (levels - 1) + 3                                                        # the last word of the last sibling
            bad = good.copy()
            bad[q, col] ^= np.uint64(1) << np.uint64(int(rng.integers(0, 32)))
            got = walk(bad, w, levels, idx, split)
            want = oracle.root_from_proof(bad[q, :w], idx[q], bad[q, w:], split)
            assert got[q].tolist() == want.tolist() != base[q].tolist(), (count, q, col)
            assert np.array_equal(np.delete(got, q, axis=0), np.delete(base, q, axis=0)), (count, q, col)


@pytest.mark.parametrize("w,split", PATH_TREES)
def test_path_walk_other_representatives(gl, oracle, w, split):
    """values and siblings replaced by word + p wherever that stays below 2^64: the same residues, so the same roots -- above width 4
    because the permutation reduces its input, up to width 4 because the path kernel canonicalises the leaf it is given"""
    MH, tree, pols, nodes, sib = resident_tree(gl, oracle, H_PATH, w, split, small=True)
    levels = sib.shape[1]
    order = [int(i) for i in np.random.default_rng(60 + w).permutation(H_PATH)]
    for count in (257, H_PATH):
        idx = order[:count]
        good = packed_openings(pols, sib, idx)
        fits = good < np.uint64((1 << 32) - 1)
        other = np.where(fits, good + PU, good)
        assert np.array_equal(mref.residues(other), good) and (other >= good).all()
        assert fits[:, :w].mean() > 0.4, "about half of the values take another representative"
        if w <= 4:
            assert fits[:, w:w + 4].any(), "and so do level-0 siblings, which are raw rows"
        got = walk(other, w, levels, idx, split)
        assert np.array_equal(got, walk(good, w, levels, idx, split)) and (got == nodes[-4:]).all()
        q = count - 1
        assert oracle.root_from_proof(other[q, :w], idx[q], other[q, w:], split).tolist() == nodes[-4:].tolist()


@pytest.mark.parametrize("w,split", [(3, False), (4, True), (5, False), (9, False), (9, True), (33, True)])
def test_path_walk_of_no_levels(gl, oracle, w, split):
    """height 1: an opening has no siblings and its root is the leaf hash -- 257 such openings in one call"""
    rows = mref.full_range(np.random.default_rng(70 + w), (257, w))
    want = np.array([oracle.root_from_proof(r, 0, np.zeros((0, 4), np.uint64), split) for r in rows], dtype=np.uint64)
    assert np.array_equal(want, np.array([oracle.linear_hash(r, split) for r in rows], dtype=np.uint64))
    assert np.array_equal(walk(rows, w, 0, [0] * 257, split), want)
    MH = gl.buildMerkleHash(split)
    assert MH.calculateRootsFromGroupProofs([(rows[0].tolist(), [])], [0]) == [want[0].tolist()]


# ---- single permutations and the chain ----
def test_poseidon_batch_on_words_above_p(gl, oracle):
    rng = np.random.default_rng(80)
    for count in (1, 256, 257):
        inp, cap = mref.noncanonical(rng, (count, 8)), mref.noncanonical(rng, (count, 4))
        want = np.array([oracle.poseidon(i, c, 12) for i, c in zip(inp, cap)], dtype=np.uint64)
        assert np.array_equal(want, np.array([oracle.poseidon(i, c, 12) for i, c in zip(mref.residues(inp), mref.residues(cap))], dtype=np.uint64))
        got = gl.poseidon_batch(inp, cap, 12)
        assert np.array_equal(got, want), first_bad(got, want, 12)
        got = gl.poseidon_batch(inp, None, 12)
        assert np.array_equal(got, np.array([oracle.poseidon(i, None, 12) for i in inp], dtype=np.uint64))


def test_sponge_chain_on_words_above_p(gl, oracle):
    rng = np.random.default_rng(81)
    for n_blocks in (1, 2, 97):
        blocks, cap = mref.noncanonical(rng, (n_blocks, 8)), mref.noncanonical(rng, (4,))
        assert (blocks >= PU).any() and (cap >= PU).any()
        st = cap
        for b in blocks:
            st = oracle.poseidon(b, st[:4], 12)
        out = np.full(12 + 4, GUARD, np.uint64)
        _lib.call("pil2gl_sponge_absorb", C.c_void_p(blocks.ctypes.data), n_blocks, C.c_void_p(cap.ctypes.data), C.c_void_p(out.ctypes.data))
        assert out[:12].tolist() == st.tolist() and (out[12:] == GUARD).all(), n_blocks


# ---- host forms ----
def test_host_forms_equal_the_resident_forms(gl, oracle):
    h, w, split = 1000, 33, True
    rows = mref.full_range(np.random.default_rng(90), (h, w))
    want = oracle.merkelize(rows, split)
    MH = gl.buildMerkleHash(split)
    resident = MH.merkelize(to_dev(rows), w, h)["nodes"]
    host = np.full(want.size + NG, GUARD, np.uint64)
    _lib.call("pil2gl_merkelize", C.c_void_p(rows.ctypes.data), w, h, int(split), C.c_void_p(host.ctypes.data))
    assert np.array_equal(host[:want.size], to_host(resident)) and np.array_equal(host[:want.size], want) and (host[want.size:] == GUARD).all()
    leaves = np.full(4 * h + NG, GUARD, np.uint64)
    _lib.call("pil2gl_linear_hash_rows", C.c_void_p(rows.ctypes.data), w, h, int(split), C.c_void_p(leaves.ctypes.data))
    assert np.array_equal(leaves[:4 * h], to_host(gl.linearHash(to_dev(rows), w, split))) and np.array_equal(leaves[:4 * h], want[:4 * h])
    assert (leaves[4 * h:] == GUARD).all()
    assert np.array_equal(MH.merkelize(rows, w, h)["nodes"], want) and np.array_equal(gl.linearHash(rows, w, split), want[:4 * h])
