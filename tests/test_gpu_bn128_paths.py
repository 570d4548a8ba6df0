"""pil2gl_bn128_roots_from_group_proofs (MerkleHash.calculateRootFromGroupProof of merklehash_bn128_p.js:184-232 for a batch of
openings, one launch, a wave per opening) against oracle/bn128_oracle.py, bit for bit: every arity and sponge rule over the widths
and heights at which the path takes another branch, Montgomery-form siblings, non-canonical siblings, the ignored own-position
slot, tampering, the launch counter and the refusals."""
import ctypes as C
import functools

import numpy as np
import pytest

from conftest import rand_field

pytestmark = pytest.mark.gpu

EINVAL = -1


@pytest.fixture(scope="module")
def bn():
    import pil2gl
    pil2gl.init(0)
    from pil2gl import bn128
    return bn128


@pytest.fixture(scope="module")
def orc():
    import bn128_oracle
    return bn128_oracle


def _lib():
    from pil2gl import _lib as L
    return L.load()


def _p(a):
    return None if a is None or a.size == 0 else C.c_void_p(a.ctypes.data)


def words(vals):
    """ints < 2^256 -> [n][4] little-endian u64 words, as they are"""
    a = np.zeros((len(vals), 4), np.uint64)
    for i, v in enumerate(vals):
        assert 0 <= v < 1 << 256
        for k in range(4):
            a[i, k] = (v >> (64 * k)) & 0xFFFFFFFFFFFFFFFF
    return a


def ints(w):
    return [sum(int(x) << (64 * k) for k, x in enumerate(r)) for r in np.asarray(w, np.uint64).reshape(-1, 4)]


def raw_roots(vals, sib, width, levels, arity, custom, mont, idxs):
    """the C entry itself; vals [n][width] u64, sib [n*levels*arity][4] u64 -> (rc, [n] ints)"""
    n = len(idxs)
    vals = np.ascontiguousarray(vals, dtype=np.uint64)
    sib = np.ascontiguousarray(sib, dtype=np.uint64)
    ii = np.array(idxs, dtype=np.uint64)
    out = np.zeros((n, 4), np.uint64)
    rc = _lib().pil2gl_bn128_roots_from_group_proofs(_p(vals), _p(sib), width, levels, arity, int(custom), int(mont), _p(ii), n, _p(out))
    return rc, ints(out)


def n_levels(height, arity):
    nl, n = 0, height
    while n > 1:
        n = (n - 1) // arity + 1
        nl += 1
    return nl


def widths_of(arity):
    # 0: value 0 | 2: one partial element, unhashed | 3: one element | one full chunk, no last chunk | a last chunk of one element holding
    # one word (t = 2, or padded when custom) | a longer last chunk | two full chunks and a ragged tail
    return [0, 2, 3, 3 * arity, 3 * arity + 1, 3 * arity + 5, 3 * (2 * arity + 3) + 2]


def heights_of(arity):
    return [1, arity, arity + 1, 37]                  # no level | one full group | a ragged second level (missing siblings are 0) | several levels


@functools.lru_cache(maxsize=None)
def oracle_tree(width, height, arity, custom, seed=0):
    """(rows, node values in normal form) of a random tree, computed once per shape by the CPU oracle"""
    import bn128_oracle as orc
    rows = rand_field(np.random.default_rng(1000 * width + 10 * height + arity + seed), (height, width))
    if width == 0:
        nodes = orc.merkelize([[] for _ in range(height)], arity, custom)
    else:
        nodes = orc.c_merkelize(rows, arity, custom)
    return rows, nodes


def tree_root(nodes, height):
    """the node a path ends at.  A tree of ONE row has no level: its path ends at the leaf, nodes[0] -- the reference's layout pads that
    only level to `arity` nodes (_getNNodes, merklehash_bn128_p.js:31-45), so its last node, what root() reads, is a padding zero"""
    return nodes[0] if height == 1 else nodes[-1]


def opened_rows(height):
    return sorted({0, min(1, height - 1), height - 1, height // 2})


@pytest.mark.parametrize("custom", [False, True])
@pytest.mark.parametrize("arity", [2, 4, 8, 16])
def test_roots_across_shapes(bn, orc, arity, custom):
    for width in widths_of(arity):
        for height in heights_of(arity):
            rows, nodes = oracle_tree(width, height, arity, custom)
            idxs = opened_rows(height)
            lv = n_levels(height, arity)
            mps = [orc.group_proof(nodes, height, arity, i) for i in idxs]
            assert all(len(mp) == lv for mp in mps)
            rc, got = raw_roots(rows[idxs], words([s for mp in mps for g in mp for s in g]), width, lv, arity, custom, 0, idxs)
            assert rc == 0, _lib().pil2gl_last_error()
            for i, mp, g in zip(idxs, mps, got):
                want = orc.root_from_group_proof(mp, i, [int(v) for v in rows[i]], arity, custom)
                assert want == tree_root(nodes, height), (width, height, i)  # the oracle agrees with itself
                assert g == want, (arity, custom, width, height, i)
            # the Python mirror of the drop-in hands the same openings to the same entry
            MH = bn.buildMerkleHash(arity, custom)
            assert MH.calculateRootsFromGroupProofs([([int(v) for v in rows[i]], mp) for i, mp in zip(idxs, mps)], idxs) == got
            assert MH.verifyGroupProofs(tree_root(nodes, height), [([int(v) for v in rows[i]], mp) for i, mp in zip(idxs, mps)], idxs)


@pytest.mark.parametrize("height,arity", [(37, 4), (17, 16)])
def test_montgomery_chaining_every_row(bn, orc, height, arity):
    """what pil2gl_bn128_group_proofs_dev returns for EVERY row of a resident tree leads back to the tree's root: as returned (normal
    form, siblingsMontgomery = 0) and in the form tree.nodes holds (pil2gl_bn128_convert to Montgomery form, siblingsMontgomery = 1)"""
    import torch
    width = 9
    rows, nodes = oracle_tree(width, height, arity, False, seed=7)
    MH = bn.buildMerkleHash(arity, False)
    tree = MH.merkelize(torch.from_numpy(rows.reshape(-1).view(np.int64)).cuda(), width, height)
    assert MH.root(tree) == orc.root(nodes)
    lv, idxs = n_levels(height, arity), list(range(height))
    ii = np.array(idxs, dtype=np.uint64)
    vals = np.zeros((height, width), np.uint64); sib = np.zeros((height * lv * arity, 4), np.uint64); nl = C.c_uint32()
    rc = _lib().pil2gl_bn128_group_proofs_dev(C.c_void_p(tree["elements"].data_ptr()), C.c_void_p(tree["nodes"].data_ptr()), width, height, arity,
                                              _p(ii), height, _p(vals), _p(sib), C.byref(nl))
    assert rc == 0 and nl.value == lv
    assert (vals == rows).all()
    rc, got = raw_roots(vals, sib, width, lv, arity, False, 0, idxs)
    assert rc == 0 and got == [orc.root(nodes)] * height
    mont = np.zeros_like(sib)
    assert _lib().pil2gl_bn128_convert(_p(sib), sib.shape[0], 1, _p(mont)) == 0
    assert ints(mont[:1]) == [ints(sib[:1])[0] * orc.MONT_R % orc.R]
    rc, got = raw_roots(vals, mont, width, lv, arity, False, 1, idxs)
    assert rc == 0 and got == [orc.root(nodes)] * height
    # the nodes of the resident tree themselves, read where getGroupProof reads them, are those Montgomery words
    node_words = tree["nodes"].cpu().numpy().view(np.uint64).reshape(-1, 4)
    assert (mont[:arity] == node_words[:arity]).all()


def _one_opening(orc, width=11, height=37, arity=4, custom=True, idx=22):
    rows, nodes = oracle_tree(width, height, arity, custom, seed=3)
    mp = orc.group_proof(nodes, height, arity, idx)
    return rows, nodes, mp, n_levels(height, arity)


def test_non_canonical_siblings_are_reduced(orc):
    """a sibling given as v + r, or v + 4r (both < 2^256), yields the same root as v; so does a Montgomery word plus r"""
    width, height, arity, custom, idx = 11, 37, 4, True, 22
    rows, nodes, mp, lv = _one_opening(orc)
    flat = [s for g in mp for s in g]
    for k in (1, 4):
        assert max(flat) + k * orc.R < 1 << 256
        rc, got = raw_roots(rows[[idx]], words([s + k * orc.R for s in flat]), width, lv, arity, custom, 0, [idx])
        assert rc == 0 and got == [orc.root(nodes)], k
    mont = [s * orc.MONT_R % orc.R for s in flat]
    for k in (0, 1, 4):
        rc, got = raw_roots(rows[[idx]], words([m + k * orc.R for m in mont]), width, lv, arity, custom, 1, [idx])
        assert rc == 0 and got == [orc.root(nodes)], k


def test_own_position_slot_is_ignored(orc):
    width, height, arity, custom, idx = 11, 37, 4, True, 22
    rows, nodes, mp, lv = _one_opening(orc)
    pos = idx
    bad = [list(g) for g in mp]
    for level in range(lv):
        bad[level][pos & (arity - 1)] = (1 << 256) - 1 - level
        pos >>= 2
    for mont in (0, 1):
        sib = [s for g in bad for s in g]
        if mont:
            own = {(l * arity + ((idx >> (2 * l)) & 3)) for l in range(lv)}
            sib = [s if k in own else s * orc.MONT_R % orc.R for k, s in enumerate(sib)]
        rc, got = raw_roots(rows[[idx]], words(sib), width, lv, arity, custom, mont, [idx])
        assert rc == 0 and got == [orc.root(nodes)], mont


def test_tampering_changes_the_root(orc):
    width, height, arity, custom, idx = 11, 37, 4, True, 22
    rows, nodes, mp, lv = _one_opening(orc)
    good = words([s for g in mp for s in g])
    root = orc.root(nodes)
    rc, got = raw_roots(rows[[idx]], good, width, lv, arity, custom, 0, [idx])
    assert rc == 0 and got == [root]
    for col in (0, width - 1):                                        # one word of a value
        v = rows[[idx]].copy(); v[0, col] ^= np.uint64(1)
        rc, got = raw_roots(v, good, width, lv, arity, custom, 0, [idx])
        assert rc == 0 and got != [root], col
    pos = idx
    for level in range(lv):                                           # one word of a sibling that is not at the path's own position
        k = level * arity + ((pos & (arity - 1)) + 1) % arity
        s = good.copy(); s[k, level % 4] ^= np.uint64(1 << 17)
        rc, got = raw_roots(rows[[idx]], s, width, lv, arity, custom, 0, [idx])
        assert rc == 0 and got != [root], level
        pos >>= 2
    for bit in range(2 * lv):                                         # the index
        rc, got = raw_roots(rows[[idx]], good, width, lv, arity, custom, 0, [idx ^ (1 << bit)])
        assert rc == 0 and got != [root], bit


def test_one_launch_per_batch(bn, orc):
    """a batch of openings goes through the path kernel, ONCE -- not through a permutation call per sponge chunk and per level"""
    width, height, arity, custom = 11, 37, 4, True
    rows, nodes = oracle_tree(width, height, arity, custom, seed=3)
    MH = bn.buildMerkleHash(arity, custom)
    idxs = list(range(height)) * 3                                    # 111 openings: more than one wave's worth of lanes, one block each
    proofs = [([int(v) for v in rows[i]], orc.group_proof(nodes, height, arity, i)) for i in idxs]
    lib = _lib()
    before = lib.pil2gl_debug_bn128_path_launches()
    got = MH.calculateRootsFromGroupProofs(proofs, idxs)
    assert lib.pil2gl_debug_bn128_path_launches() == before + 1
    assert got == [orc.root(nodes)] * len(idxs)
    assert MH.calculateRootsFromGroupProofs([], []) == [] and lib.pil2gl_debug_bn128_path_launches() == before + 1


def test_refusals(bn):
    v = np.zeros((1, 3), np.uint64); s = np.zeros((41 * 16, 4), np.uint64)
    assert raw_roots(v, s, 3, 2, 3, False, 0, [0])[0] == EINVAL       # arity 3
    assert raw_roots(v, s, 3, 2, 32, False, 0, [0])[0] == EINVAL
    assert raw_roots(v, s, 3, 41, 4, False, 0, [0])[0] == EINVAL      # levels 41
    assert raw_roots(v, s, 3, 40, 4, False, 0, [0])[0] == 0
    assert raw_roots(v, s, 3, 2, 4, False, 0, [])[0] == 0             # nIdx = 0
    lib = _lib()
    out = np.zeros(4, np.uint64); ii = np.zeros(1, np.uint64)
    assert lib.pil2gl_bn128_roots_from_group_proofs(None, _p(s), 3, 2, 4, 0, 0, _p(ii), 1, _p(out)) == EINVAL      # null buffers with nIdx > 0
    assert lib.pil2gl_bn128_roots_from_group_proofs(_p(v), None, 3, 2, 4, 0, 0, _p(ii), 1, _p(out)) == EINVAL
    assert lib.pil2gl_bn128_roots_from_group_proofs(_p(v), _p(s), 3, 2, 4, 0, 0, None, 1, _p(out)) == EINVAL
    assert lib.pil2gl_bn128_roots_from_group_proofs(_p(v), _p(s), 3, 2, 4, 0, 0, _p(ii), 1, None) == EINVAL
    assert lib.pil2gl_bn128_roots_from_group_proofs(None, None, 0, 0, 4, 0, 0, _p(ii), 1, _p(out)) == 0 and not out.any()   # no value, no level: 0
