"""tests/merkle_ref.py against the C oracle on the CPU, and the two coverage claims that tests/test_gpu_merkle_edges.py relies on: the
width list reaches every shape the split leaf kernel can take, and the tree heights put an odd level at every depth that matters.
The oracle's behaviour on words at or above p is pinned here too, since the GPU file uses it as the reference for such words."""
import numpy as np
import pytest

import merkle_ref as mref
from merkle_ref import P

SPLITS = [False, True]


def test_num_nodes_and_level_sizes(oracle):
    for h in list(range(1, 70)) + mref.TREE_HEIGHTS:
        assert mref.num_nodes(h) == oracle.merkle_num_nodes(h), h
    assert mref.level_sizes(1) == [1] and mref.level_sizes(5) == [5, 3, 2, 1] and mref.level_sizes(8) == [8, 4, 2, 1]


@pytest.mark.parametrize("split", SPLITS)
def test_leaf_rule_equals_the_oracle(oracle, split):
    rng = np.random.default_rng(11)
    for w in mref.WIDTHS + [128, 131]:
        for row in mref.full_range(rng, (6, w)):
            assert mref.leaf(row, split) == oracle.linear_hash(row, split).tolist(), (w, split)
    assert mref.leaf([], split) == [0, 0, 0, 0]


@pytest.mark.parametrize("split", SPLITS)
def test_tree_rule_equals_the_oracle(oracle, split):
    rng = np.random.default_rng(12)
    for h in mref.TREE_HEIGHTS:
        if h > mref.REF_TREE_MAX:
            continue
        rows = mref.full_range(rng, (h, 9))
        assert np.array_equal(mref.tree(rows, split), oracle.merkelize(rows, split)), (h, split)
    for w, h in [(3, 33), (33, 65), (100, 17), (0, 5), (4, 1), (5, 1)]:
        rows = mref.full_range(rng, (h, w))
        assert np.array_equal(mref.tree(rows, split), oracle.merkelize(rows, split)), (w, h, split)
    one = oracle.merkelize(mref.full_range(rng, (1, 9)), split)
    assert one.size == 8 and not one[4:].any(), "the 1-row quirk: the words read as the root stay zero"


def test_noncanonical_generator():
    rng = np.random.default_rng(13)
    a = mref.noncanonical(rng, (513, 9))
    frac = (a >= np.uint64(P)).mean()
    assert 0.25 < frac < 0.42
    assert all((a == np.uint64(v)).any() for v in (P, P + 1, mref.TOP))
    b = mref.noncanonical(rng, (64, 13), cols=[2, 12])
    high = (b >= np.uint64(P))
    assert high[:, [2, 12]].any(axis=0).all() and not np.delete(high, [2, 12], axis=1).any()
    assert all((b[:, [2, 12]] == np.uint64(v)).any() for v in (P, P + 1, mref.TOP))
    assert (mref.residues(a) < np.uint64(P)).all() and ((a - mref.residues(a)) % np.uint64(P) == 0).all()
    assert mref.noncanonical(rng, (5, 0)).shape == (5, 0)


@pytest.mark.parametrize("split", SPLITS)
def test_rows_above_p_hash_to_the_hash_of_their_residues(oracle, split):
    """widths above 4: every word goes through the permutation, which reduces it; the digest is canonical"""
    rng = np.random.default_rng(14)
    for w in [x for x in mref.WIDTHS if x > 4]:
        rows = mref.noncanonical(rng, (8, w), mref.noncanonical_columns(w, split))
        assert (rows >= np.uint64(P)).any()
        for row in rows:
            d = oracle.linear_hash(row, split)
            assert d.tolist() == oracle.linear_hash(mref.residues(row), split).tolist() == mref.leaf(row, split), (w, split)
            assert (d < np.uint64(P)).all()


@pytest.mark.parametrize("split", SPLITS)
def test_passthrough_rows_come_through_raw(oracle, split):
    """widths up to 4: the words are the digest as they are; the level above hashes residues, so the tree above equals the tree above the residues"""
    rng = np.random.default_rng(15)
    for w in (1, 3, 4):
        for h in (1, 2, 5, 33):
            rows = mref.noncanonical(rng, (h, w))
            t = oracle.merkelize(rows, split)
            want = np.zeros((h, 4), np.uint64)
            want[:, :w] = rows
            assert np.array_equal(t[:4 * h].reshape(h, 4), want), (w, h)
            assert np.array_equal(t, mref.tree(rows, split))
            tr = oracle.merkelize(mref.residues(rows), split)
            lv = 4 * (h + (h & 1))
            assert np.array_equal(t[lv:], tr[lv:]), (w, h)
            if h > 1:
                assert (t[lv:] < np.uint64(P)).all()


def test_widths_reach_every_split_shape():
    """(batch count, class of the last batch) over widths 9..128, enumerated from split_shape: WIDTHS has a width of every pair"""
    pairs = {mref.split_shape(w) for w in range(9, 129)}
    assert len(pairs) >= 7 and {c for _, c in pairs} == {mref.DIGEST, mref.ONE_CHUNK, mref.CHUNKS} and {n for n, _ in pairs} == {2, 3, 4}
    have = {mref.split_shape(w) for w in mref.WIDTHS if w > 8}
    assert pairs <= have, sorted(pairs - have)
    # the rule itself, at widths worked out by hand
    assert mref.split_shape(9) == (2, mref.DIGEST) and mref.split_shape(32) == (4, mref.ONE_CHUNK)
    assert mref.split_shape(33) == (4, mref.ONE_CHUNK) and mref.split_shape(36) == (4, mref.CHUNKS) and mref.split_shape(100) == (4, mref.CHUNKS)
    # and the plain widths on either side of the passthrough and of one chunk
    assert {0, 1, 4, 5, 8} <= set(mref.WIDTHS)
    # the columns named for words at or above p: whole passthrough rows, whole small last batches, first and last chunks
    assert mref.noncanonical_columns(3, True) == [0, 1, 2]
    assert mref.noncanonical_columns(9, True) == list(range(9))
    assert mref.noncanonical_columns(100, True) == sorted(set(sum([list(range(s, s + 8)) + [s + 24] for s in (0, 25, 50, 75)], [])))
    assert mref.noncanonical_columns(100, False) == list(range(8)) + [96, 97, 98, 99]


def test_tree_heights_reach_the_odd_levels():
    """from the level sizes: some tree is odd first at depth 0, one first at depth 1, one first at depth 2, and one has the level of three
    digests -- the highest level that can be odd, since the two under the root never are -- below at least three others"""
    first_odd, three_deep = set(), False
    for h in mref.TREE_HEIGHTS:
        s = mref.level_sizes(h)
        odd = [d for d, n in enumerate(s[:-1]) if n & 1]
        assert all(s[d] > 1 for d in odd) or h == 1
        if odd and h > 1:
            first_odd.add(odd[0])
            three_deep |= s[odd[-1]] == 3 and odd[-1] >= 3
    assert {0, 1, 2} <= first_odd
    assert three_deep
    # a padded level on a level-kernel launch of more than one workgroup, and a tree with no odd level at all
    assert any(n & 1 and n > 512 for h in mref.TREE_HEIGHTS for n in mref.level_sizes(h)[1:])
    assert any(not any(n & 1 for n in mref.level_sizes(h)[:-1]) for h in mref.TREE_HEIGHTS if h > 1)


@pytest.mark.parametrize("split", SPLITS)
def test_every_row_of_an_odd_tree_opens_to_the_root(oracle, split):
    h, w = 37, 9                                              # 37, 19, 10, 5, 3, 2, 1: four odd levels
    assert sum(n & 1 for n in mref.level_sizes(h)[:-1]) == 4
    rows = mref.full_range(np.random.default_rng(16), (h, w))
    t = oracle.merkelize(rows, split)
    for i in range(h):
        sib = oracle.group_proof(t, h, i)
        assert sib.shape == (len(mref.level_sizes(h)) - 1, 4)
        assert oracle.root_from_proof(rows[i], i, sib, split).tolist() == t[-4:].tolist(), i
    bad = rows[36].copy(); bad[0] ^= np.uint64(1)
    assert oracle.root_from_proof(bad, 36, oracle.group_proof(t, h, 36), split).tolist() != t[-4:].tolist()
