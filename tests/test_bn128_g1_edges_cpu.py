"""The operands of tests/test_gpu_bn128_g1_edges.py and the facts that file relies on, without a device: the chosen stored values are
what their names claim, and on the curve y^2 = x^3 + b' through an arbitrary pair (x, y) the checker's b-free add / mul form a group in
which scalars act as integers, (x, 0) has order 2 and (0, y) has order 3."""
import random

import numpy as np
import pytest

import bn128_g1_chosen as ch
import bn128_g1_ref as ref
from bn128_g1_chosen import BY_NAME, STORED, Y_SUBSET
from bn128_g1_ref import MONT, Q, R

FULL = 0xffffffff


# ---- the operands ---------------------------------------------------------------------------------------------------------------------
def test_stored_values_are_distinct_canonical_and_what_their_names_claim():
    assert len(STORED) == 16 and len(set(STORED)) == 16
    assert all(1 <= v <= Q - 1 for v in STORED)
    assert set(Y_SUBSET) <= set(STORED) and len(set(Y_SUBSET)) >= 6
    L, ql = ch.limbs, ch.limbs(Q)
    assert L(BY_NAME["1"]) == [1] + [0] * 7 and L(BY_NAME["2"]) == [2] + [0] * 7
    assert L(BY_NAME["q-1"]) == [ql[0] - 1] + ql[1:] and L(BY_NAME["q-2"]) == [ql[0] - 2] + ql[1:]
    assert 2 * BY_NAME["(q-1)/2"] + 1 == Q and BY_NAME["(q+1)/2"] == BY_NAME["(q-1)/2"] + 1
    assert ch.value_of(BY_NAME["2^256 mod q"]) == 1 and ch.value_of(BY_NAME["2^512 mod q"]) == MONT % Q
    assert L(BY_NAME["ones7"]) == [FULL] * 7 + [ql[7] - 1]
    assert BY_NAME["ones7"] + BY_NAME["q-ones7"] == Q and L(BY_NAME["q-ones7"])[7] == 0
    assert L(BY_NAME["2^224"]) == [0] * 7 + [1] and L(BY_NAME["2^224-1"]) == [FULL] * 7 + [0]
    assert L(BY_NAME["2^32"]) == [0, 1] + [0] * 6 and L(BY_NAME["2^32-1"]) == [FULL] + [0] * 7
    assert BY_NAME["X+1"] == BY_NAME["X"] + 1 and all(0 < limb < FULL for limb in L(BY_NAME["X"]))
    assert L(BY_NAME["2^224"] - BY_NAME["1"]) == [FULL] * 7 + [0]    # the borrow of limb 0 is handed up through every limb
    assert L((BY_NAME["1"] - BY_NAME["2^224"]) % (1 << 256))[7] == FULL      # the other way round it leaves the top: q is added back
    assert L(BY_NAME["ones7"])[:7] == L(BY_NAME["2^224-1"])[:7]      # this pair differs in the top limb only


def test_stored_words_are_written_as_they_are():
    pairs = [(STORED[i], STORED[(i + 5) % 16]) for i in range(16)] + [None, (BY_NAME["X"], 0), (0, BY_NAME["q-1"])]
    w = ch.stored_point_words(pairs)
    assert w.shape == (19, 8) and w.dtype == np.uint64 and not w[16].any()
    for row, p in zip(w, pairs):
        raw = row.tobytes()
        assert (int.from_bytes(raw[:32], "little"), int.from_bytes(raw[32:], "little")) == (p or (0, 0))
    points = [ch.point_of_stored(*p) if p else None for p in pairs]
    assert np.array_equal(w, ref.point_words(points))                # value -> Montgomery gives the chosen bytes back
    assert [ch.stored_of(p) for p in points] == pairs
    assert [ref.point_of(r) for r in w] == points
    assert all(ch.value_of(v * MONT % Q) == v for v in (0, 1, 2, Q - 1))
    with pytest.raises(AssertionError):
        ch.stored_point_words([(Q, 1)])


def test_chord_pairs_cover_every_ordered_pair_of_x_and_none_shares_an_x():
    pairs = ch.chord_pairs()
    assert len(pairs) == 16 * 15
    assert {(a[0], b[0]) for a, b in pairs} == {(u, v) for u in STORED for v in STORED if u != v}
    for a, b in pairs:
        assert a[0] != b[0] or b[1] in (a[1], (Q - a[1]) % Q)       # a same-x pair with another y is on no common curve
        assert all(v in STORED for v in a + b)
    assert {a[1] for a, _ in pairs} == set(STORED) == {b[1] for _, b in pairs}      # y cycles through all of STORED on both sides
    xs = {(a[0], b[0]) for a, b in pairs}
    for u, v in (("X", "X+1"), ("X+1", "X"), ("2^224", "1"), ("1", "2^224"), ("ones7", "2^224-1"), ("q-1", "(q-1)/2")):
        assert (BY_NAME[u], BY_NAME[v]) in xs


# ---- the group law off the curve ------------------------------------------------------------------------------------------------------
def some_points(count, seed):
    rng = random.Random(seed)
    pts = [ch.point_of_stored(sx, sy) for sx in STORED for sy in Y_SUBSET]
    return rng.sample(pts, count)


def test_section_a_points_are_off_the_curve():
    pts = [ch.point_of_stored(sx, sy) for sx in STORED for sy in Y_SUBSET]
    assert len(set(pts)) == 16 * len(Y_SUBSET)
    assert not any(ref.on_curve(p) for p in pts)
    # b' = 0 only for the value pair (1, 1): y^2 = x^3 is singular at (0, 0) alone, its other points form a group under the same formulas
    assert [p for p in pts if ch.curve_b(p) == 0] == [(1, 1)]
    assert all(ref.add(ref.mul(a, (1, 1)), ref.mul(b, (1, 1))) == ref.mul(a + b, (1, 1)) for a, b in ((1, 1), (2, 1), (15, 241), (R - 1, R - 2)))


def test_scalars_act_as_integers_on_an_arbitrary_point():
    rng = random.Random(11)
    for p in some_points(12, 1):
        a, b = rng.randrange(R), rng.randrange(R)
        assert ref.add(ref.mul(a, p), ref.mul(b, p)) == ref.mul(a + b, p)
        assert ref.add(p, p) == ref.mul(2, p) and ref.add(ref.mul(2, p), p) == ref.mul(3, p)
        assert ch.curve_b(ref.mul(a, p)) == ch.curve_b(p)                        # the multiples stay on p's curve
        assert ref.mul(a, ref.neg(p)) == ref.neg(ref.mul(a, p))


def test_signed_digit_horner_equals_the_plain_multiple():
    rng = random.Random(12)
    for c in (ref.plan(1)[0], ref.plan(300)[0], ref.plan(5000)[0]):
        for p in some_points(4, c):
            for s in (1, 2, 3, (1 << c) - 1, 1 << c, 1 << (c * (-(-255 // c) - 1)), rng.randrange(R)):
                acc = None
                for d in reversed(ref.digits(s, c)):
                    for _ in range(c):
                        acc = ref.add(acc, acc)
                    acc = ref.add(acc, ref.mul(d, p) if d >= 0 else ref.neg(ref.mul(-d, p)))
                assert acc == ref.mul(s, p), (c, hex(s))


def test_orders_two_and_three():
    for s in STORED:
        v = ch.value_of(s)
        p2, p3 = (v, 0), (0, v)
        assert ref.add(p2, p2) is None and ref.mul(2, p2) is None and ref.mul(3, p2) == p2 and ref.neg(p2) == p2
        assert ref.add(p3, p3) == ref.neg(p3) and ref.mul(2, p3) == (0, Q - v) and ref.mul(3, p3) is None and ref.mul(4, p3) == p3
    rng = random.Random(13)
    for _ in range(4):
        k = rng.randrange(R)
        assert ref.mul(k, (ch.value_of(STORED[3]), 0)) == ((ch.value_of(STORED[3]), 0) if k & 1 else None)
        assert ref.mul(k, (0, ch.value_of(STORED[8]))) == [None, (0, ch.value_of(STORED[8])), (0, Q - ch.value_of(STORED[8]))][k % 3]


def test_an_independent_point_shares_the_curve_and_the_sum_does_not_depend_on_the_order():
    rng = random.Random(14)
    for p in [(ch.value_of(BY_NAME["ones7"]), 0), (0, ch.value_of(BY_NAME["q-1"]))] + some_points(3, 2):
        t = ch.independent_point(p)
        assert ch.curve_b(t) == ch.curve_b(p) and t[0] != p[0]
        a, b = rng.randrange(R), rng.randrange(R)
        ap, bt = ref.mul(a, p), ref.mul(b, t)
        assert ref.add(ap, bt) == ref.add(bt, ap) == ref.msm([a, b], [p, t])
        assert ref.add(ref.add(ap, bt), t) == ref.add(ap, ref.add(bt, t))       # associative: p and t lie in one group


def test_chord_addition_of_arbitrary_pairs_is_commutative():
    for a, b in ch.chord_pairs():
        p, q = ch.point_of_stored(*a), ch.point_of_stored(*b)
        s = ref.add(p, q)
        assert s == ref.add(q, p) and s is not None
        assert s == ref.to_affine(ref.jac_add(ref.to_jac(p), ref.to_jac(q)))     # the checker's two formula sets agree
