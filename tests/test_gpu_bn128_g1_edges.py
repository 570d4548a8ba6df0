"""BN254 G1 multi-scalar multiplication on the device with chosen Fq coordinates and with every exceptional case of bn_g1.cuh met by value
(pil2gl.bn128.g1_msm over csrc/bn_msm.hip, bn_g1.cuh, bn_fq.cuh) against the Python checker.  Every comparison is exact equality of the
64 output bytes.

Sections a to c feed stored (Montgomery) bytes of their own choosing: the kernels' formulas never use the curve constant, so an arbitrary
pair is a point of y^2 = x^3 + b' and the checker's b-free add / mul give the expected point, scalars acting as integers
(tests/bn128_g1_chosen.py, pinned by tests/test_bn128_g1_edges_cpu.py).  Section d uses bases of the real curve with known logs and
makes two computed representations (ZZ != 1) of one point, or of a point and its negative, meet in the reduce, tail and accumulate
kernels.  Window width, window count and buckets per window are asked of the library's planner."""
import ctypes as C
import random

import numpy as np
import pytest

import bn128_g1_chosen as ch
import bn128_g1_ref as ref
from bn128_g1_chosen import BY_NAME, NAMES, STORED, Y_SUBSET
from bn128_g1_ref import G, R

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

L1, LN = 8, 16                                       # items a lane of the reduction takes: first level, later levels (bn_params.h)


@pytest.fixture(scope="module")
def bn():
    import pil2gl
    from pil2gl import bn128
    pil2gl.init(0)
    return bn128


@pytest.fixture(scope="module")
def lib():
    import pil2gl
    return pil2gl.load()


def dev(words):
    return torch.from_numpy(np.ascontiguousarray(words).view(np.int64)).cuda()


def host(t):
    return t.cpu().numpy().view(np.uint64)


def plan(lib, n):
    out = (C.c_uint32 * 4)()
    nbytes = C.c_uint64()
    assert lib.pil2gl_debug_bn128_msm_plan(n, out, C.byref(nbytes)) == 0
    return tuple(out)


def levels(nbw):
    """reduction launches for nbw buckets per window"""
    m, count = -(-nbw // L1), 1
    while m > 1:
        m, count = -(-m // LN), count + 1
    return count


def hexes(words):
    b = np.ascontiguousarray(words, dtype="<u8").reshape(8).tobytes()
    return "(%064x, %064x)" % (int.from_bytes(b[:32], "little"), int.from_bytes(b[32:], "little"))


def same(got, want_point, what=""):
    want = ref.point_words([want_point]).reshape(8)
    assert np.array_equal(np.asarray(got).reshape(8), want), "%s: got stored %s, expected stored %s" % (what, hexes(got), hexes(want))


def run_stored(bn, pairs, scalars, montgomery=True, on_host=False):
    """pairs of stored integers, as they are, and integer scalars through the device entry (or the host-pointer one)"""
    bases, sc = ch.stored_point_words(pairs), ref.scalar_words(scalars, montgomery)
    if on_host:
        return bn.g1_msm(bases, sc, n=len(pairs), montgomery=montgomery)
    return host(bn.g1_msm(dev(bases), dev(sc), n=len(pairs), montgomery=montgomery))


def describe(pairs, scalars):
    return "stored bases %s, scalars %s" % (["(%x, %x)" % p for p in pairs], [hex(s) for s in scalars])


# ---- a. one chosen point, small integer scalars -------------------------------------------------------------------------------------
@pytest.mark.parametrize("xname", NAMES)
def test_a_small_scalars_on_one_chosen_point(bn, lib, xname):
    """1: copy and to-affine at ZZ = 1 (the bytes come back); 2: the reduction's acc += run is P + P, so g1_dbl works on the chosen
    bytes; 3: a doubling, then an addition; 2^c - 1: digits (-1, +1), fq_neg of the chosen y, c doublings and an addition of -P"""
    c = plan(lib, 1)[0]
    sx = BY_NAME[xname]
    for sy in Y_SUBSET:
        p = ch.point_of_stored(sx, sy)
        for s in (1, 2, 3, (1 << c) - 1):
            got = run_stored(bn, [(sx, sy)], [s])
            same(got, ref.mul(s, p), describe([(sx, sy)], [s]))
            if s == 1:
                assert np.array_equal(got, ch.stored_point_words([(sx, sy)]).reshape(8))


FEW = [(BY_NAME[x], BY_NAME[y]) for x, y in (("q-1", "q-2"), ("ones7", "2^224"), ("2^224-1", "ones7"), ("X", "X+1"), ("2^32-1", "(q-1)/2"),
                                            ("2^512 mod q", "q-ones7"), ("1", "2^256 mod q"), ("(q+1)/2", "2"))]


def test_a_window_scalars_a_random_scalar_and_both_scalar_forms_on_a_few_points(bn, lib):
    c, n_w, nbw, _ = plan(lib, 1)
    rng = random.Random(0xA)
    top = 1 << (c * (n_w - 1))
    assert top < R
    for pair in FEW:
        p = ch.point_of_stored(*pair)
        for s in (1 << c, 1 << (c * (n_w // 2)), top, nbw << c, rng.randrange(R)):
            want = ref.mul(s, p)
            for montgomery in (True, False):
                same(run_stored(bn, [pair], [s], montgomery), want, describe([pair], [s]))
        for s in (1, 2, 3, (1 << c) - 1):
            same(run_stored(bn, [pair], [s], montgomery=False), ref.mul(s, p), describe([pair], [s]))
    pair, s = FEW[1], rng.randrange(R)                               # and once from host pointers
    got = run_stored(bn, [pair], [s], on_host=True)
    assert isinstance(got, np.ndarray)
    same(got, ref.mul(s, ch.point_of_stored(*pair)), describe([pair], [s]))


# ---- b. two arbitrary points, scalars (1, 1): one chord addition on the chosen bytes ---------------------------------------------------
CHORDS = ch.chord_pairs()


@pytest.mark.parametrize("xname", NAMES)
def test_b_chord_addition_of_two_chosen_points(bn, xname):
    """x2 - x1 and y2 - y1 are taken on the stored values themselves (both operands at ZZ = 1), to-affine inverts a power of x2 - x1"""
    mine = [(a, b) for a, b in CHORDS if a[0] == BY_NAME[xname]]
    assert len(mine) == len(STORED) - 1
    for a, b in mine:
        want = ref.add(ch.point_of_stored(*a), ch.point_of_stored(*b))
        same(run_stored(bn, [a, b], [1, 1]), want, describe([a, b], [1, 1]))


# ---- c. points of order 2 and 3 -------------------------------------------------------------------------------------------------------
ORDER_STORED = [BY_NAME[k] for k in ("1", "q-1", "2^256 mod q", "ones7", "2^224", "X")]


def with_a_second_point(bn, lib, pairs, scalars, small):
    """the same sum once more with a point of the same curve in another window: P itself, and a point that is no multiple of P.  The
    exceptional case sits in the lower window, and, where the scalars leave room (small), in the higher one, so that the tail goes on
    from an accumulator at infinity"""
    n = len(pairs) + 1
    c, n_w = plan(lib, n)[:2]
    p = ch.point_of_stored(*pairs[0])
    points = [ch.point_of_stored(*q) for q in pairs]
    for t in (p, ch.independent_point(p)):
        for w in (1, n_w // 2):
            placed = [(list(scalars) + [1 << (c * w)])]
            if small:
                placed.append([s << (c * w) for s in scalars] + [1])
            for sc in placed:
                assert all(s < R for s in sc)
                want = ref.msm(sc, points + [t])
                same(run_stored(bn, pairs + [ch.stored_of(t)], sc), want, describe(pairs + [ch.stored_of(t)], sc))


def test_c_a_point_of_order_two(bn, lib):
    """(x, 0): doubling leaves through g1_dbl's (2y)^2 == 0 exit, wherever it happens (reduction for 2, tail for 2^c - 1)"""
    c = plan(lib, 1)[0]
    assert plan(lib, 2)[0] == c
    rng = random.Random(0xC2)
    for sx in ORDER_STORED:
        p = (ch.value_of(sx), 0)
        for s in (1, 2, 3, (1 << c) - 1, rng.randrange(R) | 1, rng.randrange(R) & ~1):
            want = p if s & 1 else None
            assert want == ref.mul(s, p)
            same(run_stored(bn, [(sx, 0)], [s]), want, describe([(sx, 0)], [s]))
            with_a_second_point(bn, lib, [(sx, 0)], [s], small=s < (1 << c))


def test_c_a_point_of_order_three(bn, lib):
    """(0, y): 2P = -P, so P + 2P is a point and its negative, met by value in the reduction (3) and in the tail (2^c - 1, 2^c)"""
    c = plan(lib, 1)[0]
    rng = random.Random(0xC3)
    for sy in ORDER_STORED:
        p = (0, ch.value_of(sy))
        for s in (1, 2, 3, 4, 1 << c, (1 << c) - 1, rng.randrange(R)):
            want = [None, p, ref.neg(p)][s % 3]
            assert want == ref.mul(s, p)
            same(run_stored(bn, [(0, sy)], [s]), want, describe([(0, sy)], [s]))
            with_a_second_point(bn, lib, [(0, sy)], [s], small=s <= (1 << c))


@pytest.mark.parametrize("n", (2, 3, 64, 65))
def test_c_copies_of_a_point_of_order_two(bn, lib, n):
    """one bucket alternates between P and infinity"""
    for sx in ORDER_STORED[::2]:
        p = (ch.value_of(sx), 0)
        same(run_stored(bn, [(sx, 0)] * n, [1] * n), p if n & 1 else None, "%d copies of (%x, 0)" % (n, sx))
        with_a_second_point(bn, lib, [(sx, 0)] * n, [1] * n, small=True)


# ---- d. the same point in two representations ------------------------------------------------------------------------------------------
class Curve:
    """a few bases of the real curve with known logs; the lists are padded with them under zero scalars"""

    def __init__(self):
        self.points, self.logs = ref.known_log_bases(16, seed=2541)
        self.words = ref.point_words(self.points)

    def run(self, bn, n, actors, scalars):
        bases = np.resize(self.words, (n, 8))
        bases[:len(actors)] = ref.point_words(actors)
        sc = np.zeros((n, 4), np.uint64)
        sc[:len(actors)] = ref.scalar_words(scalars)
        return host(bn.g1_msm(dev(bases), dev(sc), n=n))


@pytest.fixture(scope="module")
def curve():
    return Curve()


def times_g(k):
    return ref.mul(k % R, G)


SIZES = ((3, 1), (300, 2), (5000, 3))                # n, the reduction levels the planner's bucket count gives it


@pytest.mark.parametrize("n,n_levels", SIZES)
def test_d_reduction_meets_a_computed_sum_and_the_same_point(bn, lib, curve, n, n_levels):
    """bucket k+1 holds {A, B} (a computed sum, ZZ != 1), bucket k the single point C = A + B, then C = -(A + B): the running sum meets
    its equal, or its negative, by value.  k and k+1 share a first-level lane (1, 7, nbw - 1), sit in neighbouring first-level lanes
    (8: the second level meets 8 (A + B) and 8 C, both computed) or in neighbouring second-level lanes (128)"""
    c, n_w, nbw, _ = plan(lib, n)
    assert levels(nbw) == n_levels
    ks = sorted({k for k in (1, L1 - 1, L1, L1 * LN, nbw - 1) if k + 1 <= nbw})
    assert len(ks) >= 2 and (n_levels < 2 or L1 in ks) and (n_levels < 3 or L1 * LN in ks)
    (A, B), (a, b) = curve.points[:2], curve.logs[:2]
    for sign in (1, -1):
        Cp = times_g(sign * (a + b))
        for k in ks:
            for w in (0, n_w // 2):
                scalars = [(k + 1) << (c * w), (k + 1) << (c * w), k << (c * w)]
                want = times_g(((k + 1) * (a + b) + sign * k * (a + b)) << (c * w))
                same(curve.run(bn, n, [A, B, Cp], scalars), want, "n %d sign %d k %d window %d" % (n, sign, k, w))


@pytest.mark.parametrize("n,n_levels", SIZES)
def test_d_tail_meets_the_doubled_window_and_the_same_point(bn, lib, curve, n, n_levels):
    """P in window 1 and 2^c P in window 0: after its c doublings (ZZ != 1) the Horner accumulator equals window 0's point; with
    -2^c P it is its negative.  One window higher with a third point in window 0, the tail goes on from the result"""
    c, n_w, nbw, _ = plan(lib, n)
    assert levels(nbw) == n_levels
    A, a, T, t = curve.points[2], curve.logs[2], curve.points[3], curve.logs[3]
    for sign in (1, -1):
        P2 = times_g(sign * (a << c))
        same(curve.run(bn, n, [A, P2], [1 << c, 1]), times_g((a << c) + sign * (a << c)), "n %d sign %d" % (n, sign))
        want = times_g((a << (2 * c)) + sign * (a << (2 * c)) + t)
        same(curve.run(bn, n, [A, P2, T], [1 << (2 * c), 1 << c, 1]), want, "n %d sign %d, one window higher" % (n, sign))


@pytest.mark.parametrize("n,n_levels", SIZES)
def test_d_bucket_accumulation_ends_on_a_point_and_its_negative(bn, lib, curve, n, n_levels):
    """one bucket holds {A, A, -2A}: in every arrival order the last addition is a computed point (ZZ != 1) and its negative.  With the
    digit -d the bucket holds the negated points, and the next window's bucket 1 the points themselves"""
    c, n_w, nbw, _ = plan(lib, n)
    assert levels(nbw) == n_levels
    m = max(n, 4)
    assert plan(lib, m)[:3] == (c, n_w, nbw)
    A, a, T, t = curve.points[4], curve.logs[4], curve.points[5], curve.logs[5]
    M = times_g(-2 * a)
    for w in (0, n_w // 2):
        for d in (1, nbw - 1, nbw):
            for digit in (d, (1 << c) - d) if d < nbw else (d,):         # 2^c - d is recoded as (-d, +1)
                s = digit << (c * w)
                same(curve.run(bn, n, [A, A, M], [s] * 3), None, "n %d window %d digit %d" % (n, w, digit))
                d2 = d - 1 if d > 1 else 2
                same(curve.run(bn, m, [A, A, M, T], [s] * 3 + [d2 << (c * w)]), times_g((d2 * t) << (c * w)), "n %d window %d digit %d and a further bucket" % (m, w, digit))
