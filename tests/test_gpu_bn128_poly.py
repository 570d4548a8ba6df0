"""BN254 Fr polynomial division by x^k - beta and evaluation on the device (pil2gl.bn128.poly_div / poly_eval over csrc/bn_poly.hip)
against the Python checker (tests/bn128_poly_ref.py: Python integers from the definition).  Every comparison is exact equality of the
Montgomery words; nothing here has a tolerance.  Shapes at the planner's thresholds are asked of the planner hook (poly_plan), never
typed in.  The checker runs on the integers the device words spell (the recurrence is linear in c), with beta as a plain integer."""
import random

import numpy as np
import pytest

import bn128_chosen
import bn128_poly_ref as ref
from bn128_poly_ref import R

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

MAX_SMALL_N = 1 << 22                                  # the planner's carry-level count stops growing here (tests/test_bn128_poly_cpu.py)


@pytest.fixture(scope="module")
def bn():
    import pil2gl
    from pil2gl import bn128
    pil2gl.init(0)
    return bn128


def dev(words):
    return torch.from_numpy(np.ascontiguousarray(words).view(np.int64)).cuda()


def host(t):
    return t.cpu().numpy().view(np.uint64)


def elem(v):
    """a plain integer as the host-side Montgomery words the entries take"""
    return ref.words([ref.mont(v)])


def check_div(bn, c, k, beta, on_device=True, in_place=True):
    """c: the integers the coefficient words spell"""
    want = ref.words(ref.scan(c, k, beta))
    w = ref.words(c)
    src = dev(w) if on_device else w.copy()
    got = bn.poly_div(src, k, elem(beta), out=src if in_place else None)
    g = host(got) if on_device else got
    bad = np.argwhere((g.reshape(-1, 4) != want).any(axis=1))
    assert bad.size == 0, "n = %d, k = %d: differs first at element %d" % (len(c), k, bad[0][0])
    if not in_place:
        assert np.array_equal(host(src) if on_device else src, w), "src was written"


def check_eval(bn, c, zs, on_device=True, stride=1):
    """-> the device's values; compared with Horner in the checker; the coefficient bytes must be unchanged afterwards"""
    w = ref.words(c)
    if stride > 1:
        m = ref.words(ref.rand_elems(len(c) * stride, 77)).reshape(len(c), stride, 4)
        m[:, 1] = w
        flat = m.reshape(-1)[4:]                                  # column 1 of a matrix `stride` wide
    else:
        flat = w.reshape(-1)
    src = dev(flat) if on_device else flat.copy()
    got = bn.poly_eval(src, ref.words([ref.mont(z) for z in zs]), n=len(c), stride=stride)
    g = host(got) if on_device else got
    assert g.shape == (len(zs), 4)
    assert ref.ints(g) == [ref.evaluate(c, z) for z in zs], (len(c), stride)
    assert np.array_equal(host(src) if on_device else src, flat), "src was written"
    return ref.ints(g)


def smallest_n(bn, k, pred, hi=MAX_SMALL_N):
    """the smallest n <= hi whose plan at k satisfies pred (pred is monotone in n)"""
    assert pred(bn.poly_plan(hi, k)), "no n up to %d" % hi
    lo = 0
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if pred(bn.poly_plan(mid, k)):
            hi = mid
        else:
            lo = mid
    return hi


BETAS = (0, 1, R - 1, 2, random.Random(14).randrange(R))


# ---- small shapes, all combinations ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (1, 2, 3, 7, 64, 65, 1000))
def test_small_shapes_every_k_and_beta(bn, n):
    c = ref.rand_elems(n, n)
    for k in sorted(k for k in {1, 2, 3, 5, 64, n - 1, n, n + 1} if k >= 1):
        for beta in BETAS:
            check_div(bn, c, k, beta)


def test_coefficients_with_limbs_of_zeros_and_ones(bn):
    pats = [w for _, w in bn128_chosen.PATTERNS]                  # 0, r - 1, powers of two, all-ones limbs, byte patterns: all below r
    c = (pats + ref.limb_pattern_elems(200, 5))[:230]
    assert all(0 <= v < R for v in c) and 0 in c and R - 1 in c
    for k in (1, 3, 64):
        for beta in BETAS + tuple(pats[-6:]):
            check_div(bn, c, k, beta)
    check_eval(bn, c, [0, 1, R - 1] + pats[-4:])


# ---- segment edges and carry levels, from the plan -------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", (1, 3))
def test_segment_edges(bn, k):
    """S = 1 and S = 2, and at a many-segment shape M = L S exactly, L S - 1 and L (S - 1) + 1 (a last segment of one link); each with
    chains of equal length and with the last chains one link shorter (n not a multiple of k: at k = 3 some last segments are empty)"""
    n2 = smallest_n(bn, k, lambda p: p["S"] >= 2)
    assert bn.poly_plan(n2 - 1, k)["S"] == 1 and bn.poly_plan(n2, k)["S"] == 2
    ms = {-(-(n2 - 1) // k), -(-n2 // k)}
    p = bn.poly_plan(1000 * k, k)
    L, S = p["L"], p["S"]
    assert S > 2 and p["form"] == 1
    for M in (L * S, L * S - 1, L * (S - 1) + 1):
        q = bn.poly_plan(M * k, k)
        assert (q["L"], q["S"]) == (L, S), "the edge shapes must keep the plan they are edges of"
        ms.add(M)
    for M in sorted(ms):
        for n in sorted({M * k, M * k - 1, (M - 1) * k + 1}):
            check_div(bn, ref.rand_elems(n, n), k, BETAS[4])
            check_eval(bn, ref.rand_elems(n, n + 1), [BETAS[4], 0])


@pytest.mark.parametrize("k", (1, 3))
def test_smallest_shape_of_every_carry_level_count(bn, k):
    top = bn.poly_plan(1 << 28, k)["levels"]
    assert top >= 3
    for levels in range(1, top + 1):
        n = smallest_n(bn, k, lambda p: p["levels"] >= levels)
        assert bn.poly_plan(n, k)["levels"] == levels and bn.poly_plan(n - 1, k)["levels"] == levels - 1
        c = ref.rand_elems(n, levels)
        check_div(bn, c, k, BETAS[4])
        if k == 1:
            zs = [BETAS[4], R - 1]
            assert check_eval(bn, c, zs)[0] == ref.scan(c, 1, zs[0])[0]


# ---- a lane per chain ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", (1 << 12, 1 << 14))
def test_lane_per_chain(bn, k):
    for M in (1, 2, 3, 8):
        for n in (M * k, M * k - 5):
            assert bn.poly_plan(n, k)["form"] == 0
            check_div(bn, ref.rand_elems(n, M), k, 1 if M == 2 else BETAS[4])


def test_where_the_plan_switches_form(bn):
    n = 4099
    ks = [k for k in range(2, n + 2) if bn.poly_plan(n, k)["form"] == 0 and bn.poly_plan(n, k - 1)["form"] == 1]
    assert len(ks) == 1, ks
    k = ks[0]
    c = ref.rand_elems(n, 8)
    check_div(bn, c, k, BETAS[4])
    check_div(bn, c, k - 1, BETAS[4])


# ---- addressing and aliasing -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("on_device", (True, False))
@pytest.mark.parametrize("stride", (1, 3))
def test_a_column_in_place_leaves_the_other_columns_alone(bn, stride, on_device):
    n, k, beta, col = 1500, 3, BETAS[4], stride - 1
    m = ref.words(ref.rand_elems(n * stride, 31)).reshape(n, stride, 4)
    c = ref.ints(m[:, col])
    want = m.copy()
    want[:, col] = ref.words(ref.scan(c, k, beta))
    for in_place in (True, False):
        src = m.reshape(-1)[4 * col:].copy()
        dst_init = ref.words(ref.rand_elems(n * stride, 32)).reshape(-1)[4 * col:].copy()
        s = dev(src) if on_device else src
        d = s if in_place else (dev(dst_init) if on_device else dst_init.copy())
        got = bn.poly_div(s, k, elem(beta), n=n, stride=stride, out=d)
        g = host(got) if on_device else got
        exp = want.reshape(-1)[4 * col:].copy()
        if not in_place:                                          # a disjoint destination keeps its own words between the elements
            e = dst_init.copy()
            idx = (np.arange(n)[:, None] * 4 * stride + np.arange(4)[None, :]).reshape(-1)
            e[idx] = exp[idx]
            exp = e
            assert np.array_equal(host(s) if on_device else s, src), "src was written"
        assert np.array_equal(g, exp), (stride, on_device, in_place)


@pytest.mark.parametrize("on_device", (True, False))
def test_disjoint_and_in_place_through_both_forms(bn, on_device):
    c = ref.rand_elems(2100, 41)
    for k in (1, 7):
        for in_place in (True, False):
            check_div(bn, c, k, BETAS[4], on_device, in_place)
    check_eval(bn, c, [3, BETAS[4]], on_device)


# ---- divZh end to end ------------------------------------------------------------------------------------------------------------------
def test_divzh_then_first_nonzero_row(bn):
    N, n = 1 << 10, 4 << 10
    q = ref.rand_elems(n - N, 51)
    c = ref.mul_back(q, [0] * N, N, 1)                            # q (x^N - 1)
    d = dev(ref.words(c))
    bn.poly_div(d, N, elem(1), out=d)
    sec = d.reshape(n, 1, 4)
    assert bn.first_nonzero_row(sec, 0, 0, N) is None
    assert ref.ints(host(d)[N:]) == q
    # one word of one coefficient flipped: the remainder position of its chain shows exactly that difference
    spoilt = list(c)
    i = 2 * N + 37
    spoilt[i] ^= 1 << 64
    assert spoilt[i] < R
    d = dev(ref.words(spoilt))
    bn.poly_div(d, N, elem(1), out=d)
    row, val = bn.first_nonzero_row(d.reshape(n, 1, 4), 0, 0, N)
    assert row == 37 and ref.ints(val) == [(spoilt[i] - c[i]) % R]
    assert ref.ints(host(d)) == ref.scan(spoilt, N, 1)


# ---- evaluation --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_points", (1, 2, 64))
def test_eval_points(bn, n_points):
    zs = ([0, 1, R - 1] + ref.rand_elems(64, 61))[:n_points] if n_points > 2 else [R - 1, BETAS[4]][:n_points]
    for n in (1, 33, 1025, 5000):
        c = ref.rand_elems(n, n)
        check_eval(bn, c, zs)
    check_eval(bn, ref.rand_elems(1100, 3), zs, stride=3)


def test_eval_is_the_first_element_of_the_division_by_x_minus_z(bn):
    c = ref.rand_elems(3000, 71)
    for z in (0, 1, R - 1, BETAS[4]):
        d = bn.poly_div(dev(ref.words(c)), 1, elem(z))
        v = check_eval(bn, c, [z])[0]
        assert ref.ints(host(d)[:1]) == [v] == [ref.evaluate(c, z)]


def test_empty_polynomial(bn):
    out = bn.poly_eval(dev(np.zeros((1, 4), np.uint64)), elem(5), n=0)
    assert not host(out).any()
    d = dev(ref.words([7]))
    bn.poly_div(d, 1, elem(5), n=0, out=d)
    assert ref.ints(host(d)) == [7]


def test_ifft_then_eval_at_a_domain_point_returns_the_evaluation(bn):
    n_bits = 8
    n = 1 << n_bits
    w = pow(5, (R - 1) >> n_bits, R)                              # ffjavascript's Fr.w[n_bits]
    c = ref.rand_elems(n, 81)                                     # plain integers here: the known polynomial
    ev = [ref.evaluate(c, pow(w, j, R)) for j in range(n)]        # the checker's evaluations on the domain
    coefs = bn.ifft(dev(ref.words([ref.mont(v) for v in ev])), 1, n_bits)
    js = (0, 1, 5, n // 2, n - 1)
    got = bn.poly_eval(coefs, ref.words([ref.mont(pow(w, j, R)) for j in js]), n=n)
    assert ref.ints(host(got)) == [ref.mont(ev[j]) for j in js]
