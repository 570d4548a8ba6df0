"""The BN254 Fr sparse products, scaled sums and degree without a device: the Python checker checked against itself (both sides of
acc' = s acc + M src evaluated at points; a zerofier vanishing at its roots), and the ABI surface: the symbols, every refusal before
any device call through the host-pointer entry and the _dev entry (bogus and misaligned device pointers), the empty case."""
import ctypes as C
import random

import numpy as np
import pytest

import bn128_polymul_ref as ref
from bn128_polymul_ref import R
from pil2gl.bn128 import poly_fma, poly_degree  # noqa: F401  (the feature under test: without it nothing here runs)

OK, EINVAL, ENODEV = 0, -1, -2
MAX_N = 1 << 28
SYMBOLS = ("pil2gl_bn128_poly_fma", "pil2gl_bn128_poly_fma_dev", "pil2gl_bn128_poly_degree", "pil2gl_bn128_poly_degree_dev")


# ---- the checker -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_src,n_acc,exps,scaled", ((1, 2, (0, 1), True), (5, 30, (0, 1, 7, 4, 5, 10), True), (40, 48, (0, 8), False),
                                                    (17, 17, (0,), True), (0, 9, (3,), True), (12, 300, (0, 100, 288), False)))
def test_checker_both_sides_agree_at_points(n_src, n_acc, exps, scaled):
    """acc'(z) = s acc(z) + M(z) src(z): the product is never truncated (n_src + e_max <= n_acc), so the identity is exact"""
    rng = random.Random(n_acc * 100 + n_src)
    exps = sorted(exps)
    terms = [(rng.randrange(R), e) for e in exps]
    acc = [rng.randrange(R) for _ in range(n_acc)]
    src = [rng.randrange(R) for _ in range(n_src)]
    s = rng.randrange(R) if scaled else None
    new = ref.fma(acc, src, terms, s)
    assert len(new) == n_acc
    for z in (0, 1, R - 1, rng.randrange(R), rng.randrange(R)):
        want = ((s or 0) * ref.evaluate(acc, z) + ref.eval_terms(terms, z) * ref.evaluate(src, z)) % R
        assert ref.evaluate(new, z) == want


def test_checker_source_is_zero_outside_its_range():
    assert ref.fma([9, 9, 9, 9], [1, 2], [(1, 0), (1, 1)], None) == [1, 3, 2, 0]
    assert ref.fma([9, 9, 9, 9], [1, 2], [(1, 2)], 1) == [9, 9, 10, 11]
    assert ref.fma([5, 6], [], [(7, 0)], 2) == [10, 12] and ref.fma([5, 6], [], [(7, 0)], None) == [0, 0]


def test_checker_zerofier_vanishes_at_its_roots():
    rng = random.Random(7)
    roots = [rng.randrange(R) for _ in range(6)]
    terms = ref.zerofier_terms([(1, a) for a in roots])
    assert [e for _, e in terms] == list(range(7)) and terms[-1][0] == 1
    for a in roots:
        assert ref.eval_terms(terms, a) == 0
    assert ref.eval_terms(terms, roots[0] + 1) != 0
    # x^k - beta factors: zero at every k-th root of beta; equal to the dense product
    k, beta = 4, pow(rng.randrange(R), 4, R)
    terms = ref.zerofier_terms([(k, beta), (2, 9), (1, 3)])
    assert ref.dense(terms) == ref.poly_mul(ref.poly_mul([-beta % R, 0, 0, 0, 1], [-9 % R, 0, 1]), [-3 % R, 1])
    # coefficients that cancel are dropped: (x - 1)(x + 1) = x^2 - 1
    assert ref.zerofier_terms([(1, 1), (1, R - 1)]) == [(R - 1, 0), (1, 2)]


def test_checker_degree_and_interpolation():
    assert ref.degree([]) == ref.NONE and ref.degree([0, 0]) == ref.NONE and ref.degree([3]) == 0 and ref.degree([0, 5, 0]) == 1
    pts, vals = [2, 5, 11, R - 3], [7, 0, R - 1, 12345]
    c = ref.interpolate(pts, vals)
    assert [ref.evaluate(c, p) for p in pts] == vals


# ---- the ABI surface -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    import pil2gl
    return pil2gl.load()


def test_every_new_symbol_is_exported(lib):
    for name in SYMBOLS:
        assert hasattr(lib, name)
    from pil2gl import bn128
    assert callable(bn128.poly_fma) and callable(bn128.poly_degree)


def _p(a, byte_offset=0):
    return None if a is None else C.c_void_p(a.ctypes.data + byte_offset)


def _fma(lib, dev, acc, n_acc, acc_stride, scale, src, n_src, src_stride, coefs, exps, t):
    args = [acc, n_acc, acc_stride, scale, src, n_src, src_stride, coefs, exps, t]
    return lib.pil2gl_bn128_poly_fma_dev(*(args + [None])) if dev else lib.pil2gl_bn128_poly_fma(*args)


def _terms(exps, coef=3):
    m = ref.words([ref.mont(coef)] * len(exps)).reshape(-1)
    return m, np.array(exps, np.uint64)


@pytest.mark.parametrize("dev", (False, True))
def test_every_fma_refusal_comes_before_any_device_call(lib, dev):
    """through the host-pointer entry AND the _dev entry, which checks its arguments as host integers first: the `device` pointers here
    are host arrays, which no kernel may ever see"""
    acc, src = np.ones(4 * 64, np.uint64), np.ones(4 * 64, np.uint64)
    sec = np.ones(4 * 5 * 40, np.uint64)                           # a section 5 wide
    one = ref.words([ref.mont(1)]).reshape(-1)
    call = lambda *a: _fma(lib, dev, *a)                           # noqa: E731
    msg = lib.pil2gl_last_error
    m2, e2 = _terms((0, 1))
    # t = 0 and t = 65
    m65, e65 = _terms(range(65))
    assert call(_p(acc), 40, 1, _p(one), _p(src), 8, 1, _p(m2), _p(e2), 0) == EINVAL and b"terms" in msg()
    assert call(_p(acc), 200, 1, _p(one), _p(src), 8, 1, _p(m65), _p(e65), 65) == EINVAL and b"terms" in msg()
    # equal, and decreasing, exponents
    for exps in ((0, 3, 3), (0, 5, 4)):
        m, e = _terms(exps)
        assert call(_p(acc), 40, 1, _p(one), _p(src), 8, 1, _p(m), _p(e), 3) == EINVAL and b"increasing" in msg()
    # an exponent above 2^28
    m, e = _terms((0, MAX_N + 1))
    assert call(_p(acc), 40, 1, _p(one), _p(src), 8, 1, _p(m), _p(e), 2) == EINVAL and b"2^28" in msg()
    # counts above 2^28
    assert call(_p(acc), MAX_N + 1, 1, _p(one), _p(src), 8, 1, _p(m2), _p(e2), 2) == EINVAL and b"2^28" in msg()
    assert call(_p(acc), 40, 1, _p(one), _p(src), MAX_N + 1, 1, _p(m2), _p(e2), 2) == EINVAL and b"2^28" in msg()
    # the product one coefficient longer than acc: nSrc + e_max = nAcc + 1
    m, e = _terms((0, 1, 7))
    assert call(_p(acc), 14, 1, _p(one), _p(src), 8, 1, _p(m), _p(e), 3) == EINVAL and b"truncated" in msg()
    # stride 0 and 2^32, either column
    for bad in (0, 1 << 32):
        assert call(_p(acc), 40, bad, _p(one), _p(src), 8, 1, _p(m2), _p(e2), 2) == EINVAL and b"stride" in msg()
        assert call(_p(acc), 40, 1, _p(one), _p(src), 8, bad, _p(m2), _p(e2), 2) == EINVAL and b"stride" in msg()
    # null pointers: acc, src (with a non-zero count), the coefficients, the exponents
    assert call(None, 40, 1, _p(one), _p(src), 8, 1, _p(m2), _p(e2), 2) == EINVAL and b"null" in msg()
    assert call(_p(acc), 40, 1, _p(one), None, 8, 1, _p(m2), _p(e2), 2) == EINVAL and b"null" in msg()
    assert call(_p(acc), 40, 1, _p(one), _p(src), 8, 1, None, _p(e2), 2) == EINVAL and b"null" in msg()
    assert call(_p(acc), 40, 1, _p(one), _p(src), 8, 1, _p(m2), None, 2) == EINVAL and b"null" in msg()
    # overlapping columns: the same column with two terms, and with one shifted term; shifted rows; another stride over the same bytes;
    # a pointer that is no element apart; a column of a section against the same column a row on
    m1, e1 = _terms((1,))
    overlaps = ((_p(acc), 40, 1, _p(acc), 8, 1, m2, e2), (_p(acc), 40, 1, _p(acc), 8, 1, m1, e1), (_p(acc), 40, 1, _p(acc, 32), 8, 1, m2, e2),
                (_p(acc), 20, 2, _p(acc), 8, 1, m2, e2), (_p(acc), 40, 1, _p(acc, 8), 8, 1, m2, e2),
                (_p(sec), 30, 5, _p(sec, 32 * 5), 8, 5, m2, e2), (_p(sec, 32), 30, 5, _p(sec, 64), 8, 3, m2, e2))
    for a, na, sa, s, ns, ss, m, e in overlaps:
        assert call(a, na, sa, _p(one), s, ns, ss, _p(m), _p(e), len(e)) == EINVAL and b"overlaps" in msg(), (na, sa, ns, ss)
    if dev:                                                        # device columns are 16-byte aligned: refused before the device is looked for
        assert call(_p(acc, 8), 40, 1, _p(one), _p(src), 8, 1, _p(m2), _p(e2), 2) == EINVAL and b"aligned" in msg()
        assert call(_p(acc), 40, 1, _p(one), _p(src, 8), 8, 1, _p(m2), _p(e2), 2) == EINVAL and b"aligned" in msg()
    # nAcc = 0 is OK and needs no device
    m0, e0 = _terms((0,))
    assert call(None, 0, 1, None, None, 0, 1, _p(m0), _p(e0), 1) == OK
    assert call(None, 0, 1, _p(one), None, 0, 1, _p(m2), _p(e2), 2) == OK


def test_the_same_column_is_accepted_only_elementwise(lib):
    """t = 1, e = 0 on the same column passes the checks (through the host-pointer entry: with a device it computes, without one it is
    ENODEV -- never EINVAL), and so do two columns of one section; the same column with t = 2 is refused"""
    vals = ref.rand_elems(16, 5)
    buf = ref.words(vals).reshape(-1)
    m0, e0 = _terms((0,), coef=3)
    rc = lib.pil2gl_bn128_poly_fma(_p(buf), 16, 1, None, _p(buf), 16, 1, _p(m0), _p(e0), 1)
    assert rc in (OK, ENODEV), lib.pil2gl_last_error()
    if rc == OK:
        assert ref.ints(buf) == ref.fma(vals, vals, [(3, 0)], None)
    sec_vals = ref.rand_elems(3 * 12, 6)
    sec = ref.words(sec_vals).reshape(-1)
    m2, e2 = _terms((0, 2), coef=5)
    rc = lib.pil2gl_bn128_poly_fma(_p(sec, 32), 12, 3, None, _p(sec, 64), 10, 3, _p(m2), _p(e2), 2)
    assert rc in (OK, ENODEV), lib.pil2gl_last_error()
    if rc == OK:
        assert ref.ints(sec) == ref.fma_column(sec_vals, 1, 3, 12, sec_vals, 2, 3, 10, [(5, 0), (5, 2)], None)
    assert lib.pil2gl_bn128_poly_fma(_p(buf), 16, 1, None, _p(buf), 8, 1, _p(m2), _p(e2), 2) == EINVAL
    assert b"overlaps" in lib.pil2gl_last_error()


@pytest.mark.parametrize("dev", (False, True))
def test_every_degree_refusal_comes_before_any_device_call(lib, dev):
    col = np.ones(4 * 64, np.uint64)
    d = C.c_uint64(5)
    call = (lambda *a: lib.pil2gl_bn128_poly_degree_dev(*(list(a) + [None]))) if dev else lib.pil2gl_bn128_poly_degree
    msg = lib.pil2gl_last_error
    assert call(_p(col), MAX_N + 1, 1, C.byref(d)) == EINVAL and b"2^28" in msg()
    for bad in (0, 1 << 32):
        assert call(_p(col), 8, bad, C.byref(d)) == EINVAL and b"stride" in msg()
    assert call(None, 8, 1, C.byref(d)) == EINVAL and b"null" in msg()
    assert call(_p(col), 8, 1, None) == EINVAL and b"null" in msg()
    if dev:
        assert call(_p(col, 8), 8, 1, C.byref(d)) == EINVAL and b"aligned" in msg()
    d = C.c_uint64(5)
    assert call(None, 0, 1, C.byref(d)) == OK and d.value == ref.NONE      # n = 0: no degree, no device


def test_the_python_wrappers_refuse_what_they_can_see():
    from pil2gl import Pil2glError
    acc, src = np.zeros((8, 4), np.uint64), np.zeros((4, 4), np.uint64)
    m = ref.words([1, 2])
    with pytest.raises(Pil2glError, match="needs"):
        poly_fma(acc, src, m, [0, 1], n_acc=9, n_src=4)
    with pytest.raises(Pil2glError, match="needs"):
        poly_fma(acc, src, m, [0, 1], n_acc=8, n_src=5)
    with pytest.raises(Pil2glError, match="exponents"):
        poly_fma(acc, src, m, [0, 1, 2], n_acc=8, n_src=4)
    with pytest.raises(Pil2glError, match="stride"):
        poly_fma(acc, src, m, [0, 1], n_acc=8, n_src=4, acc_stride=0)
    with pytest.raises(Pil2glError, match="truncated"):                # the library's refusal, raised
        poly_fma(acc, src, m, [0, 5], n_acc=8, n_src=4)
    assert poly_degree(np.zeros((0, 4), np.uint64)) is None
