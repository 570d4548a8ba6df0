"""BN254 Fr products with a sparse polynomial, scaled sums and the degree on the device (pil2gl.bn128.poly_fma / poly_degree over
csrc/bn_polymul.hip) against the Python checker (tests/bn128_polymul_ref.py: Python integers from the definition).  Every comparison is
exact equality of the WHOLE buffer's words, so a write outside the column or outside [0, nAcc) shows; nothing here has a tolerance.
The checker runs on the integers the device words spell (the form is linear in acc and src), with scale and coefficients as plain
integers.  Without a device the module is skipped as a whole by the gpu mark; without the feature it fails at the import of the checker's
users below."""
import random

import numpy as np
import pytest

import bn128_polymul_ref as ref
from bn128_polymul_ref import R, MONT, POISON

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

WG = 256                                               # threads per workgroup of both kernels (csrc/bn_polymul.hip THREADS)
LIMBS = sum(0xFFFFFFFF << (32 * j) for j in range(7))  # seven limbs of 2^32 - 1, the top limb 0: below r


@pytest.fixture(scope="module")
def bn():
    import pil2gl
    from pil2gl import bn128
    pil2gl.init(0)
    assert callable(bn128.poly_fma) and callable(bn128.poly_degree)
    return bn128


def dev(vals):
    return torch.from_numpy(ref.words(vals).reshape(-1).view(np.int64)).cuda()


def host(t):
    return t.cpu().numpy().view(np.uint64)


def elem(v):
    return ref.words([ref.mont(v)])


def pack(terms):
    return ref.words([ref.mont(m) for m, _ in terms]), np.array([e for _, e in terms], np.uint64)


def check_fma(bn, acc_buf, a_off, a_stride, n_acc, src_buf, s_off, s_stride, n_src, terms, s):
    """acc_buf / src_buf: the integers the buffers' elements spell (src_buf None: src lives in acc_buf); the columns start at element
    a_off / s_off.  The whole acc buffer is compared, and the whole src buffer must be unchanged.  -> the new acc buffer's integers"""
    one = src_buf is None
    want = ref.fma_column(acc_buf, a_off, a_stride, n_acc, acc_buf if one else src_buf, s_off, s_stride, n_src, terms, s)
    d_acc = dev(acc_buf)
    d_src = d_acc if one else dev(src_buf)
    m, e = pack(terms)
    got = bn.poly_fma(d_acc[4 * a_off:], d_src[4 * s_off:], m, e, None if s is None else elem(s),
                      n_acc=n_acc, n_src=n_src, acc_stride=a_stride, src_stride=s_stride)
    assert got.data_ptr() == d_acc[4 * a_off:].data_ptr()
    g = host(d_acc).reshape(-1, 4)
    bad = np.argwhere((g != ref.words(want)).any(axis=1))
    assert bad.size == 0, "nAcc = %d, nSrc = %d, t = %d: differs first at buffer element %d" % (n_acc, n_src, len(terms), bad[0][0])
    if not one:
        assert np.array_equal(host(d_src).reshape(-1, 4), ref.words(src_buf)), "src was written"
    return want


# ---- launch boundaries ----
@pytest.mark.parametrize("n_src", (1, 2, 63, 64, 65, WG - 1, WG, WG + 1))
def test_launch_boundaries(bn, n_src):
    """(x - v) src at the wave and workgroup edges: nAcc = nSrc + 1, then a longer acc whose tail takes only s acc"""
    rng = random.Random(n_src)
    src = ref.rand_elems(n_src, n_src)
    terms = [(rng.randrange(R), 0), (1, 1)]
    for n_acc in (n_src + 1, n_src + 70, n_src + WG + 3):
        acc = ref.rand_elems(n_acc + 2, 1000 + n_acc)              # two elements past nAcc: they must stay
        check_fma(bn, acc, 0, 1, n_acc, src, 0, 1, n_src, terms, rng.randrange(R))
        check_fma(bn, acc, 0, 1, n_acc, src, 0, 1, n_src, terms, None)


# ---- the guarded source range ----
def test_terms_outside_the_source_are_not_loaded(bn):
    """src is a view in the middle of a buffer whose other elements are poison (32 bytes of 0xFF, not canonical): the exponents put
    terms below 0 and above nSrc for some lanes of a wave and not for others; a read outside the range would change the result"""
    n_src, pad = 100, 8
    exps = (0, 1, 7, n_src - 1, n_src, n_src + 5)
    rng = random.Random(3)
    terms = [(rng.randrange(R), e) for e in exps]
    src = [POISON] * pad + ref.rand_elems(n_src, 31) + [POISON] * (2 * n_src + 16)      # poison as far above as any exponent reaches
    n_acc = n_src + exps[-1] + 9
    acc = ref.rand_elems(n_acc, 32)
    new = check_fma(bn, acc, 0, 1, n_acc, src, pad, 1, n_src, terms, rng.randrange(R))
    assert POISON not in new
    new = check_fma(bn, [POISON] * n_acc, 0, 1, n_acc, src, pad, 1, n_src, terms, None)
    assert POISON not in new


# ---- a large exponent: byXNSubValue ----
@pytest.mark.parametrize("exp", (1 << 10, (1 << 10) + 500))
def test_large_exponent(bn, exp):
    """e = (0, 2^10) with nSrc = 2^10 + 3: the two copies overlap in three elements; with e[1] > nSrc they do not meet"""
    n_src = (1 << 10) + 3
    src = ref.rand_elems(n_src, exp)
    terms = [(R - 12345, 0), (1, exp)]
    n_acc = n_src + exp
    check_fma(bn, [POISON] * n_acc, 0, 1, n_acc, src, 0, 1, n_src, terms, None)
    check_fma(bn, ref.rand_elems(n_acc, 9), 0, 1, n_acc, src, 0, 1, n_src, terms, 1)


# ---- s = NULL and the scale values ----
def test_without_a_scale_acc_is_never_read(bn):
    src = ref.rand_elems(300, 41)
    terms = [(5, 0), (R - 1, 3), (1, 9)]
    a = check_fma(bn, [POISON] * 320, 0, 1, 320, src, 0, 1, 300, terms, None)
    b = check_fma(bn, ref.rand_elems(320, 42), 0, 1, 320, src, 0, 1, 300, terms, None)
    assert a == b and a[309:] == [0] * 11                          # nothing of acc in the result; the tail is zero-filled
    c = check_fma(bn, [POISON] * 40, 0, 1, 40, [], 0, 1, 0, [(7, 0)], None)            # nSrc = 0: zero-fill
    assert c == [0] * 40


@pytest.mark.parametrize("s", (1, 0, R - 1, 0x1234567890ABCDEF << 130 | 99))
def test_scale_values(bn, s):
    src = ref.rand_elems(200, 51)
    acc = ref.rand_elems(260, 52)
    acc[0], acc[1], acc[2] = 0, R - 1, MONT
    check_fma(bn, acc, 0, 1, 260, src, 0, 1, 200, [(3, 0), (R - 2, 60)], s)
    check_fma(bn, acc, 0, 1, 260, [], 0, 1, 0, [(3, 0)], s)        # nSrc = 0: only scales


# ---- strides ----
def test_columns_of_different_sections(bn):
    """src is column 1 of a section 3 wide, acc column 4 of a section 5 wide; every other column stays byte-identical"""
    n_src, n_acc = 130, 141
    src = ref.rand_elems(3 * n_src, 61)
    acc = ref.rand_elems(5 * n_acc, 62)
    terms = [(R - 7, 0), (9, 4), (1, 11)]
    new = check_fma(bn, acc, 4, 5, n_acc, src, 1, 3, n_src, terms, 77)
    for c in range(4):
        assert new[c::5] == acc[c::5]
    assert new[4::5] != acc[4::5]


def test_two_columns_of_one_section(bn):
    n_src, n_acc, width = 270, 280, 4
    sec = ref.rand_elems(width * n_acc, 63)
    terms = [(11, 0), (R - 1, 1), (1, 10)]
    new = check_fma(bn, sec, 2, width, n_acc, None, 0, width, n_src, terms, 5)          # column 0 into column 2
    for c in (0, 1, 3):
        assert new[c::width] == sec[c::width]
    check_fma(bn, sec, 1, width, n_acc, None, 3, width, n_src, terms, None)             # column 3 into column 1: src above acc


# ---- carry edges ----
def test_carry_edges(bn):
    """source words and coefficient words from {0, 1, r - 1, Montgomery 1, limbs of 2^32 - 1}; sums of two terms that are exactly r (-> 0)
    and exactly r - 1; coefficient 1 and r - 1 (the addition and the subtraction without a product) and a general one (the product)"""
    a = ref.rand_elems(1, 71)[0]
    # consecutive source words sum to r, r - 1, r, ...: with m = (1, 1) at e = (0, 1) the final addition meets both edges
    chain = [a]
    for i in range(1, 40):
        chain.append((R if i % 2 else R - 1) - chain[-1])
    new = check_fma(bn, [POISON] * 41, 0, 1, 41, chain, 0, 1, 40, [(1, 0), (1, 1)], None)
    assert new[1:40] == [0 if i % 2 else R - 1 for i in range(1, 40)]
    # the subtraction: x - x = 0, 0 - 1 = r - 1, and s = 1 with acc = r - 1 plus a source word 1: r -> 0
    new = check_fma(bn, [R - 1, 0, 5, LIMBS], 0, 1, 4, [1, 1, 5, 0], 0, 1, 4, [(1, 0)], 1)
    assert new == [0, 1, 10, LIMBS]
    new = check_fma(bn, [1, 0, 5, LIMBS], 0, 1, 4, [1, 1, 5, LIMBS], 0, 1, 4, [(R - 1, 0)], 1)
    assert new == [0, R - 1, 0, 0]
    # every pair of the edge words as (coefficient word, source word), through the product, with both shortcuts in the same list
    edge = [0, 1, R - 1, MONT, LIMBS]
    src = [v for v in edge for _ in edge] + ref.rand_elems(7, 72)
    for w in edge[1:]:                                             # the coefficient whose WORDS spell w is w / 2^256
        m = w * ref.MONT_INV % R
        assert ref.mont(m) == w
        terms = [(m, 0), (1, 3), (R - 1, 5), (LIMBS, 6)]
        check_fma(bn, ref.rand_elems(40, 73), 0, 1, 40, src, 0, 1, len(src), terms, LIMBS)


# ---- the term count ----
def test_sixty_four_terms_and_dropped_zero_coefficients(bn):
    n_src = 200
    src = ref.rand_elems(n_src, 81)
    rng = random.Random(82)
    dense = [(rng.randrange(1, R), j) for j in range(64)]
    check_fma(bn, ref.rand_elems(n_src + 70, 83), 0, 1, n_src + 70, src, 0, 1, n_src, dense, rng.randrange(R))
    # 64 terms, 40 of them zero: the same bytes as the compacted list of 24
    zeros = set(rng.sample(range(63), 40))                         # the last exponent stays: it sizes the product either way
    sparse = [(0 if j in zeros else m, 3 * j) for j, (m, _) in enumerate(dense)]
    compact = [t for t in sparse if t[0]]
    assert len(sparse) == 64 and len(compact) == 24
    n_acc = n_src + 3 * 63
    a = check_fma(bn, [POISON] * n_acc, 0, 1, n_acc, src, 0, 1, n_src, sparse, None)
    b = check_fma(bn, [POISON] * n_acc, 0, 1, n_acc, src, 0, 1, n_src, compact, None)
    assert a == b


# ---- in place ----
def test_in_place_elementwise(bn):
    vals = ref.rand_elems(WG + 44, 91) + [0, R - 1, MONT]
    n = len(vals)
    v = ref.rand_elems(1, 92)[0]
    new = check_fma(bn, vals, 0, 1, n, None, 0, 1, n, [(v, 0)], None)                  # mulScalar
    assert new == [v * x % R for x in vals]
    s, m = ref.rand_elems(2, 93)
    new = check_fma(bn, vals, 0, 1, n, None, 0, 1, n, [(m, 0)], s)                     # acc = (s + m) acc
    assert new == [(s + m) * x % R for x in vals]
    new = check_fma(bn, vals, 0, 1, n, None, 0, 1, n - 9, [(m, 0)], 1)                 # a shorter source: the tail keeps acc
    assert new[n - 9:] == vals[n - 9:]
    sec = ref.rand_elems(3 * 50, 94)
    check_fma(bn, sec, 1, 3, 50, None, 1, 3, 50, [(v, 0)], None)                       # a column of a section, in place


def test_a_shifted_product_in_place_is_refused(bn):
    from pil2gl import Pil2glError
    d = dev(ref.rand_elems(40, 95))
    before = host(d).copy()
    m, e = pack([(3, 0), (1, 1)])
    with pytest.raises(Pil2glError, match="overlaps"):
        bn.poly_fma(d, d, m, e, None, n_acc=40, n_src=39)
    assert np.array_equal(host(d), before)


# ---- degree ----
def degree_of(bn, vals, n=None, stride=1, off=0):
    got = bn.poly_degree(dev(vals)[4 * off:], n, stride)
    return ref.NONE if got is None else got


@pytest.mark.parametrize("n", (1, 63, 64, 65, WG - 1, WG, WG + 1, 3 * WG + 7))
def test_degree_positions(bn, n):
    assert degree_of(bn, [0] * n) == ref.NONE                      # all zero
    assert degree_of(bn, [7] + [0] * (n - 1)) == 0                 # only element 0
    assert degree_of(bn, [0] * (n - 1) + [1]) == n - 1             # only element n - 1
    rng = random.Random(n)
    for last in sorted({0, n - 1, n // 2} | {p for p in (62, 63, 64, 65, WG - 1, WG, WG + 1, n - 63, n - 64, n - 65, n - 66, n - WG, n - WG - 1) if 0 <= p < n}):
        vals = [rng.randrange(R) if rng.randrange(3) else 0 for _ in range(last)] + [rng.randrange(1, R)] + [0] * (n - last - 1)
        assert degree_of(bn, vals) == last == ref.degree(vals)


def test_degree_looks_at_every_limb(bn):
    """an element whose only non-zero 32-bit word is its last one, and one with only the first"""
    n = 200
    for word, where in ((1 << 224, 150), (1, 151), (1 << 96, 64), (1 << 160, 199)):
        vals = [0] * n
        vals[3] = 5
        vals[where] = word
        assert degree_of(bn, vals) == where
    assert bn.poly_degree(ref.words([0, 0, 1 << 224, 0]).reshape(-1)) == 2            # the host-pointer form
    assert bn.poly_degree(np.zeros((5, 4), np.uint64)) is None


def test_degree_of_a_column(bn):
    """stride 3: the other columns are non-zero above the true degree, and so is the buffer past n"""
    n, width = 300, 3
    sec = ref.rand_elems(width * (n + 4), 101)
    for last in (0, 64, 255, 256, 299):
        s = list(sec)
        for i in range(last + 1, n):
            s[1 + i * width] = 0
        assert s[1 + last * width] != 0
        assert degree_of(bn, s, n, width, off=1) == last
    s = list(sec)
    for i in range(n):
        s[1 + i * width] = 0
    assert degree_of(bn, s, n, width, off=1) == ref.NONE


# ---- composition: the open path at the smallest size where all three opening-set shapes occur ----
def test_open_builds_w_and_every_factor_divides_it(bn):
    """W = sum_i alpha^i (f_i - r_i) Z_{T \\ S_i} with |S_i| = 1, 2, 4 the k-th roots of random values: r_i from the existing poly_eval and
    Lagrange interpolation here, W from poly_fma and the zerofier's terms, then the existing poly_div by every factor of Z_T: every
    remainder position is zero and the quotient is the checker's"""
    N = 1 << 10
    rng = random.Random(2024)
    lens, ks = (N, 2 * N + 5, 4 * N), (1, 2, 4)
    f = [ref.rand_elems(n, 110 + i) for i, n in enumerate(lens)]   # the integers the coefficient words spell
    w4 = pow(5, (R - 1) // 4, R)
    assert pow(w4, 2, R) == R - 1
    h = [rng.randrange(1, R) for _ in ks]
    S = [[h[i] * pow(w4, (4 // k) * j, R) % R for j in range(k)] for i, k in enumerate(ks)]
    factors = [(k, pow(h[i], k, R)) for i, k in enumerate(ks)]     # Z_{S_i} = x^k - h^k
    for i, (k, beta) in enumerate(factors):
        assert all(pow(z, k, R) == beta for z in S[i]) and len(set(S[i])) == k
    alpha = rng.randrange(1, R)
    n_w = max(n + sum(k for j, k in enumerate(ks) if j != i) for i, n in enumerate(lens))
    d_f = [dev(c) for c in f]
    d_w = dev([POISON] * n_w)
    want_w = [0] * n_w
    one = [(1, 0)]
    for i in range(3):
        # r_i: the values of f_i on S_i from the device, interpolated on the host
        vals = ref.ints(host(bn.poly_eval(d_f[i], ref.words([ref.mont(z) for z in S[i]]))))
        assert vals == [ref.evaluate(f[i], z) for z in S[i]]
        r_i = ref.interpolate(S[i], vals)
        z_terms = ref.zerofier_terms([fac for j, fac in enumerate(factors) if j != i])
        a_i = pow(alpha, i, R)
        scaled = [(a_i * m % R, e) for m, e in z_terms]
        bn.poly_fma(d_w, d_f[i], *pack(scaled), None if i == 0 else elem(1), n_acc=n_w, n_src=lens[i])
        # - alpha^i Z r_i: a few coefficients, formed on the host and added from a short source
        low = [(-v) % R for v in ref.poly_mul(ref.dense(scaled), r_i)]
        bn.poly_fma(d_w, dev(low), *pack(one), elem(1), n_acc=n_w, n_src=len(low))
        want_w = ref.fma(want_w, f[i], scaled, 1)
        want_w = ref.fma(want_w, low, one, 1)
    assert ref.ints(host(d_w)) == want_w
    assert bn.poly_degree(d_w) == ref.degree(want_w) == n_w - 1
    # divide by every factor of Z_T; the quotient of a division starts k elements up
    import bn128_poly_ref as pref
    off, cur = 0, want_w
    for k, beta in factors:
        view = d_w[4 * off:]
        bn.poly_div(view, k, elem(beta), n=n_w - off, out=view)
        assert bn.first_nonzero_row(view.reshape(-1, 1, 4), 0, 0, k) is None, "a remainder of the division by x^%d - beta" % k
        q, rem = pref.divmod_xk(cur, k, beta)
        assert not any(rem)
        off, cur = off + k, q
    assert ref.ints(host(d_w[4 * off:])) == cur and len(cur) == n_w - sum(ks)
