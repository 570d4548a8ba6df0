"""BN254 Fr batch inverse, grand product and grand sum on the device (pil2gl.bn128.batch_inverse / gprod / gsum over csrc/bn_scan.hip)
against the Python checker (tests/bn128_hints_ref.py: Python integers from the definitions).  Every comparison is exact equality of the
Montgomery words.  Shapes at the planner's thresholds are asked of the planner hook (scan_plan), never typed in; apart from one case of
2^20 rows and the smallest shape of the highest level count, everything is at most 2^14 rows."""
import numpy as np
import pytest

import bn128_chosen
import bn128_fft_ref as fref
import bn128_hints_ref as ref
from bn128_hints_ref import R

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SENTINEL = np.uint64(0xA5A5A5A5A5A5A5A5)


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


def strided(words, stride, fill_seed=None):
    """(n, 4) words as a column of stride `stride`: flat words, element i at 4 * i * stride, up to the last element; between the
    elements the sentinel, or random canonical elements"""
    n = words.shape[0]
    if fill_seed is None or stride == 1:
        m = np.full((n, stride, 4), SENTINEL, np.uint64)
    else:
        m = ref.words(ref.rand_elems(n * stride, fill_seed)).reshape(n, stride, 4)
    m[:, 0] = words
    return m.reshape(-1)[:((n - 1) * stride + 1) * 4].copy()


def column_of(flat, n, stride):
    idx = (np.arange(n)[:, None] * 4 * stride + np.arange(4)[None, :]).reshape(-1)
    return flat[idx].reshape(n, 4), idx


def differs(got, want, what):
    bad = np.argwhere((got != want).any(axis=1))
    assert bad.size == 0, "%s: %d rows, differs first at row %d" % (what, got.shape[0], bad[0][0])


def check_all(bn, num, den, strides=(1, 1, 1), ops=("batch_inverse", "gprod", "gsum"), on_device=True, want=None):
    """num, den: plain integers.  strides: of num, den and out.  Every output is compared in whole, the words between a strided
    output's elements against the sentinel they were filled with; the inputs must be left as they were."""
    n, (sn, sd, so) = len(den), strides
    wn, wd = strided(ref.mont_words(num), sn, 5), strided(ref.mont_words(den), sd, 6)
    to = dev if on_device else (lambda a: a.copy())
    back = host if on_device else (lambda a: a)
    dn, dd = to(wn), to(wd)
    c = num[0]
    want = want or {}
    for op in ops:
        out0 = np.full(((n - 1) * so + 1) * 4, SENTINEL, np.uint64)
        out = to(out0)
        if op == "batch_inverse":
            bn.batch_inverse(dd, n=n, stride=sd, out=out, out_stride=so)
            exp = want.get(op) or ref.batch_inverse(den)
        elif op == "gprod":
            bn.gprod(dn, dd, n=n, num_stride=sn, den_stride=sd, out=out, out_stride=so)
            exp = want.get(op) or ref.gprod(num, den)
        else:
            bn.gsum(ref.mont_words([c]), dd, n=n, den_stride=sd, out=out, out_stride=so)
            exp = want.get(op) or ref.gsum(c, den)
        g = back(out)
        col, idx = column_of(g, n, so)
        differs(col, ref.mont_words(exp), "%s n = %d strides %s" % (op, n, strides))
        rest = np.ones(g.shape[0], bool)
        rest[idx] = False
        assert (g[rest] == SENTINEL).all(), "%s wrote between the elements of its output" % op
        assert np.array_equal(back(dn), wn) and np.array_equal(back(dd), wd), "%s wrote an input" % op


def columns(n, seed, zeros=()):
    num, den = ref.rand_elems(n, seed), [v or 1 for v in ref.rand_elems(n, seed + 1000)]
    for i in zeros:
        den[i] = 0
    return num, den


def geometry(bn):
    """(L, rows of one workgroup's share) of a shape of several workgroups, and that shape's n"""
    n = 3 * 4096 + 37
    p = bn.scan_plan(n)
    assert p["S"] > 2 * p["segsPerWorkgroup"] and p["levels"] >= 3
    return p["L"], p["L"] * p["segsPerWorkgroup"], n


def smallest_n(bn, levels):
    lo, hi = 0, 1 << 20
    assert bn.scan_plan(hi)["levels"] >= levels
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if bn.scan_plan(mid)["levels"] >= levels:
            hi = mid
        else:
            lo = mid
    return hi


# ---- sizes -------------------------------------------------------------------------------------------------------------------------------
def test_sizes_at_the_segment_and_workgroup_edges(bn):
    """n = 1, 2, L - 1, L, L + 1 (one lane's), 64 and 65 (where a second level begins), a last segment of L - 1, L and 1 rows, and one
    workgroup's share - 1, share, share + 1"""
    L, share, _ = geometry(bn)
    edges = {20 * L - 1, 20 * L, 20 * L + 1, share - 1, share, share + 1}
    for n in sorted({1, 2, 3, L - 1, L, L + 1, 63, 64, 65} | edges):
        if n in edges:
            assert bn.scan_plan(n)["L"] == L, "the edge shapes must keep the segment length they are edges of"
        check_all(bn, *columns(n, n))


def test_smallest_shape_of_every_level_count(bn):
    top = bn.scan_plan(1 << 28)["levels"]
    assert top >= 4 and all(bn.scan_plan(1 << 28, op)["levels"] == top for op in bn.SCAN_OPS)
    for levels in range(1, top + 1):
        n = smallest_n(bn, levels)
        assert bn.scan_plan(n)["levels"] == levels and (n == 1 or bn.scan_plan(n - 1)["levels"] == levels - 1)
        num, den = columns(n, levels, zeros=(n // 3,) if n > 2 else ())
        check_all(bn, num, den)


@pytest.fixture(scope="module")
def million():
    n = 1 << 20
    num, den = columns(n, 20, zeros=(n - 77,))
    return num, den


@pytest.mark.parametrize("op", ("batch_inverse", "gprod", "gsum"))
def test_a_million_rows(bn, million, op):
    check_all(bn, *million, ops=(op,))


# ---- zero denominators -------------------------------------------------------------------------------------------------------------------
def test_zero_denominators(bn):
    L, share, n = geometry(bn)
    places = {"row 0": (0,), "row n - 1": (n - 1,), "first row of a segment": (5 * L,), "last row of a segment": (5 * L - 1,),
              "both sides of a workgroup boundary": (share - 1, share), "two in one segment": (7 * L + 2, 7 * L + 9),
              "a whole segment": tuple(range(9 * L, 10 * L)), "every row": tuple(range(n))}
    for what, zeros in places.items():
        num, den = columns(n, 31, zeros)
        z = ref.gprod(num, den)
        first = min(zeros)
        clean = ref.gprod(*columns(n, 31))
        assert z[:first + 1] == clean[:first + 1] and not any(z[first + 1:]), what       # unchanged before, 0 from the row after on
        check_all(bn, num, den, want={"gprod": z})
    # and on the one lane that inverts the total: shapes of a single level
    for n1, zeros in ((1, (0,)), (2, (1,)), (5, (0, 4)), (64, (0, 31, 63)), (64, tuple(range(64)))):
        check_all(bn, *columns(n1, n1 + 40, zeros))


# ---- chosen values -----------------------------------------------------------------------------------------------------------------------
def test_chosen_values(bn):
    pats = [w for _, w in bn128_chosen.PATTERNS]                  # words (Montgomery representations) of zeros-and-ones limbs, below r
    word_vals = [ref.unmont(w) for w in pats + ref.limb_pattern_elems(120, 5) if w]     # the plain values those words spell
    special = [1, R - 1, (1 << 255) % R, 2, R - 2]
    vals = (special + word_vals) * 3
    n = len(vals)
    assert n > 64
    num = ref.rand_elems(n, 1)
    num[3] = num[70] = 0                                          # a zero numerator is ordinary arithmetic
    check_all(bn, num, vals)
    check_all(bn, vals[::-1], vals)
    # den == num: z is 1 on every row
    ones = ref.gprod(vals, vals)
    assert ones == [1] * n
    check_all(bn, vals, vals, ops=("gprod",), want={"gprod": ones})
    # a column whose product over all rows is 1: the last element closes it (z[n] would be 1: z[n - 1] * num / den)
    den = ref.rand_elems(n, 2)
    den = [v or 1 for v in den]
    prod = 1
    for v in den[:-1]:
        prod = prod * v % R
    den[-1] = pow(prod, -1, R)
    z = ref.gprod([1] * n, den)
    assert z[-1] * pow(den[-1], -1, R) % R == 1
    check_all(bn, [1] * n, den, want={"gprod": z})


# ---- addressing and aliasing ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("strides", ((1, 1, 1), (3, 3, 3), (7, 7, 7), (3, 7, 1), (1, 3, 7), (7, 1, 3)))
def test_strides(bn, strides):
    _, share, _ = geometry(bn)
    n = share + 300
    check_all(bn, *columns(n, sum(strides), zeros=(11,)), strides=strides)


@pytest.mark.parametrize("stride", (1, 3, 7))
def test_batch_inverse_in_place(bn, stride):
    for n in (1, 64, 65, 5000):
        _, den = columns(n, n + stride, zeros=(n // 2,))
        w = strided(ref.mont_words(den), stride, 8)
        d = dev(w)
        assert bn.batch_inverse(d, n=n, stride=stride, out=d) is d
        want = w.copy()
        _, idx = column_of(w, n, stride)
        want[idx] = ref.mont_words(ref.batch_inverse(den)).reshape(-1)
        assert np.array_equal(host(d), want), (n, stride)        # the other columns are as they were


def test_columns_of_one_section_interleave(bn):
    n, w = 3000, 3
    num, den = columns(n, 9)
    sec = ref.words(ref.rand_elems(n * w, 10)).reshape(n, w, 4)
    sec[:, 0], sec[:, 1] = ref.mont_words(num), ref.mont_words(den)
    d = dev(sec.reshape(-1))
    bn.batch_inverse(d[4:], n=n, stride=w, out=d[8:], out_stride=w)      # column 1 into column 2
    got = host(d).reshape(n, w, 4)
    assert np.array_equal(got[:, :2], sec[:, :2])
    differs(got[:, 2], ref.mont_words(ref.batch_inverse(den)), "column 2")
    from pil2gl import Pil2glError
    with pytest.raises(Pil2glError):
        bn.gprod(d, d[4:], n=n, num_stride=w, den_stride=w, out=d[4:], out_stride=w)     # a hint never runs in place


# ---- chained, resident -----------------------------------------------------------------------------------------------------------------
def test_eval_program_then_gprod_then_ifft_without_leaving_the_device(bn):
    n_bits = 10
    n = 1 << n_bits
    a, b = ref.rand_elems(n, 61), [v or 1 for v in ref.rand_elems(n, 62)]
    src = dev(fref.matrix_words([a, b]))                          # section 0: a, b
    work = dev(np.zeros((n, 3, 4), np.uint64))                    # section 1: num = a * b (column 0), den = a + b (column 2)
    sec = lambda s, i: (1, 1, s, 0, i)                            # noqa: E731  (SEC, dim, section, prime, column)
    code = [(bn.OPC["mul"], sec(1, 0), sec(0, 0), sec(0, 1)), (bn.OPC["add"], sec(1, 2), sec(0, 0), sec(0, 1))]
    bn.eval_program(code, [src, work], np.zeros((0, 4), np.uint64), n_bits)
    num, den = [x * y % R for x, y in zip(a, b)], [(x + y) % R for x, y in zip(a, b)]
    den_zero = [i for i, v in enumerate(den) if not v]
    committed = dev(ref.words(ref.rand_elems(n * 2, 63)).reshape(n, 2, 4))       # another section: z goes to its column 1
    before = host(committed).copy()
    flat_w, flat_c = work.reshape(-1), committed.reshape(-1)
    bn.gprod(flat_w, flat_w[8:], n=n, num_stride=3, den_stride=3, out=flat_c[4:], out_stride=2)
    z = ref.gprod(num, den)
    assert not den_zero or not any(z[den_zero[0] + 1:])
    got = host(committed)
    differs(got[:, 1], ref.mont_words(z), "z")
    assert np.array_equal(got[:, 0], before[:, 0])
    assert ref.plain(got[n - 1, 1]) == [z[n - 1]]                 # the hint's result field
    coefs = bn.ifft(committed, 2, n_bits)
    want = fref.matrix_words([fref.intt(ref.plain(before[:, 0])), fref.intt(z)])
    assert np.array_equal(host(coefs).reshape(n, 2, 4), want)


# ---- host-pointer forms ------------------------------------------------------------------------------------------------------------------
def test_host_pointer_forms_equal_the_device_forms(bn):
    n = 4500
    num, den = columns(n, 71, zeros=(0, 2000))
    check_all(bn, num, den, strides=(3, 1, 7), on_device=False)
    check_all(bn, num, den, strides=(3, 1, 7), on_device=True)
    w = ref.mont_words(den).reshape(-1)
    assert np.array_equal(bn.batch_inverse(w, out=w).reshape(-1, 4), ref.mont_words(ref.batch_inverse(den)))     # in place on the host


def test_gprod_on_the_host_into_a_column_of_the_inputs_section(bn):
    n, w = 65, 3                                                  # the smallest two-level plan
    assert bn.scan_plan(n, "gprod")["levels"] == 2 and bn.scan_plan(n - 1, "gprod")["levels"] == 1
    num, den = columns(n, 11)
    sec = ref.words(ref.rand_elems(n * w, 12)).reshape(n, w, 4)
    sec[:, 0], sec[:, 1] = ref.mont_words(num), ref.mont_words(den)
    s = sec.reshape(-1).copy()
    bn.gprod(s, s[4:], n=n, num_stride=w, den_stride=w, out=s[8:], out_stride=w)     # columns 0 and 1 into column 2, host pointers
    got = s.reshape(n, w, 4)
    differs(got[:, 2], ref.mont_words(ref.gprod(num, den)), "column 2")
    assert np.array_equal(got[:, :2], sec[:, :2])


def test_no_rows(bn):
    d = dev(ref.mont_words([7]))
    bn.batch_inverse(d, n=0, out=d)
    bn.gprod(d, d, n=0, out=d)
    bn.gsum(ref.mont_words([3]), d, n=0, out=d)
    assert ref.plain(host(d)) == [7]
