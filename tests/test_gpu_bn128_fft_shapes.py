"""BN254 Fr transforms on the device (csrc/bn_ntt.hip) at the shapes where its tile geometry changes: several column groups with a
narrower last one, in one sweep below the largest tile and across the seam of two sweeps; chosen words in every twiddle product; and a
dense closed form through both seams of three sweeps.  Every comparison is exact equality of the Montgomery words, against the Python
checker (tests/bn128_fft_ref.py).  Every threshold is read from the library's plan (pil2gl_debug_bn128_fft_plan, _tile_bytes), and each
group of shapes asserts from the plan that it lies on the edge it names."""
import ctypes as C
import functools
import random

import numpy as np
import pytest

import bn128_fft_dif as dif
import bn128_fft_ref as ref
from bn128_fft_ref import R
from test_gpu_bn128_fft import chosen_pairs, host, max_single_sweep, same

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def bn():
    import pil2gl
    from pil2gl import bn128
    pil2gl.init(0)
    return bn128


def _lib():
    import pil2gl
    return pil2gl.load()


def dev(words):
    return torch.from_numpy(np.array(words).view(np.int64)).cuda()          # a copy: the shared inputs stay as they are


# ---- the plan ----------------------------------------------------------------------------------------------------------------------
def plan(n_bits):
    layers = (C.c_uint32 * 8)(); n = C.c_uint32()
    assert _lib().pil2gl_debug_bn128_fft_plan(n_bits, layers, 8, C.byref(n)) == 0
    return list(layers[:n.value])


def cap(k):
    """columns a tile of a sweep of k layers holds"""
    return (_lib().pil2gl_debug_bn128_fft_tile_bytes() // 32) >> k


def groups(n_pols, k):
    """widths of the column groups of a sweep of k layers over n_pols columns"""
    cg = min(n_pols, cap(k))
    return [min(cg, n_pols - c0) for c0 in range(0, n_pols, cg)]


def smallest_with_sweeps(s):
    n_bits = 1
    while len(plan(n_bits)) < s:
        n_bits += 1
    assert len(plan(n_bits)) == s
    return n_bits


# ---- inputs and references, made once ------------------------------------------------------------------------------------------------
def chosen_columns(n_pols):
    """two columns of the first group and the last two: the last group where it has two columns, the seam between the last two groups
    where it has one"""
    return sorted({0, 1 % n_pols, max(n_pols - 2, 0), n_pols - 1})


def dense_input(n_bits, n_pols, seed):
    """random canonical words; the chosen words of chosen_pairs() cycled down the rows of chosen_columns()"""
    rng = random.Random(seed)
    n = 1 << n_bits
    vals = [rng.randrange(R) for _ in range(n * n_pols)]
    flat = [v for p in chosen_pairs() for v in p]
    for i, c in enumerate(chosen_columns(n_pols)):
        for j in range(n):
            vals[j * n_pols + c] = flat[(j + 7 * i * n) % len(flat)]
    x = ref.pack_words(vals).reshape(n, n_pols, 4)
    assert all(v < R for v in vals)
    return x


def cols_words(cols):
    """ref.matrix_words, packed in one go"""
    rows, n_pols = len(cols[0]), len(cols)
    return frozen(ref.pack_words([ref.to_mont(cols[i][j]) for j in range(rows) for i in range(n_pols)]).reshape(rows, n_pols, 4))


def transform_words(fn, words):
    """ref.apply_cols"""
    return cols_words([fn(c) for c in ref.matrix_cols(words)])


def frozen(a):
    a = np.array(a)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def dense_case(n_bits, n_pols):
    """(input, its fft, its ifft) by the checker"""
    x = frozen(dense_input(n_bits, n_pols, 7000 + 100 * n_bits + n_pols))
    return x, transform_words(ref.ntt, x), transform_words(ref.intt, x)


def check_device_forms(bn, n_bits, n_pols, in_place):
    x, f, fi = dense_case(n_bits, n_pols)
    same(host(bn.fft(dev(x), n_pols, n_bits)), f)
    same(host(bn.ifft(dev(x), n_pols, n_bits)), fi)
    if in_place:
        d = dev(x); r = bn.fft(d, n_pols, n_bits, out=d)
        assert r.data_ptr() == d.data_ptr()
        same(host(d), f)
        d = dev(x); bn.ifft(d, n_pols, n_bits, out=d)
        same(host(d), fi)


# ---- A: two sweeps, several column groups ------------------------------------------------------------------------------------------------
A_NAMES = ("c0+1", "c1", "c1+1", "2c0-1")


def two_sweep_shape(which):
    """(n_bits, n_pols) of case `which`, after asserting from the plan what its name claims"""
    n_bits = max_single_sweep(_lib()) + 1
    layers = plan(n_bits)
    assert len(layers) == 2 and len(plan(n_bits - 1)) == 1               # the smallest size with a seam
    c0, c1 = cap(layers[0]), cap(layers[1])
    assert 1 < c0 < c1 and c1 % c0 == 0
    n_pols = (c0 + 1, c1, c1 + 1, 2 * c0 - 1)[which]
    g0, g1 = groups(n_pols, layers[0]), groups(n_pols, layers[1])
    assert sum(g0) == sum(g1) == n_pols
    if which == 0:
        assert g0 == [c0, 1] and g1 == [c0 + 1]                          # first sweep split, last sweep not
    elif which == 1:
        assert g0 == [c0] * (c1 // c0) and len(g0) > 1 and g1 == [c1]    # whole groups in both sweeps
    elif which == 2:
        assert g0 == [c0] * (c1 // c0) + [1] and g1 == [c1, 1]           # a narrow last group in both sweeps, at different columns
    else:
        assert g0 == [c0, c0 - 1] and c0 - 1 >= 2                        # a narrow last group of more than one column
    return n_bits, n_pols


@pytest.mark.parametrize("which", range(4), ids=A_NAMES)
def test_two_sweeps_with_several_column_groups(bn, which):
    """every word of fft and ifft, out of place and with dst == src: the seam twiddles of the groups behind the first, the scale and
    the bit-reversed scatter of a last sweep of several groups"""
    n_bits, n_pols = two_sweep_shape(which)
    check_device_forms(bn, n_bits, n_pols, in_place=True)


def test_two_sweeps_host_pointer_forms(bn):
    n_bits, n_pols = two_sweep_shape(2)
    x, f, fi = dense_case(n_bits, n_pols)
    same(bn.fft(np.array(x), n_pols, n_bits), f)
    same(bn.ifft(np.array(x), n_pols, n_bits), fi)
    h = np.array(x); bn.fft(h, n_pols, n_bits, out=h)
    same(h, f)
    h = np.array(x); bn.ifft(h, n_pols, n_bits, out=h)
    same(h, fi)


def test_interpolate_into_two_sweeps_with_several_column_groups(bn):
    """a one-sweep ifft of many narrow groups, then the two-sweep fft in place in the extended buffer; coefficients returned"""
    n_ext, n_pols = two_sweep_shape(2)
    n_bits = n_ext - 2
    assert len(plan(n_bits)) == 1 and len(groups(n_pols, n_bits)) > 1 and groups(n_pols, n_bits)[-1] < cap(n_bits)
    x = frozen(dense_case(n_ext, n_pols)[0][:1 << n_bits])
    want = [ref.interpolate(c, n_ext) for c in ref.matrix_cols(x)]
    w_coefs, w_ext = cols_words([c for c, _ in want]), cols_words([e for _, e in want])
    coefs, ext = bn.interpolate(dev(x), n_pols, n_bits, n_ext)
    same(host(coefs), w_coefs); same(host(ext), w_ext)
    coefs, ext = bn.interpolate(np.array(x), n_pols, n_bits, n_ext)
    same(coefs, w_coefs); same(ext, w_ext)


# ---- B: one sweep below the largest tile, more columns than its cap -------------------------------------------------------------------
B_SHAPES = ((1, 1, 1), (3, 1, 1), (5, 1, -1), (5, 1, 0), (5, 1, 1), (5, 2, 1), (9, 1, 1))         # (n_bits, a, b): nPols = a * cap + b


def one_sweep_shape(which):
    n_bits, a, b = B_SHAPES[which]
    assert plan(n_bits) == [n_bits] and n_bits < max_single_sweep(_lib())
    c = cap(n_bits)
    assert c >= 2
    n_pols = a * c + b
    assert groups(n_pols, n_bits) == ([c] * a + [b] if b > 0 else [c] * (a - 1) + [c + b])
    return n_bits, n_pols


@pytest.mark.parametrize("which", range(len(B_SHAPES)), ids=["%d-%dcap%+d" % s for s in B_SHAPES])
def test_one_sweep_with_more_columns_than_the_cap(bn, which):
    n_bits, n_pols = one_sweep_shape(which)
    check_device_forms(bn, n_bits, n_pols, in_place=B_SHAPES[which] == (5, 1, 1))


# ---- C: chosen words in the twiddle products ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_bits", (2, 3))
def test_chosen_words_in_every_twiddle_product(bn, n_bits):
    """bn128_fft_dif.twiddle_cases: each chosen word is the difference a - b that meets each twiddle of a 4- and an 8-row transform"""
    n, n_pols = 1 << n_bits, 8
    words = dif.chosen_words(chosen_pairs())
    cols = []
    for x in words:
        cases = dif.twiddle_cases(n_bits, x)
        for inverse in (False, True):
            met = set().union(*(dif.dif(col, inverse)[1] for col in cases))
            assert {(x, t, j) for t, j in dif.twiddles_of(n_bits)} <= met
        cols += cases
    while len(cols) % n_pols:
        cols.append([0] * n)
    for o in range(0, len(cols), n_pols):                              # nPols 8: a row fills the lanes of the column group
        grp = cols[o:o + n_pols]
        x = ref.pack_words([grp[i][j] for j in range(n) for i in range(n_pols)]).reshape(n, n_pols, 4)
        same(host(bn.fft(dev(x), n_pols, n_bits)), transform_words(ref.ntt, x))
        same(host(bn.ifft(dev(x), n_pols, n_bits)), transform_words(ref.intt, x))


# ---- D: geometric columns, closed form --------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def geometric_case(n_bits, n_pols):
    """((c_p, a_p) per column, the matrix of the columns x_j = c_p a_p^j)"""
    rng = random.Random(2100 + n_bits)
    par = []
    while len(par) < n_pols:
        c, a = rng.randrange(1, R), rng.randrange(2, R)
        if pow(a, 1 << n_bits, R) != 1:
            par.append((c, a))
    return par, frozen(np.stack([ref.geometric_words(c, a, n_bits) for c, a in par], axis=1))


def covering_rows(n_bits, seed):
    """one row in every residue class modulo 2^(n_bits - K), K the layers of the last sweep -- that sweep's tile b stores its rows at
    brev(q) 2^(n_bits - K) + brev(b), so the outputs of one sub-transform are one such class, and an error at a seam before it shows in
    whole classes; plus 0, 1, n/2, n-1 and the first and last output row of every tile of the last sweep"""
    n = 1 << n_bits
    mod = n >> plan(n_bits)[-1]
    rng = random.Random(seed)
    rows = {c + mod * rng.randrange(n // mod) for c in range(mod)}
    assert {k % mod for k in rows} == set(range(mod)) and len(rows) == mod
    rows |= {0, 1, n // 2, n - 1} | set(range(mod)) | set(range(n - mod, n))
    return sorted(rows)


def closed_form_words(par, n_bits, rows, inverse):
    cols = [ref.geometric_ntt_rows(c, a, n_bits, rows, inverse) for c, a in par]
    return ref.pack_words([ref.to_mont(col[i]) for i in range(len(rows)) for col in cols]).reshape(len(rows), len(par), 4)


@pytest.mark.parametrize("inverse", (False, True), ids=("fft", "ifft"))
def test_three_sweeps_on_dense_geometric_columns(bn, inverse):
    """every tile of every sweep carries data, and every sub-transform of the last sweep is sampled: row k of the transform of
    c a^j is c (a^n - 1) / (a w^k - 1)"""
    n_bits, n_pols = smallest_with_sweeps(3), 2
    assert len(plan(n_bits - 1)) == 2
    par, x = geometric_case(n_bits, n_pols)
    rows = covering_rows(n_bits, 31)
    out = (bn.ifft if inverse else bn.fft)(dev(x), n_pols, n_bits)
    same(host(out[torch.tensor(rows, device="cuda")]), closed_form_words(par, n_bits, rows, inverse))


@pytest.mark.parametrize("inverse", (False, True), ids=("fft", "ifft"))
def test_two_sweeps_on_dense_geometric_columns(bn, inverse):
    """the same at the smallest two-sweep size with a split first sweep, on all rows, where the checker can follow: checker, closed
    form and device agree"""
    n_bits, n_pols = two_sweep_shape(0)
    par, x = geometric_case(n_bits, n_pols)
    rows = list(range(1 << n_bits))
    want = closed_form_words(par, n_bits, rows, inverse)
    same(transform_words(ref.intt if inverse else ref.ntt, x), want)
    same(host((bn.ifft if inverse else bn.fft)(dev(x), n_pols, n_bits)), want)
