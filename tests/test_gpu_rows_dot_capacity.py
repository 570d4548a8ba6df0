"""The row-sum kernels of csrc/dot.hip with operands that fill their unreduced accumulators, and the FRI combine step against plain
extension arithmetic.  Every device comparison is exact equality of canonical words with sum(m[r][c] * w[o][c][k]) mod p (or the Horner
sum of the combine step) in Python integers, on every row of every call; every row-sum call is bracketed by the launch counters
(pil2gl_debug_rows_dot_launches), so that a case is known to have run on the kernel it names.

Which bound each case leans on (move the case when the bound moves):

rows_dot_kernel / rows_dot_stream_kernel (the vector kernels)
  - six u64 sums S[h][l] += half_h * limb_l per output component, halves of 32 bits, limbs of 22 / 22 / 20 bits, folded once per launch;
    the host cuts a matrix into windows of 1024 columns (dot.hip, rows_dot_ext_plain).  1024 (2^32 - 1)(2^22 - 1) = 2^64 - 2^42 - 2^32 +
    2^10 fits, 1025 such terms do not.
  - which (value, weight) pair fills which sum at 1024 terms (test_reference_side_vector_sums_fill_at_1024_and_wrap_at_1025):
      S[0][0]  value 0xFFFFFFFEFFFFFFFF (low half 2^32 - 1)  x  weight 2^44 - 1 or 0xFFFFFFFEFFFFFFFF (limb 0 all ones)
      S[0][1]  value 0xFFFFFFFEFFFFFFFF                      x  weight 2^44 - 1 (limb 1 all ones)
      S[1][0]  value P - 1 (high half 2^32 - 1)              x  weight 2^44 - 1 or 0xFFFFFFFEFFFFFFFF
      S[1][1]  value P - 1                                   x  weight 2^44 - 1
    S[0][2] and S[1][2] take the 20-bit limb: 1024 terms reach 2^62 at the most and cannot fill the register.
  - the stream kernel's four waves split the columns of a window and add their sums in LDS: the total is still one window's 1024 terms.
  - a window of under 32 columns (the one-column tail of 1025 and 2049) goes to the column-tile kernel whatever the switches say.
rows_dot_mfma_kernel (the matrix cores)
  - sixteen i32 plane sums per output started at MF_PLANE_OFFSET = 2^24: a plane takes up to 8 (byte - 128) x (signed digit) pairs of
    magnitude 2^14 at the most per column over MF_MAXW = 112 staged columns.  The largest plane magnitude the model finds over the
    inputs of this file is 8 * 112 * 2^14 = 14680064 = 0.875 * 2^24 (value 0 against weight 0x7F7F7F7F7F7F7F80, whose digits are -128
    eight times, then +1: plane 7 is all (-128)(-128)); the most negative plane is -8 * 112 * 128 * 127 = -14565376 (value 0 against
    weight 0x7F7F7F7F7F7F7F7F, digits +127).  The recombined w[j] stay below 2^50 (test_reference_side_mfma_planes_stay_inside_the_offset).
fri_combine_kernel: add, sub and e3_mul on canonical words, whose edge is P - 1.

The tests named test_reference_side_* need no device.
"""
import ctypes as C
import itertools

import numpy as np
import pytest

from conftest import P, rand_field

pytestmark = pytest.mark.gpu

EINVAL = -1
MFMA, STREAM, TILE = 0, 1, 2

LOW_FULL = 0xFFFFFFFEFFFFFFFF           # canonical, low half 2^32 - 1 (high half 2^32 - 2)
LIMBS01_FULL = (1 << 44) - 1            # limbs 0 and 1 all ones, limb 2 zero
DIGITS_MIN = 0x7F7F7F7F7F7F7F80         # canonical; signed base-256 digits -128 eight times, then +1

VEC_VALUES = [LOW_FULL, P - 1, 0, 1]
VEC_WEIGHTS = [LIMBS01_FULL, LOW_FULL, P - 1]
VEC_WIDTHS = [1024, 1025, 2048, 2049]
VEC_WINDOW = 1024                       # rows_dot_ext_plain's window
VEC_STREAM_MIN = 32                     # narrower windows go to the column-tile kernel

MF_VALUES = [0, 0x8080808080808080, 0x7F7F7F7F7F7F7F7F, P - 1, LOW_FULL, 0x00FF00FF00FF00FF]
MF_WEIGHTS = [DIGITS_MIN, 0x7F7F7F7F7F7F7F7F, 0x8080808080808080, P - 1, 1, 0]
MF_MAXW, MF_PLANE_OFFSET = 112, 1 << 24
# widths of the matrices of a call -> launches of one sweep (rows_dot_mfma_plan: 113 columns are windows of 58 and 55, 58 + 56 > 112)
MF_SHAPES = [((32,), 1), ((112,), 1), ((111,), 1), ((27, 27, 27, 27), 1), ((2, 18, 81, 6), 1), ((113,), 2)]


@pytest.fixture(scope="module")
def gl():
    import pil2gl
    pil2gl.init(0)
    return pil2gl


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


def dev_filled(n, word=0):
    import torch
    return torch.from_numpy(np.full(n, word, np.uint64).view(np.int64)).cuda()


def host(t):
    return t.cpu().numpy().view(np.uint64)


def same(got, want, what=""):
    got, want = np.asarray(got, dtype=np.uint64).reshape(-1), np.asarray(want, dtype=np.uint64).reshape(-1)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, "%s: %d words differ, first at %d: got %#x, want %#x" % (what, bad.size, bad[0], int(got[bad[0]]), int(want[bad[0]]))


def launches(gl):
    out = (C.c_uint64 * 3)()
    assert gl._lib.load().pil2gl_debug_rows_dot_launches(out) == 0
    return [int(v) for v in out]


# ------------------------------------------------------------------------------------------------------------------ 1. reference side
def exact_sum(values, weights):
    return sum(v * w for v, w in zip(values, weights)) % P


def vector_model(values, weights, window, wrapped=range(6)):
    """the six-sum accumulation of rows_dot_kernel / rows_dot_stream_kernel over one row and one weight component, cut into windows of
    `window` columns as rows_dot_ext_plain cuts them: the sums named in `wrapped` are 64-bit registers, the others exact; each window is
    folded as fold6 folds it and added to the windows before it"""
    res = 0
    for c0 in range(0, len(values), window):
        S = [0] * 6
        for v, w in zip(values[c0:c0 + window], weights[c0:c0 + window]):
            half = (v & 0xFFFFFFFF, v >> 32)
            limb = (w & 0x3FFFFF, (w >> 22) & 0x3FFFFF, w >> 44)
            for h in range(2):
                for l in range(3):
                    S[3 * h + l] += half[h] * limb[l]
        S = [s % (1 << 64) if i in wrapped else s for i, s in enumerate(S)]
        res += S[0] + (S[1] << 22) + (S[2] << 44) + (S[3] << 32) + (S[4] << 54) + (S[5] << 76)
    return res % P


def test_reference_side_vector_sums_fill_at_1024_and_wrap_at_1025():
    """the operands of test_vector_kernels_at_capacity against the model: with windows of 1024 columns every sum is exact at every width of
    that test; with windows of 1025 each of S[0][0], S[0][1], S[1][0], S[1][1] -- taken alone as the only 64-bit register -- wraps under
    the pair that maximises it and the folded result is wrong, so a window one column too long fails the device test.  S[0][2] and
    S[1][2] take the 20-bit limb: 1024 terms stay below 2^62 and 1025 below 2^63, they cannot be filled by any operand."""
    assert all(0 <= x < P for x in VEC_VALUES + VEC_WEIGHTS)
    for v in VEC_VALUES:
        for w in VEC_WEIGHTS:
            for n in VEC_WIDTHS:
                assert vector_model([v] * n, [w] * n, VEC_WINDOW) == exact_sum([v] * n, [w] * n) == n * v * w % P, (hex(v), hex(w), n)
    # (the sum, the pair that maximises it)
    fills = [(0, LOW_FULL, LIMBS01_FULL), (0, LOW_FULL, LOW_FULL), (1, LOW_FULL, LIMBS01_FULL),
             (3, P - 1, LIMBS01_FULL), (3, P - 1, LOW_FULL), (4, P - 1, LIMBS01_FULL)]
    assert {i for i, _, _ in fills} == {0, 1, 3, 4}
    full = (2 ** 32 - 1) * (2 ** 22 - 1)
    assert 1024 * full == 2 ** 64 - 2 ** 42 - 2 ** 32 + 2 ** 10 < 2 ** 64 <= 1025 * full
    for i, v, w in fills:
        half, limb = (v & 0xFFFFFFFF, v >> 32)[i // 3], (w & 0x3FFFFF, (w >> 22) & 0x3FFFFF, w >> 44)[i % 3]
        assert half * limb == full, (i, hex(v), hex(w))                      # the largest term the sum can take, in every column
        for n in (1025, 2049):
            assert vector_model([v] * n, [w] * n, 1025, wrapped=[i]) != exact_sum([v] * n, [w] * n), (i, hex(v), hex(w), n)
            assert vector_model([v] * n, [w] * n, 1025) != exact_sum([v] * n, [w] * n), (i, hex(v), hex(w), n)
        assert vector_model([v] * 1024, [w] * 1024, 1025, wrapped=[i]) == exact_sum([v] * 1024, [w] * 1024)
    # the 20-bit limb: the largest canonical word has limb 2 = 0xFFFFF
    assert (P - 1) >> 44 == 0xFFFFF and all(w >> 44 <= 0xFFFFF for w in VEC_WEIGHTS)
    assert 1024 * (2 ** 32 - 1) * 0xFFFFF < 2 ** 62 and 1025 * (2 ** 32 - 1) * 0xFFFFF < 2 ** 63
    for i in (2, 5):
        assert vector_model([P - 1] * 1025, [P - 1] * 1025, 1025, wrapped=[i]) == exact_sum([P - 1] * 1025, [P - 1] * 1025)


def signed_digits(w):
    """launch_rows_dot_mfma's recoding: nine signed base-256 digits in [-128, 127] with sum_j d_j 2^(8j) = w"""
    d, carry = [], 0
    for j in range(9):
        b = ((w >> (8 * j)) & 255 if j < 8 else 0) + carry
        carry = 0
        if b >= 128:
            b -= 256; carry = 1
        d.append(b)
    assert carry == 0 and all(-128 <= x <= 127 for x in d) and sum(x << (8 * j) for j, x in enumerate(d)) == w
    return d


def mfma_planes(values, weights):
    """the sixteen plane sums of one row and one output: G[p] = sum_c sum_i (byte_i(m[c]) - 128) * d_(p - i)(w[c]), as the matrix
    instruction accumulates them (bytes fed as b ^ 0x80, digit tables as atab lays them out: j = p - i in 0..8)"""
    G = [0] * 16
    for v, w in zip(values, weights):
        d = signed_digits(w)
        for i in range(8):
            b = ((v >> (8 * i)) & 255) - 128
            for j in range(9):
                G[i + j] += b * d[j]
    return G


def mfma_model(values, weights):
    """what the kernel makes of the planes: accumulators started at the offset, recombined into four words, folded, the bias added"""
    G = mfma_planes(values, weights)
    acc = [g + MF_PLANE_OFFSET for g in G]
    assert all(0 <= a < 2 ** 31 for a in acc)
    w = [sum(acc[4 * j + k] << (8 * k) for k in range(4)) for j in range(4)]
    bias = (sum(128 << (8 * i) for i in range(8)) * sum(weights) - sum(MF_PLANE_OFFSET << (8 * p) for p in range(16))) % P
    return (w[0] + (w[1] << 32) + (w[2] << 64) + (w[3] << 96) + bias) % P, G, w


def test_reference_side_mfma_planes_stay_inside_the_offset():
    """every (value, weight) pair of test_mfma_kernel_at_its_extremes in all 112 staged columns: the plane sums stay above -2^24 (the
    accumulators, started at 2^24, never go negative), 2^24 + max stays an i32, the recombined words stay below 2^50 (canonical operands
    for add and sub), and the model's result is the exact sum.  The weight 0x7F7F7F7F7F7F7F80 is canonical and the only one whose eight
    low digits are all -128: against all-zero values (bytes fed as -128) plane 7 reaches 8 * 112 * 2^14 = 0.875 * 2^24, the figure the
    kernel's comment leans on.  That is the positive side; the side the offset guards is the negative one, where the extreme is
    all-zero values against 0x7F7F7F7F7F7F7F7F (digits +127): -8 * 112 * 128 * 127 = -14565376."""
    assert all(0 <= x < P for x in MF_VALUES + MF_WEIGHTS)
    assert signed_digits(DIGITS_MIN) == [-128] * 8 + [1]
    assert [w for w in MF_WEIGHTS if signed_digits(w)[:8] == [-128] * 8] == [DIGITS_MIN]
    lo, hi, wmax = 0, 0, 0
    for v in MF_VALUES:
        for w in MF_WEIGHTS:
            got, G, words = mfma_model([v] * MF_MAXW, [w] * MF_MAXW)
            assert got == exact_sum([v] * MF_MAXW, [w] * MF_MAXW), (hex(v), hex(w))
            lo, hi, wmax = min(lo, min(G)), max(hi, max(G)), max(wmax, max(words))
    assert lo > -2 ** 24 and MF_PLANE_OFFSET + hi < 2 ** 31
    assert wmax < 2 ** 50
    G = mfma_planes([0] * MF_MAXW, [DIGITS_MIN] * MF_MAXW)
    assert max(G) == G[7] == hi == 8 * MF_MAXW * 2 ** 14 == 14680064
    G = mfma_planes([0] * MF_MAXW, [0x7F7F7F7F7F7F7F7F] * MF_MAXW)
    assert min(G) == G[7] == lo == -8 * MF_MAXW * 128 * 127 == -14565376
    # no operand at all can pass the offset at this width: 8 pairs of magnitude 2^14 at the most per column
    assert 8 * MF_MAXW * 128 * 128 < 2 ** 24


def test_reference_side_mfma_shapes_are_planned_as_the_device_test_assumes():
    """rows_dot_mfma_plan in Python integers for the shapes of the device test: windows of at most 112 staged columns (an odd width
    counted as the next even one), largest first into launches of at most four segments, every launch at least 32 columns wide"""
    for widths, n_launch in MF_SHAPES:
        wins = []
        for W in widths:
            n = (W + (W & 1) + MF_MAXW - 1) // MF_MAXW
            per = (W + n - 1) // n; per += per & 1
            wins += [min(per, W - c0) for c0 in range(0, W, per)]
        bins = []
        for w in sorted(wins, reverse=True):
            pw = w + (w & 1)
            for b in bins:
                if len(b) < 4 and sum(b) + pw <= MF_MAXW:
                    b.append(pw); break
            else:
                bins.append([pw])
        assert len(bins) == n_launch and all(32 <= sum(b) <= MF_MAXW for b in bins), (widths, bins)


def test_reference_side_launch_counter_needs_no_device():
    """three host counters: readable before any device call, monotonic, a null buffer refused"""
    from pil2gl import _lib
    lib = _lib.load()
    a, b = (C.c_uint64 * 3)(), (C.c_uint64 * 3)()
    assert lib.pil2gl_debug_rows_dot_launches(a) == 0 and lib.pil2gl_debug_rows_dot_launches(b) == 0
    assert list(a) == list(b)
    assert lib.pil2gl_debug_rows_dot_launches(None) == EINVAL


# ------------------------------------------------------------------------------------------------------------------ 2. vector kernels
def rows_dot_constant_rows(gl, widths, row_values, out_weights, accumulate):
    """matrices of the given widths whose row r holds row_values[r] in every column, output o weighing every column (all three
    components) with out_weights[o] -> (rc, acc as rows x nOut x 3, launch counts of the call); accumulate: onto an acc full of P - 1"""
    lib = gl._lib.load()
    n_rows, n_out, n = len(row_values), len(out_weights), len(widths)
    col = np.array(row_values, dtype=np.uint64).reshape(n_rows, 1)
    mats = [dev(np.repeat(col, w, axis=1)) for w in widths]
    coefs = [np.ascontiguousarray(np.broadcast_to(np.array(out_weights, dtype=np.uint64).reshape(n_out, 1, 1), (n_out, w, 3))) for w in widths]
    ptrs = (C.c_void_p * n)(*[t.data_ptr() for t in mats])
    cps = (C.c_void_p * n)(*[c.ctypes.data for c in coefs])
    ws = np.array(widths, dtype=np.uint64)
    acc = dev_filled(n_rows * n_out * 3, P - 1 if accumulate else 0x7777)
    before = launches(gl)
    rc = lib.pil2gl_rows_dot_ext_multi_dev(ptrs, C.c_void_p(ws.ctypes.data), n, n_rows, cps, n_out, C.c_void_p(acc.data_ptr()), accumulate, None)
    after = launches(gl)
    return rc, host(acc).reshape(n_rows, n_out, 3), [a - b for a, b in zip(after, before)]


def expected_rows(widths, row_values, out_weights, accumulate):
    """sum(m[r][c] * w[o][c][k]) mod p over all columns of all matrices, once per distinct row value"""
    base = P - 1 if accumulate else 0
    per = {}
    for v in set(row_values):
        per[v] = [(base + sum(v * w for wd in widths for _ in range(wd))) % P for w in out_weights]
    return np.array([[[per[v][o]] * 3 for o in range(len(out_weights))] for v in row_values], dtype=np.uint64)


@pytest.mark.parametrize("n_out", [1, 4])
@pytest.mark.parametrize("width", VEC_WIDTHS)
@pytest.mark.parametrize("mode", ["stream", "tile"])
def test_vector_kernels_at_capacity(gl, monkeypatch, mode, width, n_out):
    """windows exactly full (1024, 2048) and full windows followed by a one-column window (1025, 2049) of rows that hold one value with
    a half at 2^32 - 1 against weights with limbs of all ones: the pairs test_reference_side_vector_sums_fill_at_1024_and_wrap_at_1025
    shows to fill S[0][0], S[0][1], S[1][0], S[1][1] with 1024 terms and to wrap them with 1025.  65 rows: a full 64-row tile and one
    row of the next.  Output o takes weight (o + k) mod 3 in call k, so every output meets every weight.  Then the same onto an acc
    full of P - 1, the top edge of add(v, out)."""
    monkeypatch.setenv("PIL2GL_ROWS_DOT_MFMA", "0")
    if mode == "tile":
        monkeypatch.setenv("PIL2GL_ROWS_DOT_STREAM", "0")
    else:
        monkeypatch.delenv("PIL2GL_ROWS_DOT_STREAM", raising=False)
    n_rows = 65
    row_values = [VEC_VALUES[r % len(VEC_VALUES)] for r in range(n_rows)]
    full, tail = divmod(width, VEC_WINDOW)
    assert tail < VEC_STREAM_MIN
    want_launches = [0, 0, full + (tail > 0)] if mode == "tile" else [0, full, int(tail > 0)]
    for k in range(len(VEC_WEIGHTS)):
        out_weights = [VEC_WEIGHTS[(o + k) % len(VEC_WEIGHTS)] for o in range(n_out)]
        for accumulate in (0, 1):
            rc, got, took = rows_dot_constant_rows(gl, [width], row_values, out_weights, accumulate)
            assert rc == 0
            assert took == want_launches, (mode, width, took)
            same(got, expected_rows([width], row_values, out_weights, accumulate),
                 "%s, width %d, weights %s, accumulate %d" % (mode, width, [hex(w) for w in out_weights], accumulate))


# ------------------------------------------------------------------------------------------------------------------ 3. matrix cores
@pytest.mark.parametrize("n_out", [1, 2, 4])
@pytest.mark.parametrize("widths,n_launch", MF_SHAPES)
def test_mfma_kernel_at_its_extremes(gl, monkeypatch, widths, n_launch, n_out):
    """whole rows of one extreme byte pattern against whole weight vectors of one extreme digit pattern, at the narrowest (32) and the
    widest (112) staged row, an odd width (111: the ODD form, padded to 112), four odd segments (27 x 4: 112 staged), the permutation
    AIR's widths, and one column too many (113: two windows, two launches).  Four outputs are two sweeps of the same launches.
    129 rows: two full 64-row tiles (both 32-row groups of each) and one row of a third.  Default switches: the counters must show
    the matrix-core kernel alone."""
    monkeypatch.delenv("PIL2GL_ROWS_DOT_MFMA", raising=False)
    monkeypatch.delenv("PIL2GL_ROWS_DOT_STREAM", raising=False)
    n_rows = 129
    row_values = [MF_VALUES[r % len(MF_VALUES)] for r in range(n_rows)]
    sweeps = (n_out + 1) // 2
    for w in MF_WEIGHTS:
        for accumulate in (0, 1):
            rc, got, took = rows_dot_constant_rows(gl, list(widths), row_values, [w] * n_out, accumulate)
            assert rc == 0
            assert took == [sweeps * n_launch, 0, 0], (widths, n_out, took)
            same(got, expected_rows(widths, row_values, [w] * n_out, accumulate),
                 "widths %s, %d outputs, weight %#x, accumulate %d" % (widths, n_out, w, accumulate))


# ------------------------------------------------------------------------------------------------------------------ 4. FRI combine
def e3_mul(a, b):
    """the cubic extension u^3 = u + 1 (oracle/gl_oracle.py, f3g.js:94-102), schoolbook"""
    d0, d1, d2 = a[0] * b[0], a[0] * b[1] + a[1] * b[0], a[0] * b[2] + a[1] * b[1] + a[2] * b[0]
    d3, d4 = a[1] * b[2] + a[2] * b[1], a[2] * b[2]
    return ((d0 + d3) % P, (d1 + d3 + d4) % P, (d2 + d4) % P)         # u^3 = u + 1, u^4 = u^2 + u


def combine_reference(acc, K, vf1, xdiv, order):
    """f[r] = Horner over vf1 of (acc[r][o] - K_o) * X[r][o], the k-th term being opening order[k] (friPolinomial.js:38-50)"""
    f = []
    for a_row, x_row in zip(acc, xdiv):
        res = None
        for o in order:
            t = e3_mul([(a_row[o][q] - K[o][q]) % P for q in range(3)], x_row[o])
            res = t if res is None else tuple((x + y) % P for x, y in zip(e3_mul(vf1, res), t))
        f.append(res)
    return f


COMBINE_ROWS = [1, 255, 256, 257]
COMBINE_ORDERS = {1: [(0,)], 2: [(0, 1), (1, 0)], 3: list(itertools.permutations(range(3))), 4: [(0, 1, 2, 3), (3, 2, 1, 0), (1, 2, 0, 3)]}


def combine(gl, dacc, K, vf1, dx, n_open, order, n_rows):
    lib = gl._lib.load()
    f = dev_filled(3 * n_rows, 0x7777)
    Kh = np.array(K, dtype=np.uint64).reshape(-1); vh = np.array(vf1, dtype=np.uint64)
    args = (C.c_void_p(dacc.data_ptr()), gl._ptr(Kh), gl._ptr(vh), C.c_void_p(dx.data_ptr()), n_open)
    if order is None:
        rc = lib.pil2gl_fri_combine_dev(*args, n_rows, C.c_void_p(f.data_ptr()), None)
    else:
        oh = np.array(order, dtype=np.uint32)
        rc = lib.pil2gl_fri_combine_order_dev(*args, C.c_void_p(oh.ctypes.data), n_rows, C.c_void_p(f.data_ptr()), None)
    return rc, host(f).reshape(n_rows, 3)


@pytest.mark.parametrize("n_open", [1, 2, 3, 4])
def test_fri_combine_against_plain_extension_arithmetic(gl, n_open):
    """pil2gl_fri_combine_order_dev in every order of the list (all six for three openings), and pil2gl_fri_combine_dev where the order is
    the identity, on 1, 255, 256 and 257 rows (a lane, a block less one, a block, a block and one): random rows, rows whose bracket
    acc - K is zero in every opening or in one, rows of P - 1 in every word of acc and X, rows of zero acc; K random and K of P - 1 in
    every word; vf1 of P - 1 in every word, zero, one and random.  The reference is computed once per (K, vf1, order) on 257 rows; the
    shorter calls read the same buffers and must give its first rows."""
    rng = np.random.default_rng(40 + n_open)
    n_max = max(COMBINE_ROWS)
    for K in ([[int(v) for v in k] for k in rand_field(rng, (n_open, 3))], [[P - 1] * 3] * n_open):
        acc = rand_field(rng, (n_max, n_open, 3)); xd = rand_field(rng, (n_max, n_open, 3))
        Ka = np.array(K, dtype=np.uint64)
        for r in range(n_max):
            kind = r % 6
            if kind == 1:
                acc[r] = Ka                                          # the bracket is zero in every opening
            elif kind == 2:
                acc[r] = P - 1; xd[r] = P - 1
            elif kind == 3:
                acc[r, r % n_open] = Ka[r % n_open]                  # zero in one opening only
            elif kind == 4:
                acc[r] = 0; xd[r, :, 1:] = P - 1                     # 0 - K, the borrow of sub
        dacc, dx = dev(acc), dev(xd)
        acc_l, xd_l = acc.tolist(), xd.tolist()
        for vf1 in ((P - 1, P - 1, P - 1), (0, 0, 0), (1, 0, 0), tuple(int(v) for v in rand_field(rng, 3))):
            for order in COMBINE_ORDERS[n_open]:
                want = np.array(combine_reference(acc_l, K, vf1, xd_l, order), dtype=np.uint64)
                for n_rows in COMBINE_ROWS:
                    rc, got = combine(gl, dacc, K, vf1, dx, n_open, order, n_rows)
                    assert rc == 0
                    same(got, want[:n_rows], "nOpen %d, order %s, vf1 %s, %d rows" % (n_open, order, vf1, n_rows))
                    if order == tuple(range(n_open)):
                        rc, got = combine(gl, dacc, K, vf1, dx, n_open, None, n_rows)
                        assert rc == 0
                        same(got, want[:n_rows], "nOpen %d, identity call, vf1 %s, %d rows" % (n_open, vf1, n_rows))


def test_fri_combine_refuses_bad_orders_and_opening_counts(gl):
    rng = np.random.default_rng(5)
    n_rows = 3
    dacc = dev(rand_field(rng, (n_rows, 5, 3))); dx = dev(rand_field(rng, (n_rows, 5, 3)))
    K = [[1, 2, 3]] * 5
    for n_open, order in [(2, (0, 0)), (2, (0, 2)), (3, (0, 1, 1)), (4, (0, 1, 2, 4)), (0, (0, 1, 2, 3)), (5, (0, 1, 2, 3, 4))]:
        rc, f = combine(gl, dacc, K, (1, 2, 3), dx, n_open, order, n_rows)
        assert rc == EINVAL and (f == 0x7777).all(), (n_open, order)
    for n_open in (0, 5):
        rc, f = combine(gl, dacc, K, (1, 2, 3), dx, n_open, None, n_rows)
        assert rc == EINVAL and (f == 0x7777).all(), n_open
