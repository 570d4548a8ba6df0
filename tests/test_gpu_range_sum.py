"""The range-check grand sum on the device, bit-exact in both fields against the integer checker (tests/range_sum_ref.py) AND against
logup_sum_dev on the materialised columns -- the statement's promise.  Every case goes through run(): the resident form on a non-default
stream, twice, with guard words behind out's matrix; the host form on copies; logup_sum_dev with each range replaced by a k = 1 term over a
materialised t column and m zeroed outside the window; the checker on the same bit patterns, which never looks at m outside a window.  The
m columns are random non-zero words in EVERY row, non-canonical ones among them, so the rows outside a window are poison.  Every input
matrix, the guard words and every word of out's matrix outside the column must come back unchanged (out is strided by default).
Shapes are the smallest at which the kernels can still go wrong: the lane (8 rows) and block (2048 rows) edges of the Goldilocks scan against
the window's two ends, bnscan's level thresholds over Fr."""
import random

import numpy as np
import pytest

import logup_sum_ref as lref
import range_sum_ref as rref
import bn128_hints_ref as bref
import conn_pols_ref as cref
from hints_ref import P

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from pil2gl import pilcheck  # noqa: E402

R, MONT = bref.R, bref.MONT
Q = {"gl": P, "bn128": R}
TOP = {"gl": 1 << 64, "bn128": 1 << 256}
GUARD = 0x6B6B6B6B6B6B6B6B
FIELDS = ("gl", "bn128")
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1


# ---- bit patterns <-> the library's words <-> the checker's values ----
def words(field, rows):
    if field == "gl":
        return np.array(rows, np.uint64).reshape(len(rows), -1)
    return cref.fr_words([v for row in rows for v in row]).reshape(len(rows), -1, 4)


def patterns(w):
    if w.ndim == 2:
        return [[int(v) for v in row] for row in w]
    return [[sum(int(e[k]) << (64 * k) for k in range(4)) for e in row] for row in w]


def value(field, pat):
    """a bit pattern as the checker's integer"""
    return pat % P if field == "gl" else bref.unmont(pat % R)


def pattern_of(field, v):
    """the canonical pattern of a value"""
    return v % P if field == "gl" else v % R * MONT % R


def elem(field, v):
    """a base-field value as the call takes coef / busId"""
    return v % P if field == "gl" else [int(x) for x in cref.fr_words([pattern_of(field, v)])[0]]


def chal_words(field, pat):
    """a challenge's PATTERN as the call takes it: three words, or the four words of one 256-bit pattern"""
    return [int(x) for x in pat] if field == "gl" else [int(x) for x in cref.fr_words([pat])[0]]


def chal_value(field, pat):
    return tuple(x % P for x in pat) if field == "gl" else value(field, pat)


def chal_pattern(field, v):
    return tuple(v) if field == "gl" else pattern_of(field, v)


def s_words(field, s):
    """the checker's s as the words the column must hold: (n, 3) or (n, 4)"""
    if field == "gl":
        return np.array(s, np.uint64).reshape(len(s), 3)
    return cref.fr_words([v * MONT % R for v in s])


def to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


def rand_rows(rng, field, n, stride):
    return [[rng.randrange(Q[field]) for _ in range(stride)] for _ in range(n)]


def poison_rows(rng, field, n, stride):
    """non-zero words in every row, one in three at or above the modulus"""
    q, top = Q[field], TOP[field]
    return [[rng.choice((q, q + 1, top - 1, q + rng.randrange(top - q))) if rng.randrange(3) == 0 else 1 + rng.randrange(q - 1) for _ in range(stride)] for _ in range(n)]


def rand_chal(rng, field):
    return tuple(rng.randrange(P) for _ in range(3)) if field == "gl" else rng.randrange(R)


def neg(field, a):
    return tuple((P - x) % P for x in a) if field == "gl" else (R - a) % R


def zero_beta(field, rng_spec, alpha, i):
    """the beta that makes E of this range zero at row i"""
    F = lref.FIELDS[field]
    return neg(field, rref.range_denominator(F, rng_spec, F.ext(alpha), F.zero, i))


_STREAM = []


def side_stream():
    """one non-default stream for the whole module"""
    if not _STREAM:
        _STREAM.append(torch.cuda.Stream())
    return _STREAM[0]


def materialised(field, ranges, pats, n):
    """the matrix of the statement's promise: for range r the column 2 r = t_r as canonical patterns, 2 r + 1 = m_r's pattern inside the window, 0 outside"""
    rows = [[0] * (2 * len(ranges)) for _ in range(n)]
    for r, (name, col, lo, size, row0, _, _) in enumerate(ranges):
        for i in range(n):
            rows[i][2 * r] = pattern_of(field, lo + min(max(i - row0, 0), size - 1))
            rows[i][2 * r + 1] = pats[name][i][col] if row0 <= i < row0 + size else 0
    return rows


def run(field, mats, terms, ranges, alpha, beta, n, out=None, raw=None, host_form=True):
    """mats: name -> rows of bit patterns; terms: (name, cols, (numerator's name, col) or None, coef, bus); ranges: (m's name, col, lo, size,
    row0, coef, bus); coef and bus VALUES; alpha, beta: values (a triple / an integer) or, with raw, bit patterns; out: (name, col), default a
    matrix of its own with stride gaps -> s as the checker gives it, which the resident form (twice), the host form and logup_sum_dev on
    the materialised columns gave too"""
    width = 3 if field == "gl" else 1
    mats = dict(mats)
    if out is None:
        out = ("$out", 1)
        mats["$out"] = [[(0xD00D << 32) + 7 * i + j for j in range(width + 2)] for i in range(n)]
    host = {name: words(field, rows) for name, rows in mats.items()}
    pats = {name: patterns(w) for name, w in host.items()}
    a_pat, b_pat = (alpha, beta) if raw else (chal_pattern(field, alpha), chal_pattern(field, beta))
    a_val, b_val = chal_value(field, a_pat), chal_value(field, b_pat)
    ref_terms = []
    for name, cols, num, coef, bus in terms:
        tuples = [[value(field, row[c]) for c in cols] for row in pats[name][:n]]
        w = None if num is None else [value(field, row[num[1]]) for row in pats[num[0]][:n]]
        ref_terms.append((tuples, w, coef, bus))
    ref_ranges = [([value(field, pats[name][i][col]) if row0 <= i < row0 + size else None for i in range(n)], lo, size, row0, coef, bus)
                  for name, col, lo, size, row0, coef, bus in ranges]
    want = rref.range_sum(field, ref_terms, ref_ranges, a_val, b_val, n)
    call_terms = [(name, cols, num, elem(field, coef), elem(field, bus)) for name, cols, num, coef, bus in terms]
    call_ranges = [(name, col, lo, size, row0, elem(field, coef), elem(field, bus)) for name, col, lo, size, row0, coef, bus in ranges]
    a_w, b_w = chal_words(field, a_pat), chal_words(field, b_pat)
    expect = host[out[0]].copy()
    expect[:n, out[1]:out[1] + width] = s_words(field, want).reshape((n, width) + expect.shape[2:])

    def spec(bufs):
        return ([(bufs[name], cols, None if num is None else (bufs[num[0]], num[1]), c, b) for name, cols, num, c, b in call_terms],
                [((bufs[name], col), lo, size, row0, c, b) for name, col, lo, size, row0, c, b in call_ranges])
    # the resident form: out's matrix followed by guard words in one allocation, a non-default stream, twice
    dev = {name: to_dev(w) for name, w in host.items() if name != out[0]}
    own = host[out[0]]
    held = torch.full((own.size + 16,), GUARD, dtype=torch.int64, device="cuda")
    fresh = to_dev(own).reshape(-1)
    dev[out[0]] = held[:own.size].view(own.shape)
    stream = side_stream()
    got = []
    for _ in range(2):
        held[:own.size] = fresh
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            pilcheck.range_sum_dev(*spec(dev), a_w, b_w, (dev[out[0]], out[1]), n, field)
        stream.synchronize()
        got.append(held.cpu().numpy().view(np.uint64))
    assert (got[0] == got[1]).all(), "two calls give identical words"
    assert (got[0][own.size:] == np.uint64(GUARD)).all(), "the guard words behind out's matrix"
    bad = np.argwhere(got[0][:own.size].reshape(own.shape) != expect)
    assert bad.size == 0, "the resident form: first differing (row, word ..) %s" % (bad[0],)
    for name, w in host.items():
        if name != out[0]:
            assert (dev[name].cpu().numpy().view(np.uint64) == w).all(), name + " is only read"
    # the promise: logup_sum_dev with each range as a k = 1 term over the materialised columns
    if len(terms) + len(ranges) <= 9:
        tm = to_dev(words(field, materialised(field, ranges, pats, n)))
        lo_out = torch.zeros((n, width) if field == "gl" else (n, 1, 4), dtype=torch.int64, device="cuda")
        as_terms = spec(dev)[0] + [(tm, [2 * r], (tm, 2 * r + 1), c[5], c[6]) for r, c in enumerate(call_ranges)]
        pilcheck.logup_sum_dev(as_terms, a_w, b_w, (lo_out, 0), n, field)
        torch.cuda.synchronize()
        assert (lo_out.cpu().numpy().view(np.uint64).reshape(n, -1) == s_words(field, want)).all(), "logup_sum_dev on the materialised columns"
    # the host form on copies
    if host_form:
        h = {name: w.copy() for name, w in host.items()}
        pilcheck.range_sum(*spec(h), a_w, b_w, (h[out[0]], out[1]), n, field)
        for name, w in host.items():
            assert (h[name] == (expect if name == out[0] else w)).all(), "the host form: " + name
    return want


GL_EDGES = (1, 2, 7, 8, 9, 255, 256, 257, 2047, 2048, 2049, 4097)           # SCAN_ITEMS, a wave, SCAN_CHUNK
FR_EDGES = (1, 2, 63, 64, 65, 1024, 1025, 16385)                            # bnscan's level thresholds


@pytest.mark.parametrize("field,n", [("gl", n) for n in GL_EDGES] + [("bn128", n) for n in FR_EDGES])
def test_row_edges_one_range_no_f(field, n):
    """nF = 0, the range table's own AIR: one range whose window is all rows"""
    rng = random.Random(n)
    q = Q[field]
    m = poison_rows(rng, field, n, 2)
    run(field, {"m": m}, [], [("m", 1, rng.randrange(1 << 20), n, 0, q - 1, rng.randrange(q))], rand_chal(rng, field), rand_chal(rng, field), n, host_form=n <= 2049)


WINDOW_N = {"gl": 4097, "bn128": 1025}
# Goldilocks: the issue's row0 values.  Fr has 1025 rows, so 2047 and 2048 cannot start a window there: 255 / 256 (a workgroup's edge) and
# 1023 / 1024 (the last rows) stand in for them
ROW0 = {"gl": (0, 1, 7, 8, 9, 2047, 2048), "bn128": (0, 1, 7, 8, 9, 255, 256, 1023, 1024)}


@pytest.mark.parametrize("field,row0", [(f, r) for f in FIELDS for r in ROW0[f]])
def test_window_edges(field, row0):
    """the window's end at a lane's first row (the last in-window row is row 8 j), at a lane's last row, mid-lane, at a block boundary and
    at n; and size = 1.  m is poison outside the window: non-zero, one word in three non-canonical"""
    rng = random.Random(row0)
    n, q = WINDOW_N[field], Q[field]
    block = 2048 if field == "gl" else 256
    m = poison_rows(rng, field, n, 3)
    f = rand_rows(rng, field, n, 2)
    lane = (row0 // 8 + 2) * 8                        # the start of the second lane behind row0's
    ends = {row0 + 1, lane + 1, lane + 8, lane + 5, (row0 // block + 1) * block, n}
    alpha, beta = rand_chal(rng, field), rand_chal(rng, field)
    for i, end in enumerate(sorted(e for e in ends if row0 < e <= n)):
        terms = [("f", [0], None, 1, 5)] if i % 2 else []
        run(field, {"m": m, "f": f}, terms, [("m", 1, -3, end - row0, row0, q - 1, 5)], alpha, beta, n, host_form=i < 2)


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("lo,size", [(0, 300), (-3, 8), (I64_MIN, 300), (I64_MAX - 300 + 1, 300), ((1 << 32) - 2, 300)])
def test_lo_values(field, lo, size):
    """lo = 0, a range that crosses zero, the two ends of int64 and one that crosses 2^32"""
    rng = random.Random(size + (lo & 0xFFFF))
    n, q = 313, Q[field]
    m = poison_rows(rng, field, n, 2)
    run(field, {"m": m}, [], [("m", 0, lo, size, 5, q - 1, 77)], rand_chal(rng, field), rand_chal(rng, field), n)


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("n_f,n_r", [(0, 1), (0, 8), (1, 1), (8, 1), (4, 5), (1, 8)])
def test_shapes(field, n_f, n_r):
    """f terms of k = 1, 3, 16 with and without numerators; the ranges in pairs on one m matrix, each with a bus id, a window and a lo of its own"""
    rng = random.Random(10 * n_f + n_r)
    n, q = 300, Q[field]
    mats = {"a": rand_rows(rng, field, n, 19)}
    terms = []
    for u in range(n_f):
        k = (1, 3, 16)[u % 3]
        terms.append(("a", [rng.randrange(16) for _ in range(k)], ("a", 16 + u % 3) if u % 2 == 0 else None, rng.choice((1, q - 1, 5)), rng.randrange(q)))
    ranges = []
    for r in range(n_r):
        name = "m%d" % (r // 2)                       # two ranges share one m matrix
        mats.setdefault(name, poison_rows(rng, field, n, 3))
        row0 = rng.randrange(0, 40)
        ranges.append((name, r % 2, rng.randrange(-1000, 1000), rng.randrange(1, n - row0 + 1), row0, rng.choice((q - 1, 1, 5)), 1000 + r))
    run(field, mats, terms, ranges, rand_chal(rng, field), rand_chal(rng, field), n)


@pytest.mark.parametrize("field", FIELDS)
def test_overlapping_windows(field):
    rng = random.Random(43)
    n, q = 300, Q[field]
    m = poison_rows(rng, field, n, 2)
    ranges = [("m", 0, 0, 200, 3, q - 1, 1), ("m", 1, 100, 150, 130, q - 1, 2)]
    run(field, {"m": m, "f": rand_rows(rng, field, n, 1)}, [("f", [0], None, 1, 1)], ranges, rand_chal(rng, field), rand_chal(rng, field), n)


@pytest.mark.parametrize("field", FIELDS)
def test_non_canonical_m_coefficients_and_challenges(field):
    """m holds words at or above the modulus (poison_rows) inside the window too; coef -1, 1 and 5; alpha and beta given as words at or above
    the modulus (over Fr any 256-bit pattern)"""
    rng = random.Random(47)
    n, q, top = 263, Q[field], TOP[field]
    m = poison_rows(rng, field, n, 2)
    for i in range(0, n, 5):
        m[i][0] = rng.choice((q, top - 1, q + rng.randrange(top - q)))
    f = poison_rows(rng, field, n, 2)
    for coef in (q - 1, 1, 5):
        run(field, {"m": m, "f": f}, [("f", [0], ("f", 1), 1, 9)], [("m", 0, -7, 250, 9, coef, 9)], rand_chal(rng, field), rand_chal(rng, field), n)
    if field == "gl":
        raws = [((P, (1 << 64) - 1, P + 5), ((1 << 64) - 1, P + 1, P)), ((0, 1, 0), (P, P, P))]     # P + 5 = 5, 2^64 - 1 = 2^32 - 2; beta = 0
    else:
        raws = [((1 << 256) - 1, R + 12345), (R, (1 << 256) - 1 - rng.randrange(1 << 100))]
    for a, b in raws:
        run(field, {"m": m, "f": f}, [("f", [0], ("f", 1), 1, 9)], [("m", 0, -7, 250, 9, q - 1, 9)], a, b, n, raw=True)


@pytest.mark.parametrize("field", FIELDS)
def test_zero_denominators(field):
    """beta chosen from the checker so that E vanishes at a lane's first in-window row (the window's first row, mid-lane, and the first row
    of the next lane), at a middle row, at the last in-window row; the rows behind a zero still get E + alpha.  Then an f term and the range
    both zero at one row: the row adds only what the second range gives"""
    rng = random.Random(53)
    n, q, F = 300, Q[field], lref.FIELDS[field]
    m = [[v if value(field, v) else 3 for v in row] for row in poison_rows(rng, field, n, 2)]       # no multiplicity is zero: a zero step is a zero E
    f = rand_rows(rng, field, n, 1)
    alpha = rand_chal(rng, field)
    lo, size, row0, bus = -20, 101, 19, 7            # rows 19 .. 119: the window starts at row 3 of a lane and ends at row 7 of one
    spec = (None, lo, size, row0, q - 1, bus)
    step = lambda s, i: F.add(s[i], neg(field, s[i - 1] if i else F.zero))        # noqa: E731
    for hit in (19, 24, 20, 77, 119):
        beta = zero_beta(field, spec, alpha, hit)
        s = run(field, {"m": m}, [], [("m", 0, lo, size, row0, q - 1, bus)], alpha, beta, n)
        assert step(s, hit) == F.zero and step(s, hit - 1 if hit > row0 else hit + 1) != F.zero
        if hit < 119:
            assert step(s, hit + 1) != F.zero, "the chain goes on behind a zero"
    hit = 64
    f[hit][0] = pattern_of(field, lo + hit - row0)    # the f term's tuple is the range's value at that row, with the same bus id
    beta = zero_beta(field, spec, alpha, hit)
    ranges = [("m", 0, lo, size, row0, q - 1, bus), ("m", 1, 5, 200, 10, 5, bus + 1)]
    s = run(field, {"m": m, "f": f}, [("f", [0], None, 1, bus)], ranges, alpha, beta, n)
    only = rref.row_fraction(F, [], [([value(field, r[1]) for r in m], 5, 200, 10, 5, bus + 1)], F.ext(alpha), F.ext(beta), hit)[2]
    assert step(s, hit) == only != F.zero
    s = run(field, {"m": m, "f": f}, [("f", [0], None, 1, bus)], ranges[:1], alpha, beta, n)
    assert step(s, hit) == F.zero and step(s, hit + 1) != F.zero, "every term of the row is zero: the row adds 0"


@pytest.mark.parametrize("field", FIELDS)
def test_out_as_spare_columns_of_m(field):
    rng = random.Random(59)
    n, q = 300, Q[field]
    width = 3 if field == "gl" else 1
    m = poison_rows(rng, field, n, 2 + width + 1)     # m0, m1, then s, then one more column that must survive
    run(field, {"m": m, "f": rand_rows(rng, field, n, 1)}, [("f", [0], None, 1, 2)], [("m", 0, 0, 256, 0, q - 1, 2), ("m", 1, -5, 100, 200, q - 1, 3)],
        rand_chal(rng, field), rand_chal(rng, field), n, out=("m", 2))


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("size", [256, 10000])
def test_closing_through_range_logup(field, size):
    """range_mult_dev (256: its LDS path, 10000: its global path) then range_sum_dev: with every f in range the report is clean and
    s[n-1] = 0; with one value out of range the report names it and s[n-1] != 0"""
    rng = random.Random(size)
    n, q, lo = 10007, Q[field], -100
    width = 3 if field == "gl" else 1
    alpha, beta = rand_chal(rng, field), rand_chal(rng, field)
    vals = [[lo + rng.randrange(size), lo + rng.randrange(size)] for _ in range(n)]
    for alter in (False, True):
        rows = [[pattern_of(field, v) for v in r] + [0] * (1 + width) for r in vals]      # f0 f1 m s..
        if alter:
            rows[4321][1] = pattern_of(field, lo + size)
        cm = to_dev(words(field, rows))
        rep, last = pilcheck.range_logup([(cm, [0]), (cm, [1])], lo, size, (cm, 2), chal_words(field, chal_pattern(field, alpha)),
                                         chal_words(field, chal_pattern(field, beta)), (cm, 3), n, field, row0=3)
        torch.cuda.synchronize()
        got = cm.cpu().numpy().view(np.uint64)
        assert (got[n - 1, 3:3 + width].reshape(-1) == last).all()
        if alter:
            assert rep == (1, 1, 4321, 2 * n - 1) and last.any(), "the report names the value out of range and the sum stays open"
        else:
            assert rep == (0, pilcheck.NONE, pilcheck.NONE, 2 * n) and not last.any(), "the sum closes"


@pytest.mark.parametrize("field,n", [("gl", 2048 * 256 + 1), ("bn128", 262145)])
def test_deep_scans_periodic_inputs(field, n):
    """257 block totals (a lane of the second pass walks two) / five levels.  The checker takes a periodic f term and three ranges with
    short windows (the start, the middle across a block edge, the last rows); a range over ALL rows, whose denominators no period shortens,
    is compared with logup_sum_dev on the materialised columns.  The resident form only."""
    rng = random.Random(61)
    q, per = Q[field], 64
    width = 3 if field == "gl" else 1
    base = poison_rows(rng, field, per, 3)
    mat = words(field, base)
    dev = to_dev(np.concatenate([mat] * (n // per + 1))[:n])
    shape = (n, width) if field == "gl" else (n, 1, 4)
    out = torch.zeros(shape, dtype=torch.int64, device="cuda")
    alpha, beta = rand_chal(rng, field), rand_chal(rng, field)
    a_w, b_w = chal_words(field, chal_pattern(field, alpha)), chal_words(field, chal_pattern(field, beta))
    mid = (n // 2) // 2048 * 2048 - 37
    windows = [(1, 0, -5, 90, 0, q - 1, 11), (1, 0, I64_MAX - 99, 100, mid, 5, 12), (2, 0, 1 << 40, 70, n - 70, q - 1, 13)]
    f_term = [(dev, [0], (dev, 2), elem(field, 1), elem(field, 3))]
    pilcheck.range_sum_dev(f_term, [((dev, c), lo, size, row0, elem(field, co), elem(field, b)) for c, _, lo, size, row0, co, b in windows], a_w, b_w, (out, 0), n, field)
    torch.cuda.synchronize()
    vals = [[value(field, v) for v in row] for row in patterns(mat)]
    ref_ranges = [((lambda i, c=c: vals[i % per][c]), lo, size, row0, co, b) for c, _, lo, size, row0, co, b in windows]
    want = rref.range_sum(field, [([r[:1] for r in vals], [r[2] for r in vals], 1, 3)], ref_ranges, alpha, beta, n, period=per)
    assert (out.cpu().numpy().view(np.uint64).reshape(n, -1) == s_words(field, want)).all()
    # one range over all rows against logup_sum_dev on its materialised t column
    lo = (1 << 32) - 1000
    if field == "gl":
        t = ((np.arange(n, dtype=np.uint64) + np.uint64(lo)) % np.uint64(P)).reshape(n, 1)
    else:
        t = cref.fr_words([pattern_of(field, lo + i) for i in range(n)]).reshape(n, 1, 4)
    tm = to_dev(t)
    other = torch.zeros(shape, dtype=torch.int64, device="cuda")
    pilcheck.range_sum_dev(f_term, [((dev, 1), lo, n, 0, elem(field, q - 1), elem(field, 9))], a_w, b_w, (out, 0), n, field)
    pilcheck.logup_sum_dev(f_term + [(tm, [0], (dev, 1), elem(field, q - 1), elem(field, 9))], a_w, b_w, (other, 0), n, field)
    torch.cuda.synchronize()
    assert torch.equal(out, other) and bool(out[n - 1].any())


@pytest.mark.parametrize("field", FIELDS)
def test_resident_call_only_enqueues(field):
    """the call returns before its work is done: after one warm-up (the working slots grow with a device synchronise on first use), four
    calls of one f term and eight ranges over 2^22 (Goldilocks) / 2^20 (Fr) rows -- milliseconds of device work each -- are sent on a side
    stream and an event recorded behind them has not completed when the last call returns; nothing is compared here but that and the two
    runs' words"""
    n = 1 << (22 if field == "gl" else 20)
    g = torch.Generator(device="cuda").manual_seed(41)
    mat = torch.randint(0, 1 << 62, (n, 4) if field == "gl" else (n, 4, 4), dtype=torch.int64, device="cuda", generator=g)     # below both moduli
    out = torch.zeros((n, 3) if field == "gl" else (n, 1, 4), dtype=torch.int64, device="cuda")
    terms = [(mat, [0, 1, 2], (mat, 3), elem(field, 1), elem(field, 9))]
    ranges = [((mat, r % 4), -r, n - r, r, elem(field, 1 + r), elem(field, 9 + r)) for r in range(8)]
    a, b = (chal_words(field, chal_pattern(field, rand_chal(random.Random(s), field))) for s in (1, 2))
    stream = side_stream()
    with torch.cuda.stream(stream):
        pilcheck.range_sum_dev(terms, ranges, a, b, (out, 0), n, field)
    stream.synchronize()
    first = out.clone()
    torch.cuda.synchronize()
    done = torch.cuda.Event()
    with torch.cuda.stream(stream):
        for _ in range(4):
            pilcheck.range_sum_dev(terms, ranges, a, b, (out, 0), n, field)
        done.record(stream)
        pending = not done.query()
    stream.synchronize()
    assert pending, "range_sum_dev waited for the device"
    assert done.query() and torch.equal(out, first)
