"""The multiplicity sessions on the device (csrc/mult_session.hip) against the checker over Python integers (tests/mult_session_ref.py)
and against the one-shot entries: every element of m, every word of every add's report and the session's total; both fields, both table
kinds, both count paths of a range session forced.  Elements are bit patterns: Goldilocks words at or above p and non-canonical Fr
patterns are among them everywhere (bump).  The shapes are the smallest at which each piece can go wrong: one row, the wave and workgroup
edges, sides longer and shorter than the table, several adds."""
import numpy as np
import pytest

import conn_pols_ref as ref
import mult_session_ref as sref
import range_mult_ref as rref
from conn_pols_ref import P, R

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from pil2gl import pilcheck  # noqa: E402

FIELDS = {"gl": P, "bn128": R}
NONE = sref.NONE
PATHS = (0, 1)
SEED = (1 << 32) - 2


def words(field, rows):
    """rows of integer bit patterns -> the library's matrix: (n, stride) uint64, or (n, stride, 4)"""
    if field == "gl":
        return np.array(rows, np.uint64).reshape(len(rows), -1)
    return ref.fr_words([v for row in rows for v in row]).reshape(len(rows), -1, 4)


def to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


def pat(field, v, bump=False):
    """the integer v as a pattern; bump: the same value as a word >= p, or a non-canonical Fr pattern"""
    q = FIELDS[field]
    return rref.pattern(v, q) + (q if bump and rref.pattern(v, q) + q < (1 << (64 if field == "gl" else 256)) else 0)


def matrix(field, rng, n, stride, top):
    """n rows of `stride` random values below top, every third one bumped"""
    return [[pat(field, int(v), (i + j) % 3 == 0) for j, v in enumerate(row)] for i, row in enumerate(rng.integers(0, top, (max(n, 1), stride)))][:n]


def tuple_rows(field, rng, n, k, top, spare=0):
    """n rows whose tuple is (v, v + 1, .., v + k - 1) for a random v below top, then `spare` columns of zeroes"""
    return [[pat(field, int(v) + j, (i + j) % 3 == 0) for j in range(k)] + [0] * spare for i, v in enumerate(rng.integers(0, top, max(n, 1)))][:n]


def selector(field, rng, n):
    """0, p | r (zero as a value) and non-zero patterns"""
    q = FIELDS[field]
    return [[(0, q, 1, pat(field, 7, True))[int(v)]] for v in rng.integers(0, 4, max(n, 1))][:n]


def poisoned(field, n, stride):
    return to_dev(words(field, [[(1 << 63) + 5 * i + j for j in range(stride)] for i in range(n)]))


def column(field, dev, col, n):
    """column col of a device matrix as n integer patterns"""
    a = dev.cpu().numpy().view(np.uint64)
    if field == "gl":
        return [int(v) for v in a[:n, col]]
    return [sum(int(w) << (64 * i) for i, w in enumerate(e)) for e in a[:n, col]]


def elements(field, counts):
    return [sref.element(c, FIELDS[field]) for c in counts]


def col_of(rows, c):
    return [row[c] for row in rows]


class Lookup:
    """one lookup session on the device beside the checker's; t: rows of k + 1 patterns, the last column spare"""

    def __init__(self, field, t, k, sel_t=None, seed=None):
        self.field, self.k, self.n = field, k, len(t)
        self.dt = to_dev(words(field, t))
        self.ds = None if sel_t is None else to_dev(words(field, sel_t))
        self.dev = pilcheck.LookupSession((self.dt, list(range(k)), None if sel_t is None else (self.ds, 0)), self.n, field, seed)
        self.ref = sref.LookupSession([row[:k] for row in t], FIELDS[field], None if sel_t is None else col_of(sel_t, 0), seed or 0)

    def add(self, fs, sels=None):
        """fs: host row lists of k columns; the device's report against the checker's -> the report"""
        sels = sels or [None] * len(fs)
        sides = [(words(self.field, f) if f else np.zeros((1, self.k) + ((4,) if self.field == "bn128" else ()), np.uint64), list(range(self.k)),
                  None if s is None else (words(self.field, s), 0)) for f, s in zip(fs, sels)]
        got = self.dev.add(sides, [len(f) for f in fs])
        want = self.ref.add(fs, [None if s is None else col_of(s, 0) for s in sels])
        assert got == want, (got, want)
        return got

    def check(self, into=None, col=0):
        """write, m against the checker, the total -> m as patterns"""
        into = poisoned(self.field, self.n, 2) if into is None else into
        total = self.dev.write((into, col))
        got = column(self.field, into, col, self.n)
        assert got == elements(self.field, self.ref.m()), "m differs from the checker"
        assert total == self.ref.total
        return got


class Range:
    """one range session on the device beside the checker's"""

    def __init__(self, field, lo, size, path=None, seed=None):
        self.field, self.size = field, size
        self.dev = pilcheck.RangeSession(lo, size, field, path, seed)
        self.ref = sref.RangeSession(lo, size, FIELDS[field], seed or 0)

    def add(self, fs, sels=None):
        sels = sels or [None] * len(fs)
        sides = [(words(self.field, f) if f else np.zeros((1, 1) + ((4,) if self.field == "bn128" else ()), np.uint64), [0],
                  None if s is None else (words(self.field, s), 0)) for f, s in zip(fs, sels)]
        got = self.dev.add(sides, [len(f) for f in fs])
        want = self.ref.add([col_of(f, 0) for f in fs], [None if s is None else col_of(s, 0) for s in sels])
        assert got == want, (got, want)
        return got

    def check(self, n_m, row0=0, into=None, col=0):
        into = poisoned(self.field, n_m, 2) if into is None else into
        total = self.dev.write((into, col), n_m, row0)
        got = column(self.field, into, col, n_m)
        assert got == elements(self.field, self.ref.m(n_m, row0)), "m differs from the checker"
        assert total == self.ref.total
        return got


# ---- equivalence 1: one add of equal lengths is the one-shot call, word for word ----
@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("k", (1, 3, 16))
def test_lookup_session_of_one_add_is_lookup_mult(field, k):
    rng = np.random.default_rng(100 + k)
    for n in (1, 5, 64, 1000):
        top = max(2, n // 2)
        t, sel_t = tuple_rows(field, rng, n, k, top, 1), selector(field, rng, n)
        fs, sels = [tuple_rows(field, rng, n, k, top + (n > 5)) for _ in range(3)], [None, selector(field, rng, n), selector(field, rng, n)]
        s = Lookup(field, t, k, sel_t)
        rep = s.add(fs, sels)
        m = s.check()
        dt, ds = to_dev(words(field, t)), to_dev(words(field, sel_t))
        one = pilcheck.lookup_mult_dev([(to_dev(words(field, f)), list(range(k)), None if x is None else (to_dev(words(field, x)), 0)) for f, x in zip(fs, sels)],
                                       (dt, list(range(k)), (ds, 0)), (dt, k), n, field)
        assert rep == one and m == column(field, dt, k, n), (n, rep, one)


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("path", PATHS)
def test_range_session_of_one_add_is_range_mult(field, path):
    rng = np.random.default_rng(200 + path)
    for n in (1, 5, 64, 1000):
        size, lo = max(1, n // 2), -3
        row0 = n - size if n > 5 else 0
        fs = [[[pat(field, lo + int(v), i % 3 == 0)] for i, v in enumerate(rng.integers(-1 if n > 5 else 0, size + (n > 5), n))] for _ in range(3)]
        sels = [None, selector(field, rng, n), None]
        s = Range(field, lo, size, path)
        rep = s.add(fs, sels)
        m = s.check(n, row0)
        dm = poisoned(field, n, 2)
        one = pilcheck.range_mult_dev([(to_dev(words(field, f)), [0], None if x is None else (to_dev(words(field, x)), 0)) for f, x in zip(fs, sels)],
                                      lo, size, (dm, 1), n, field, row0, path)
        assert rep == one and m == column(field, dm, 1, n), (n, rep, one)


# ---- own lengths: eight sides of their own row counts in one add ----
def lengths(n_t):
    return [0, 1, 63, 64, 65, 257, 3 * n_t + 1, 1000]


@pytest.mark.parametrize("field", FIELDS)
def test_lookup_sides_of_their_own_lengths(field):
    rng = np.random.default_rng(300)
    for n_t in (5, 100):
        s = Lookup(field, matrix(field, rng, n_t, 3, 4), 2, selector(field, rng, n_t))
        rows = lengths(n_t)
        rep = s.add([matrix(field, rng, n, 2, 4) for n in rows], [selector(field, rng, n) if i % 2 else None for i, n in enumerate(rows)])
        assert rep[3] > 0
        s.check()


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("path", PATHS)
def test_range_sides_of_their_own_lengths(field, path):
    rng = np.random.default_rng(310 + path)
    for size in (5, 100):
        s = Range(field, 10, size, path)
        rows = lengths(size)
        side = lambda n: [[pat(field, 10 + int(v), i % 3 == 1)] for i, v in enumerate(rng.integers(0, size, max(n, 1)))][:n]      # noqa: E731
        rep = s.add([side(n) for n in rows], [selector(field, rng, n) if i % 2 else None for i, n in enumerate(rows)])
        assert rep[0] == 0 and rep[3] > 0
        s.check(size + 7, 4)


# ---- the grid of a count launch comes from ITS side's rows, never from the table ----
@pytest.mark.parametrize("field", FIELDS)
def test_an_adds_grids_come_from_its_sides_rows(field):
    rng = np.random.default_rng(350)
    side = lambda n, k=1: tuple_rows(field, rng, n, k, 5)                        # noqa: E731
    big = Lookup(field, tuple_rows(field, rng, 1000, 1, 500, 1), 1)             # the table's own launches take 4 workgroups
    big.add([side(100), [], side(257), side(1025)])
    assert pilcheck.mult_session_grids() == [1, 0, 2, 5, 0, 0, 0, 0], "small sides against a larger table: not the table's grid"
    small = Lookup(field, tuple_rows(field, rng, 5, 1, 5, 1), 1)                # one workgroup for the table
    small.add([side(2049)])
    assert pilcheck.mult_session_grids() == [9, 0, 0, 0, 0, 0, 0, 0], "a long side against a table of 5 rows is not starved; the last add only"
    for path, want in ((0, [1, 2, 3]), (1, [1, 5, 9])):
        r = Range(field, 0, 5, path)
        r.add([side(100), side(1025), side(2049)])
        assert pilcheck.mult_session_grids() == want + [0] * 5, path
    r = Range(field, 0, 9000)                         # the global path; 9000 rows would be 36 workgroups
    r.add([side(100)])
    assert pilcheck.mult_session_grids()[0] == 1
    for s in (big, small):
        s.check()


# ---- equivalence 2: m depends on the rows offered, not on how they were cut ----
def cuts(n):
    return [(0, 1), (1, 64), (64, n - 1), (n - 1, n)]


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("kind", ("lookup", "range0", "range1"))
def test_partition_invariance(field, kind):
    rng = np.random.default_rng(400)
    rows = (130, 257, 66)
    if kind == "lookup":
        t, sel_t = matrix(field, rng, 50, 3, 5), selector(field, rng, 50)
        fs = [matrix(field, rng, n, 2, 6) for n in rows]
        make = lambda: Lookup(field, t, 2, sel_t)                              # noqa: E731
        check = lambda s: s.check()                                            # noqa: E731
    else:
        fs = [[[pat(field, int(v), i % 3 == 0)] for i, v in enumerate(rng.integers(-1, 42, n))] for n in rows]
        make = lambda: Range(field, 0, 40, int(kind[-1]))                      # noqa: E731
        check = lambda s: s.check(64, 20)                                      # noqa: E731
    sels = [selector(field, rng, n) for n in rows]
    whole = make()
    whole.add(fs, sels)
    per_side = make()
    reps = [per_side.add([f], [x]) for f, x in zip(fs, sels)]
    assert sum(r[3] for r in reps) == per_side.ref.total
    cut = make()                                      # each side cut at rows 1, 64 and n - 1 by advancing the base of ONE device matrix
    matched = 0
    width = len(fs[0][0])
    for f, x in zip(fs, sels):
        df, dx = to_dev(words(field, [row + [0] * (2 - width % 2) for row in f])), to_dev(words(field, [row + [0] for row in x]))   # even strides: 16-byte rows
        got = cut.dev.add([(df[a:b], list(range(width)), (dx[a:b], 0)) for a, b in cuts(len(f))], [b - a for a, b in cuts(len(f))])
        want = cut.ref.add([f[a:b] if kind == "lookup" else col_of(f[a:b], 0) for a, b in cuts(len(f))], [col_of(x[a:b], 0) for a, b in cuts(len(f))])
        assert got == want
        matched += got[3]
    m = check(whole)
    assert check(per_side) == m and check(cut) == m and matched == cut.ref.total == whole.ref.total


# ---- an add's report is its own ----
@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("kind", ("lookup", "range0", "range1"))
def test_failing_add_in_the_middle_of_three(field, kind):
    v = lambda *vals: [[pat(field, x)] for x in vals]                          # noqa: E731
    if kind == "lookup":
        s = Lookup(field, [[pat(field, x), 0] for x in (3, 4, 5, 4)], 1)
        check = lambda: s.check()                                              # noqa: E731
    else:
        s = Range(field, 3, 3, int(kind[-1]))
        check = lambda: s.check(4)                                             # noqa: E731
    assert s.add([v(3, 4), v(5)]) == (0, NONE, NONE, 3)
    assert s.add([v(3, 4, 5), v(4, 9, 5, 2), v(7)]) == (1, 1, 1, 5), "the smallest failing (side, row) of this add; the matched rows still count"
    assert s.add([v(4)]) == (0, NONE, NONE, 1), "the next add reports clean"
    assert check()[:3] == elements(field, [2, 4, 3]) and s.ref.total == 9


# ---- write does not end the session ----
@pytest.mark.parametrize("field", FIELDS)
def test_write_twice_and_into_a_spare_column_of_t(field):
    rng = np.random.default_rng(500)
    n = 70
    t = matrix(field, rng, n, 3, 6)                   # columns 0, 1 the tuple, column 2 spare
    s = Lookup(field, t, 2)
    out = poisoned(field, n, 4)
    s.add([matrix(field, rng, 100, 2, 6)])
    first = s.check(out, 1)
    s.check(s.dt, 2)                                  # m as a spare column of t's matrix; the session goes on
    s.add([matrix(field, rng, 33, 2, 6), matrix(field, rng, 1, 2, 6)])
    later = s.check(out, 3)
    assert column(field, out, 1, n) == first != later, "the snapshot stays, the later state differs"
    assert s.check(s.dt, 2) == later and col_of(t, 0) == column(field, s.dt, 0, n) and col_of(t, 1) == column(field, s.dt, 1, n)
    r = Range(field, -2, 9, None)
    r.add([[[pat(field, int(x))] for x in rng.integers(-2, 7, 80)]])
    first = r.check(12, 1, out, 0)
    r.add([[[pat(field, 0)]] * 3])
    assert r.check(12, 3, out, 2) != first == column(field, out, 0, 12)


# ---- counters are 64 bits wide ----
@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("kind", ("lookup", "range0", "range1"))
def test_carry_past_32_bits(field, kind):
    q = FIELDS[field]
    v = lambda *vals: [[pat(field, x)] for x in vals]                          # noqa: E731
    if kind == "lookup":
        make = lambda: Lookup(field, [[pat(field, x), 0] for x in (3, 4, 5)], 1, seed=SEED)      # noqa: E731
        check = lambda s: s.check()                                            # noqa: E731
    else:
        make = lambda: Range(field, 3, 3, int(kind[-1]), seed=SEED)            # noqa: E731
        check = lambda s: s.check(3)                                           # noqa: E731
    s = make()
    assert s.add([v(4, 4, 3, 4, 4, 4)]) == (0, NONE, NONE, 6)
    want = [(1 << 32) - 1, (1 << 32) + 3, (1 << 32) - 2]
    assert check(s) == [c if q == P else c * ref.MONT % R for c in want], "2^32 + 3 and 2^32 - 1 as field elements (Montgomery over Fr)"
    s = make()                                        # 64 lanes of one wave on one counter: the merged add
    assert s.add([v(*[5] * 64)]) == (0, NONE, NONE, 64)
    assert check(s) == elements(field, [SEED, SEED, SEED + 64])


# ---- the window of a range write ----
@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("path", PATHS)
def test_range_windows(field, path):
    for lo, size, n_m in ((-5, 7, 20), (-1, 1, 3), (0, 1, 2), (-(1 << 40), 3, 9)):
        s = Range(field, lo, size, path)
        vals = [lo + size - 1, lo, lo - 1, lo, lo + size, lo + size // 2]
        assert s.add([[[pat(field, x, i % 2 == 0)] for i, x in enumerate(vals)]]) == (1, 0, 2, 4), "lo - 1 and lo + size fail"
        for row0 in (0, 1, n_m - size):
            s.check(n_m, row0)


# ---- one table AIR, two user AIRs: the bus closes ----
def field_sum(field, elems):
    """the sum of s's last elements: three words each mod p, or Montgomery words mod r"""
    if field == "gl":
        return [sum(int(e[i]) for e in elems) % P for i in range(3)]
    return [sum(sum(int(w) << (64 * i) for i, w in enumerate(e)) for e in elems) % R]


@pytest.mark.parametrize("field", FIELDS)
def test_range_logup_cross_closes_the_bus(field):
    rng = np.random.default_rng(600)
    q, lo, size, row0, n_table = FIELDS[field], -7, 200, 3, 1 << 8
    users = []
    for n in (1 << 6, 1 << 9):
        vals = [[pat(field, lo + int(v), i % 5 == 0), 1 if i % 4 else 0] for i, v in enumerate(rng.integers(0, size, n))]
        d = to_dev(words(field, [[a, rref.pattern(b, q)] for a, b in vals]))
        users.append(([(d, [0]), (d, [0], (d, 1))], n))        # the column twice: once every row, once under a 0 / 1 selector
    wide = 3 if field == "gl" else 1
    challenge = lambda: np.array([int(x) for x in rng.integers(1, 1 << 62, 3)], np.uint64) if field == "gl" else ref.fr_words([int(rng.integers(1, 1 << 62))]).reshape(-1)   # noqa: E731
    alpha, beta = challenge(), challenge()
    table = poisoned(field, n_table, 1 + wide)
    outs = [(poisoned(field, n, wide), 0) for _, n in users]
    reports, total, last = pilcheck.range_logup_cross(users, lo, size, (table, 0), n_table, alpha, beta, outs, (table, 1), field, row0)
    assert all(r[0] == 0 for r in reports) and total == sum(r[3] for r in reports) == sum(n + sum(1 for i in range(n) if i % 4) for _, n in users)
    assert not any(field_sum(field, last)), "the three last elements sum to zero"
    m = column(field, table, 0, n_table)
    assert m[:row0] == [0] * row0 and sum(1 for c in m if c) > 100 and m[row0 + size:] == [0] * (n_table - row0 - size)
    # one count altered on the host: the bus stays open
    host = table.cpu().numpy().view(np.uint64).copy()
    host[row0 + 5, 0] = words(field, [[sref.element(1003, q)]])[0, 0]
    bad = to_dev(host)
    terms, rng_term = pilcheck._range_logup_terms([], lo, size, (bad, 0), row0, None, 1 if field == "gl" else 4)
    pilcheck.range_sum_dev([], [rng_term], alpha, beta, (bad, 1), n_table, field)
    assert any(field_sum(field, last[:2] + [pilcheck._last_element((bad, 1), n_table, 1 if field == "gl" else 4)]))
