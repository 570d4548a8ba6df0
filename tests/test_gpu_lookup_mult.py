"""The lookup multiplicities on the device (csrc/lookup_mult.hip) against the dictionary checker (tests/lookup_mult_ref.py): every element of
m and all four words of the report, both fields, the resident and the host forms.  Every case goes through run(): the resident form with
the caller's working buffer followed by guard words, the host form on copies, and the checker on the same words; the guard words, every
input matrix and every column of m's matrix other than m must come back unchanged.  Elements are given as bit patterns: the checker and
the device both count them mod the modulus (over Fr two Montgomery patterns are equal mod r exactly when their values are).
The shapes are the smallest at which the kernels can still go wrong: the wave and workgroup edges, k = 1, 3 and 16, 1, 2 and 8 sides,
2^15 rows on one counter, three tuples that share a home slot."""
import ctypes as C

import numpy as np
import pytest

import lookup_mult_ref as mref
import conn_pols_ref as ref
from conn_pols_ref import P, R, MONT

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from pil2gl import _lib, pilcheck  # noqa: E402
import pil2gl  # noqa: E402

FIELDS = {"gl": P, "bn128": R}
NONE = mref.NONE
GUARD = 0x6B6B6B6B6B6B6B6B
POISON = {"gl": 0xDEADBEEFDEADBEEF, "bn128": (1 << 256) - 0x1234567}


def words(field, rows):
    """rows of integer bit patterns -> the library's matrix: (n, stride) uint64, or (n, stride, 4)"""
    if field == "gl":
        return np.array(rows, np.uint64).reshape(len(rows), -1)
    return ref.fr_words([v for row in rows for v in row]).reshape(len(rows), -1, 4)


def patterns(w):
    """the library's words back as rows of integers"""
    if w.ndim == 2:
        return [[int(v) for v in row] for row in w]
    return [[sum(int(e[k]) << (64 * k) for k in range(4)) for e in row] for row in w]


def to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


def run(field, mats, fs, t, m, n, order=None):
    """mats: name -> rows of bit patterns (a matrix); fs, t: sides (name, cols) or (name, cols, (selector's name, col)); m: (name, col), a
    name that mats lacks being a matrix of its own, 3 wide and poisoned; order: the f sides as the call gets them (a permutation)
    -> (m as counts, the report), which the resident form, the host form and the checker all give"""
    q, ew = FIELDS[field], 1 if field == "gl" else 4
    mats = dict(mats)
    if m[0] not in mats:
        mats[m[0]] = [[POISON[field] - i - j for j in range(3)] for i in range(n)]
    host = {name: words(field, rows) for name, rows in mats.items()}
    pats = {name: patterns(w) for name, w in host.items()}
    col = lambda s: None if len(s) < 3 or s[2] is None else [row[s[2][1]] for row in pats[s[2][0]]]      # noqa: E731
    tup = lambda s: [[row[c] for c in s[1]] for row in pats[s[0]]]                                       # noqa: E731
    fs = [fs[i] for i in order] if order else list(fs)
    want_m, want = mref.multiplicities([tup(s) for s in fs], tup(t), q, [col(s) for s in fs], col(t))
    k = len(t[1])
    lib = _lib.load()
    need = pilcheck.lookup_mult_plan(n, k, len(fs), field)["scratchBytes"]
    work = torch.full((need // 8 + 8,), GUARD, dtype=torch.int64, device="cuda")
    dev = {name: to_dev(w) for name, w in host.items()}
    keep = []

    def struct(s, ptr_of):
        cols = np.array(s[1], np.uint64)
        keep.append(cols)
        sel = s[2] if len(s) > 2 and s[2] is not None else None
        return _lib.TupleSide(ptr_of(s[0]), host[s[0]].shape[1], cols.ctypes.data, None if sel is None else ptr_of(sel[0]),
                              0 if sel is None else host[sel[0]].shape[1], 0 if sel is None else sel[1])
    dptr = lambda name: dev[name].data_ptr()                                     # noqa: E731
    F = (_lib.TupleSide * len(fs))(*[struct(s, dptr) for s in fs])
    T = struct(t, dptr)
    rep = (C.c_uint64 * 4)()
    fn = lib.pil2gl_lookup_mult_dev if ew == 1 else lib.pil2gl_bn128_lookup_mult_dev
    rc = fn(F, len(fs), C.byref(T), dptr(m[0]), host[m[0]].shape[1], m[1], n, k, work.data_ptr(), need, rep, None)
    assert rc == 0, lib.pil2gl_last_error()
    got = tuple(int(x) for x in rep)
    assert (work[need // 8:].cpu().numpy().view(np.uint64) == GUARD).all(), "a write past scratchBytes"
    expect = {name: w.copy() for name, w in host.items()}
    expect[m[0]][:n, m[1]] = words(field, [[mref.element(c, q)] for c in want_m])[:, 0]
    for name, w in expect.items():
        back = dev[name].cpu().numpy().view(np.uint64).reshape(w.shape)
        assert (back == w).all(), "matrix %s: an input changed, or m differs from the checker at rows %s" % (
            name, np.argwhere((back != w).reshape(len(w), -1).any(1)).ravel()[:8])
    assert got == want, (got, want)
    assert sum(want_m) == got[3], "the sum of m is `matched`"
    # the host form, on copies; one array a name, so that what shares a matrix above shares one here
    hc = {name: w.copy() for name, w in host.items()}
    side = lambda s: (hc[s[0]], s[1], None if len(s) < 3 or s[2] is None else (hc[s[2][0]], s[2][1]))      # noqa: E731
    assert pilcheck.lookup_mult([side(s) for s in fs], side(t), (hc[m[0]], m[1]), n, field) == want
    for name, w in expect.items():
        assert (hc[name] == w).all(), "host form, matrix " + name
    return want_m, got


def distinct(n, k=3, salt=0):
    """n pairwise distinct tuples of k small patterns"""
    return [[(i * 2654435761 + salt) % 1000003] + [(i * (j + 3) + j) % 65521 for j in range(1, k)] for i in range(n)]


def shuffled(rows, seed):
    rows = list(rows)
    ref.rng(seed).shuffle(rows)
    return rows


@pytest.mark.parametrize("field", list(FIELDS))
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 257])
def test_wave_and_workgroup_edges(field, n):
    t = distinct(n, 1)
    f = [t[(i * 7 + 3) % n] for i in range(n)]
    f[n - 1] = t[n - 1]                                                          # the last lane's row counts
    m, rep = run(field, {"T": t, "F": f}, [("F", [0])], ("T", [0]), ("M", 1), n)
    assert rep == (0, NONE, NONE, n) and m[n - 1] >= 1
    g = [list(r) for r in f]
    g[n - 1][0] += 2000000                                                       # in no row of t: the last row fails, the rest still count
    m, rep = run(field, {"T": t, "F": g}, [("F", [0])], ("T", [0]), ("M", 0), n)
    assert rep == (1, 0, n - 1, n - 1)


@pytest.mark.parametrize("field", list(FIELDS))
def test_duplicates_in_t_and_its_selector(field):
    n = 96
    tup = distinct(6, 2, salt=5)
    t = [tup[i % 4] for i in range(n)]                                           # tuples 0..3 at rows 0..3 first, then again and again
    f = [tup[(i * i) % 4] for i in range(n)]
    m, rep = run(field, {"T": t, "F": f}, [("F", [0, 1])], ("T", [0, 1]), ("M", 2), n)
    assert rep == (0, NONE, NONE, n) and all(m[j] == 0 for j in range(4, n)) and sum(m[:4]) == n
    # selT unselects the first occurrence of tuples 0 and 1: the count lands on rows 4 and 5; the selector words 0 and q are both zero
    q = FIELDS[field]
    sel = [[0 if j == 0 else q if j == 1 else 1 + j] for j in range(n)]
    m2, rep = run(field, {"T": t, "F": f, "S": sel}, [("F", [0, 1])], ("T", [0, 1], ("S", 0)), ("M", 2), n)
    assert rep == (0, NONE, NONE, n) and (m2[0], m2[1], m2[4], m2[5]) == (0, 0, m[0], m[1]) and m2[2:4] == m[2:4]
    # tuple 4 is in t at an unselected row only, tuple 5 nowhere: f rows with either fail, and the unselected row of t gets 0
    t2 = [list(r) for r in t]
    t2[7] = list(tup[4])
    sel = [[0 if j == 7 else 1] for j in range(n)]
    g = [list(r) for r in f]
    g[50], g[20] = list(tup[4]), list(tup[5])
    m3, rep = run(field, {"T": t2, "F": g, "S": sel}, [("F", [0, 1])], ("T", [0, 1], ("S", 0)), ("M", 0), n)
    assert rep == (1, 0, 20, n - 2) and m3[7] == 0


@pytest.mark.parametrize("field", list(FIELDS))
@pytest.mark.parametrize("k", [1, 3, 16])
def test_widths_columns_out_of_order_and_where_m_lies(field, k):
    n, stride = 130, 2 * k + 5
    t = distinct(n, k)
    f = [t[(i * 11) % 40] for i in range(n)]
    # f in descending, non-adjacent columns stride-1, stride-3, ..; t in ascending columns 1, 3, ..; every other column holds poison
    f_cols, t_cols = [stride - 1 - 2 * j for j in range(k)], [1 + 2 * j for j in range(k)]
    fm = [[POISON[field] - c for c in range(stride)] for _ in range(n)]
    tm = [[POISON[field] - 1 - c for c in range(stride)] for _ in range(n)]
    for i in range(n):
        for j in range(k):
            fm[i][f_cols[j]], tm[i][t_cols[j]] = f[i][j], t[i][j]
    mats = {"T": tm, "F": fm}
    first = run(field, mats, [("F", f_cols)], ("T", t_cols), ("T", 0), n)       # a spare column of t's matrix
    assert first[1] == (0, NONE, NONE, n)
    assert run(field, mats, [("F", f_cols)], ("T", t_cols), ("F", 0), n) == first       # of f's matrix, whose columns read start at 6
    assert run(field, mats, [("F", f_cols)], ("T", t_cols), ("M", 1), n) == first       # a matrix of its own
    # ONE matrix for t and f: f in the descending odd columns from stride - 2, t in the even columns from 0, m in the last column
    f_cols, t_cols = [stride - 2 - 2 * j for j in range(k)], [2 * j for j in range(k)]
    both = [[POISON[field] - c for c in range(stride)] for _ in range(n)]
    for i in range(n):
        for j in range(k):
            both[i][f_cols[j]], both[i][t_cols[j]] = f[i][j], t[i][j]
    assert run(field, {"B": both}, [("B", f_cols)], ("B", t_cols), ("B", stride - 1), n) == first


@pytest.mark.parametrize("field", list(FIELDS))
@pytest.mark.parametrize("n_f", [1, 2, 8])
def test_sides_with_selectors_of_their_own(field, n_f):
    n = 100
    q = FIELDS[field]
    t = distinct(n, 2)
    mats = {"T": t}
    fs = []
    for s in range(n_f):
        mats["F%d" % s] = [t[(i * (s + 2) + s) % (10 + 7 * s)] + [q if (i + s) % 3 == 0 else 2 if s != 1 else 0] for i in range(n)]
        fs.append(("F%d" % s, [0, 1], ("F%d" % s, 2)))                            # the selector: column 2 of the side's own matrix; side 1 selects nothing
    m, rep = run(field, mats, fs, ("T", [0, 1]), ("M", 2), n)
    assert rep == (0, NONE, NONE, sum(1 for s in range(n_f) if s != 1 for i in range(n) if (i + s) % 3))


@pytest.mark.parametrize("field", list(FIELDS))
def test_elements_past_the_modulus_and_a_canonical_m(field):
    q, n = FIELDS[field], 70
    t = distinct(n, 2)
    f = [t[i % 9] for i in range(n)]
    lift = [q, 2 * q, 5 * q][:1 if field == "gl" else 3]                        # value + p fits 64 bits for these small values, + 2 p does not; + 5 r fits 256
    g = [[v + lift[(i + j) % len(lift)] if (i + j) % 3 else v for j, v in enumerate(r)] for i, r in enumerate(f)]
    t2 = [[v + q if (i + j) % 2 else v for j, v in enumerate(r)] for i, r in enumerate(t)]
    m, rep = run(field, {"T": t2, "F": g}, [("F", [0, 1])], ("T", [0, 1]), ("M", 0), n)
    assert rep == (0, NONE, NONE, n) and m[:9] == [8, 8, 8, 8, 8, 8, 8, 7, 7] and not any(m[9:])
    # run() compared m with the checker's element(): over Fr the Montgomery form of the count, computed here in Python
    assert mref.element(8, q) == (8 if field == "gl" else 8 * MONT % R) < q


@pytest.mark.parametrize("field", list(FIELDS))
def test_every_row_of_eight_sides_on_one_counter(field):
    n = 1 << 12
    t = distinct(n, 1)
    hot = 1234
    mats = {"T": t, "F": [t[hot]] * n}
    m, rep = run(field, mats, [("F", [0])] * 8, ("T", [0]), ("M", 1), n)
    assert rep == (0, NONE, NONE, 1 << 15) and m[hot] == 8 << 12 and sum(m) == 8 << 12


@pytest.mark.parametrize("field", list(FIELDS))
def test_three_tuples_that_share_a_home_slot(field):
    n, k = 8, 3
    cap = 1 << pilcheck.lookup_mult_plan(n, k, 1, field)["capBits"]
    assert cap == 16
    ew = 1 if field == "gl" else 4
    homes = {}
    for i in range(4096):                                                        # among any 2 cap + 1 candidates three share a slot
        tup = np.zeros((k, ew), np.uint64)
        tup[0, 0] = i
        homes.setdefault(pilcheck.tuple_home(tup, k, field, cap), []).append(i)
    three = next((v[:3] for v in homes.values() if len(v) >= 3), None)
    assert three is not None, "no three candidates share a home slot"
    t = [[three[i % 3], 0, 0] for i in range(n)]
    f = [[three[j], 0, 0] for j in (0, 0, 0, 0, 1, 1, 2, 2)]                     # four, two and two ... of which the selector keeps 4, 2, 1
    sel = [[1]] * 7 + [[0]]
    m, rep = run(field, {"T": t, "F": f, "S": sel}, [("F", [0, 1, 2], ("S", 0))], ("T", [0, 1, 2]), ("M", 0), n)
    assert pilcheck.lookup_mult_probe() > 0, "three tuples, one home: two of them lie past it"
    assert m == [4, 2, 1, 0, 0, 0, 0, 0] and rep == (0, NONE, NONE, 7)


@pytest.mark.parametrize("field", list(FIELDS))
def test_a_probe_run_that_wraps_past_the_last_slot(field):
    n, k = 4, 3
    cap = 1 << pilcheck.lookup_mult_plan(n, k, 1, field)["capBits"]
    assert cap == 16
    ew = 1 if field == "gl" else 4
    last, other = [], None
    for i in range(4096):                                                        # the first four small integers at home in the last slot, the first elsewhere
        tup = np.zeros((k, ew), np.uint64)
        tup[0, 0] = i
        if pilcheck.tuple_home(tup, k, field, cap) == cap - 1:
            last.append(i)
        elif other is None:
            other = i
        if len(last) == 4 and other is not None:
            break
    assert len(last) == 4 and other is not None, "too few candidates at home in slot 15"
    t = [[v, 0, 0] for v in last[:3] + [other]]                                  # slots 15, 0 and 1 whatever the order of arrival
    f = [t[2], t[0], t[2], t[3]]
    m, rep = run(field, {"T": t, "F": f}, [("F", [0, 1, 2])], ("T", [0, 1, 2]), ("M", 0), n)
    assert pilcheck.lookup_mult_probe() >= 2, "three tuples at home in the last slot: one of them lies in slot 1"
    assert m == [1, 0, 2, 1] and rep == (0, NONE, NONE, n)
    g = [list(r) for r in f]
    g[1] = [last[3], 0, 0]                                                       # in no row of t, and its search walks the wrapped run to its end
    m, rep = run(field, {"T": t, "F": g}, [("F", [0, 1, 2])], ("T", [0, 1, 2]), ("M", 0), n)
    assert m == [0, 0, 2, 1] and rep == (1, 0, 1, n - 1)


@pytest.mark.parametrize("field", list(FIELDS))
def test_absent_rows_in_two_sides(field):
    n = 300
    t = distinct(n, 2)
    f0 = [t[(i * 3) % 50] for i in range(n)]
    f1 = [t[(i * 5) % 70] for i in range(n)]
    f2 = [t[i % 20] for i in range(n)]
    for f, rows in ((f1, (290, 64, 129)), (f2, (5, 200))):
        for i in rows:
            f[i] = [f[i][0] + 3000000, f[i][1]]
    m, rep = run(field, {"T": t, "F0": f0, "F1": f1, "F2": f2}, [("F0", [0, 1]), ("F1", [0, 1]), ("F2", [0, 1])], ("T", [0, 1]), ("M", 2), n)
    assert rep == (1, 1, 64, 3 * n - 5), "side 1 before side 2 whatever the rows; within side 1 the smallest row"
    assert sum(m) == 3 * n - 5


@pytest.mark.parametrize("field", list(FIELDS))
def test_the_same_call_twice_and_the_sides_in_another_order(field):
    n = 1 << 10
    t = distinct(n, 2)
    mats = {"T": [r + [0] for r in t]}
    for s in range(3):
        mats["F%d" % s] = [t[(i * (s + 3)) % (5 + 40 * s)] for i in range(n)]
    fs = [("F%d" % s, [0, 1]) for s in range(3)]
    a = run(field, mats, fs, ("T", [0, 1]), ("T", 2), n)
    assert run(field, mats, fs, ("T", [0, 1]), ("T", 2), n) == a
    assert run(field, mats, fs, ("T", [0, 1]), ("T", 2), n, order=[2, 0, 1]) == a
    assert a[1] == (0, NONE, NONE, 3 * n)


@pytest.mark.parametrize("field", list(FIELDS))
def test_the_log_derivative_identity(field):
    """sum over the selected f rows of 1 / (c(f) + gamma) = sum over t's rows of m / (c(t) + gamma), c the alpha-compression: the identity
    the column exists for, in Python integers over the values the device wrote"""
    q, n, k = FIELDS[field], 1 << 10, 3
    rng = ref.rng(2024)
    table = distinct(200, k, salt=3)
    t = [table[i % 200] for i in range(n)]
    sel_t = [[0 if i < 100 else 1] for i in range(n)]                            # the first hundred tuples' first rows are not selected
    f0 = [table[rng.randrange(200)] for _ in range(n)]
    f1 = [table[rng.randrange(17)] for _ in range(n)]
    sel1 = [[rng.randrange(2)] for _ in range(n)]
    mats = {"T": [r + [POISON[field]] for r in t], "F0": f0, "F1": f1, "ST": sel_t, "S1": sel1}
    m, rep = run(field, mats, [("F0", [0, 1, 2]), ("F1", [0, 1, 2], ("S1", 0))], ("T", [0, 1, 2], ("ST", 0)), ("T", 3), n)
    assert rep[0] == 0
    alpha, gamma = rng.randrange(q), rng.randrange(q)
    val = (lambda v: v % q) if field == "gl" else (lambda v: v % q * pow(MONT, -1, q) % q)      # a pattern's field value
    c = lambda row: sum(pow(alpha, j, q) * val(v) for j, v in enumerate(row)) % q               # noqa: E731
    lhs = sum(pow(c(r) + gamma, -1, q) for r in f0) + sum(pow(c(r) + gamma, -1, q) for r, s in zip(f1, sel1) if s[0])
    rhs = sum(mj * pow(c(r) + gamma, -1, q) for mj, r in zip(m, t))
    assert lhs % q == rhs % q and rep[3] == n + sum(s[0] for s in sel1)


def test_python_resident_forms_and_refusals_with_a_device():
    lib = _lib.load()
    n = 64
    t = distinct(n, 2)
    tw = words("gl", [r + [7, 7] for r in t])
    d = to_dev(tw)
    assert pilcheck.lookup_mult_dev([(d, [0, 1]), (d, [0, 1], (d, 2))], (d, [0, 1]), (d, 3), n) == (0, NONE, NONE, 2 * n)
    assert (d.cpu().numpy().view(np.uint64).reshape(n, 4)[:, 3] == 2).all()
    assert pilcheck.lookup_mult_dev([(d, [1, 0])], (d, [0, 1]), (d, 2), n)[:3] == (1, 0, 0), "(a, b) against (b, a)"
    fr = to_dev(words("bn128", [r + [1] for r in t]))
    assert pilcheck.lookup_mult_dev([(fr, [1], (fr, 0))], (fr, [1], (fr, 0)), (fr, 2), n, field="bn128")[0] == 0
    with pytest.raises(pil2gl.Pil2glError):
        pilcheck.lookup_mult_dev([(tw, [0, 1])], (d, [0, 1]), (d, 3), n)
    with pytest.raises(pil2gl.Pil2glError, match="m overlaps"):
        pilcheck.lookup_mult_dev([(d, [0, 1])], (d, [0, 1]), (d, 1), n)
    need = pilcheck.lookup_mult_plan(n, 2)["scratchBytes"]
    work = torch.empty(need // 8, dtype=torch.int64, device="cuda")
    cols = np.array([0, 1], np.uint64)
    side = _lib.TupleSide(d.data_ptr(), 4, cols.ctypes.data, None, 0, 0)
    rep = (C.c_uint64 * 4)()
    ok = [C.byref(side), 1, C.byref(side), d.data_ptr(), 4, 2, n, 2, work.data_ptr(), need, rep, None]

    def call(**kw):
        args = list(ok)
        for key, v in kw.items():
            args[int(key[1:])] = v
        return lib.pil2gl_lookup_mult_dev(*args)
    assert call() == 0 and tuple(rep) == (0, NONE, NONE, n)
    assert call(a8=d.data_ptr() + 16) == -1 and b"overlaps" in lib.pil2gl_last_error()
    assert call(a9=need - 16) == -1 and b"scratch" in lib.pil2gl_last_error()
    assert call(a5=0) == -1 and b"m overlaps" in lib.pil2gl_last_error()
    assert call(a3=d.data_ptr() + 32, a5=3) == -1 and b"m overlaps" in lib.pil2gl_last_error(), "another base over the same words"
    assert call(a4=1) == -1 and b"stride" in lib.pil2gl_last_error()
    assert call(a1=9) == -1 and call(a7=17) == -1 and call(a6=(1 << 28) + 1) == -1
    assert call(a6=0, a8=None) == 0 and tuple(rep) == (0, NONE, NONE, 0)
