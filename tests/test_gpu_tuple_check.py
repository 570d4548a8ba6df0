"""The lookup and permutation checks on the device (csrc/tuple_check.hip) against the dictionary checker (tests/tuple_check_ref.py): all
five words of the report, both fields, both modes, the resident and the host forms.  Every case goes through check(): the resident form
with the caller's working buffer followed by guard words, the host form, and the checker on the same words; the guard words and the
input matrices must come back unchanged.  Elements are given as bit patterns: the checker and the device both count them mod the modulus
(over Fr two Montgomery patterns are equal mod r exactly when their values are), so no case needs a conversion.
The shapes are the smallest at which the kernels can still go wrong: one row, fewer rows than a wave (16), failing rows across a wave
edge (63 | 64), more than one workgroup (2^12 distinct tuples: 8192 table rows), four tuples under 2^10 rows each side (counters in the
hundreds, atomicMin chains on one slot), k = 1, 3 and 16, three tuples that share a home slot."""
import ctypes as C

import numpy as np
import pytest

import tuple_check_ref as tref
import conn_pols_ref as ref
from conn_pols_ref import P, R

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from pil2gl import _lib, pilcheck  # noqa: E402
import pil2gl  # noqa: E402

FIELDS = {"gl": P, "bn128": R}
L, M = tref.LOOKUP, tref.PERMUTATION
NONE, CLEAN = tref.NONE, tref.CLEAN_REPORT
GUARD = 0x6B6B6B6B6B6B6B6B
POISON = {"gl": 0xDEADBEEFDEADBEEF, "bn128": (1 << 256) - 0x1234567}
BOTH = [(f, m) for f in FIELDS for m in (L, M)]


def words(field, rows):
    """rows of integer bit patterns -> the library's matrix: (n, stride) uint64, or (n, stride, 4)"""
    if field == "gl":
        return np.array(rows, np.uint64).reshape(len(rows), -1)
    return ref.fr_words([v for row in rows for v in row]).reshape(len(rows), -1, 4)


def to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


def check(field, mode, f, f_cols, t, t_cols, n, sel_f=None, sel_t=None, one=False):
    """f, t: word matrices; sel_*: (word matrix, col) or None; one: f and t are ONE device tensor -> the report, which all three give"""
    q, ew = FIELDS[field], 1 if field == "gl" else 4
    k = len(f_cols)
    want = tref.check(tref.tuples(f, f_cols, q), tref.tuples(t, t_cols, q), mode, q,
                      None if sel_f is None else tref.column(sel_f[0], sel_f[1], q), None if sel_t is None else tref.column(sel_t[0], sel_t[1], q))
    lib = _lib.load()
    need = pilcheck.tuple_check_plan(n, k, field, mode)["scratchBytes"]
    work = torch.full((need // 8 + 8,), GUARD, dtype=torch.int64, device="cuda")
    df = to_dev(f)
    dt = df if one else to_dev(t)
    dsf, dst = (None if s is None else to_dev(s[0]) for s in (sel_f, sel_t))
    fc, tc = np.array(f_cols, np.uint64), np.array(t_cols, np.uint64)
    rep = (C.c_uint64 * 5)()
    ptr = lambda x: None if x is None else x.data_ptr()                          # noqa: E731
    stride = lambda s: 0 if s is None else s[0].shape[1]                         # noqa: E731
    col = lambda s: 0 if s is None else s[1]                                     # noqa: E731
    fn = lib.pil2gl_tuple_check_dev if ew == 1 else lib.pil2gl_bn128_tuple_check_dev
    rc = fn(df.data_ptr(), f.shape[1], fc.ctypes.data, dt.data_ptr(), t.shape[1], tc.ctypes.data, ptr(dsf), stride(sel_f), col(sel_f),
            ptr(dst), stride(sel_t), col(sel_t), n, k, mode, work.data_ptr(), need, rep, None)
    assert rc == 0, lib.pil2gl_last_error()
    got = tuple(int(x) for x in rep)
    assert (work[need // 8:].cpu().numpy().view(np.uint64) == GUARD).all(), "a write past scratchBytes"
    for d, h in ((df, f), (dt, t)) + tuple((d, s[0]) for d, s in ((dsf, sel_f), (dst, sel_t)) if s is not None):
        assert (d.cpu().numpy().view(np.uint64).reshape(h.shape) == h).all(), "an input matrix changed"
    host = (pilcheck.lookup_check if mode == L else pilcheck.perm_check)(f, f_cols, t, t_cols, n, field, sel_f=sel_f, sel_t=sel_t)
    assert got == want and host == want, (got, host, want)
    return got


def distinct(n, k=3, salt=0):
    """n pairwise distinct tuples of k small patterns"""
    return [[(i * 2654435761 + salt) % 1000003] + [(i * (j + 3) + j) % 65521 for j in range(1, k)] for i in range(n)]


def shuffled(rows, seed):
    rows = list(rows)
    ref.rng(seed).shuffle(rows)
    return rows


@pytest.mark.parametrize("field,mode", BOTH)
def test_small_and_edge_sizes(field, mode):
    cols = [0, 1, 2]
    assert check(field, mode, words(field, [[5, 6, 7]]), cols, words(field, [[5, 6, 7]]), cols, 1) == CLEAN
    assert check(field, mode, words(field, [[5, 6, 8]]), cols, words(field, [[5, 6, 7]]), cols, 1) == (1, 0, NONE, 1, 0)
    for n in (16, 128, 1 << 12):
        t = distinct(n)
        f = shuffled(t, n)
        assert check(field, mode, words(field, f), cols, words(field, t), cols, n) == CLEAN
        for x in {n - 1, 0} | ({63, 64} if n == 128 else set()):
            g = [list(r) for r in f]
            g[x][2] += 70000                                                     # differs in the last column only: in no row of t
            assert check(field, mode, words(field, g), cols, words(field, t), cols, n) == (1, x, NONE, 1, 0)
    # rows 63 and 64 of t, across the wave edge, in a permutation whose f has nothing selected: kind 3 at the smaller of those t selects
    t = distinct(128)
    zero = words(field, [[0]] * 128)
    for first in (63, 64):
        sel_t = words(field, [[1 if i >= first else 0] for i in range(128)])
        want = CLEAN if mode == L else (3, first, NONE, 0, 1)
        assert check(field, mode, words(field, t), cols, words(field, t), cols, 128, sel_f=(zero, 0), sel_t=(sel_t, 0)) == want


@pytest.mark.parametrize("field", list(FIELDS))
def test_four_tuples_under_a_thousand_rows(field):
    n, cols = 1 << 10, [0, 1, 2]
    tup = distinct(4, salt=9)
    t = shuffled([tup[i % 4] for i in range(n)], 1)                               # 256 of each
    f = shuffled([tup[0]] * 300 + [tup[1]] * 212 + [tup[2]] * 256 + [tup[3]] * 256, 2)
    fw, tw = words(field, f), words(field, t)
    assert check(field, L, fw, cols, tw, cols, n) == CLEAN
    first_f, first_t = f.index(tup[0]), t.index(tup[0])
    assert check(field, M, fw, cols, tw, cols, n) == (2, first_f, first_t, 300, 256)
    # the same counts on both sides, then tuple 1 deselected in f from row 400 on: t has more of it, f's first row of it is the partner
    f = shuffled(t, 3)
    sel = [[0 if r == tup[1] and i >= 400 else 1] for i, r in enumerate(f)]
    left = sum(1 for i, r in enumerate(f) if r == tup[1] and i < 400)
    assert 50 < left < 200
    got = check(field, M, words(field, f), cols, tw, cols, n, sel_f=(words(field, sel), 0))
    assert got == (3, t.index(tup[1]), f.index(tup[1]), left, 256)


@pytest.mark.parametrize("field,mode", BOTH)
@pytest.mark.parametrize("k", [1, 3, 16])
def test_widths_and_columns_of_wider_matrices(field, mode, k):
    n, stride = 200, 2 * k + 5
    t = distinct(n, k)
    f = shuffled(t, k)
    f[150] = list(f[10])                                                         # one tuple twice in f: row 10 in a permutation; its old tuple is t's alone
    # f in descending, non-adjacent columns stride-1, stride-3, ..; t in ascending columns 1, 3, ..; every other column holds poison
    f_cols, t_cols = [stride - 1 - 2 * j for j in range(k)], [1 + 2 * j for j in range(k)]
    fm = [[POISON[field]] * stride for _ in range(n)]
    tm = [[POISON[field] - 1] * stride for _ in range(n)]
    for i in range(n):
        for j in range(k):
            fm[i][f_cols[j]], tm[i][t_cols[j]] = f[i][j], t[i][j]
    got = check(field, mode, words(field, fm), f_cols, words(field, tm), t_cols, n)
    assert got == (CLEAN if mode == L else (2, 10, t.index(f[10]), 2, 1))
    # f and t as column sets of ONE matrix 2 k + 5 wide: f in the descending odd columns from stride - 2, t in the even columns from 0
    f_cols, t_cols = [stride - 2 - 2 * j for j in range(k)], [2 * j for j in range(k)]
    both = [[POISON[field]] * stride for _ in range(n)]
    for i in range(n):
        for j in range(k):
            both[i][f_cols[j]], both[i][t_cols[j]] = f[i][j], t[i][j]
    w = words(field, both)
    assert check(field, mode, w, f_cols, w, t_cols, n, one=True) == got


@pytest.mark.parametrize("field,mode", BOTH)
def test_selectors(field, mode):
    q, n, cols = FIELDS[field], 96, [1, 0]
    top = (1 << 64) - 1 if field == "gl" else (1 << 256) - 1
    t = distinct(n, 2)
    f = shuffled(t, 5)
    pat = [0, q, 1, top]                                                         # zero, zero, selected, selected (top is not 0 mod q)
    sel_f = words(field, [[POISON[field], pat[i % 4]] for i in range(n)])
    in_f = {tuple(r) for i, r in enumerate(f) if i % 4 >= 2}
    sel_t = words(field, [[1 if tuple(r) in in_f else q] for r in t])
    fw, tw = words(field, [r[::-1] for r in f]), words(field, [r[::-1] for r in t])
    assert check(field, mode, fw, cols, tw, cols, n, sel_f=(sel_f, 1), sel_t=(sel_t, 0)) == CLEAN
    assert check(field, mode, fw, cols, tw, cols, n, sel_f=(sel_f, 1)) == (CLEAN if mode == L else (3, min(i for i, r in enumerate(t) if tuple(r) not in in_f), NONE, 0, 1))
    x = min(i for i, r in enumerate(f) if tuple(r) not in in_f)
    assert check(field, mode, fw, cols, tw, cols, n, sel_t=(sel_t, 0)) == (1, x, NONE, 1, 0)
    none = words(field, [[0]] * n)
    assert check(field, mode, fw, cols, tw, cols, n, sel_f=(none, 0)) == (CLEAN if mode == L else (3, 0, NONE, 0, 1))
    assert check(field, mode, fw, cols, tw, cols, n, sel_t=(none, 0)) == (1, 0, NONE, 1, 0)


@pytest.mark.parametrize("field,mode", BOTH)
def test_elements_past_the_modulus_equal_their_residues(field, mode):
    q, n, cols = FIELDS[field], 70, [0, 1]
    t = distinct(n, 2)
    f = shuffled(t, 8)
    lift = [q, 2 * q, 5 * q][:1 if field == "gl" else 3]                        # value + p fits 64 bits for these small values, + 2 p does not; + 5 r fits 256
    g = [[v + lift[(i + j) % len(lift)] if (i + j) % 3 else v for j, v in enumerate(r)] for i, r in enumerate(f)]
    assert check(field, mode, words(field, g), cols, words(field, t), cols, n) == CLEAN
    g[33][1] += 1                                                                # still past the modulus, now another residue
    assert check(field, mode, words(field, g), cols, words(field, t), cols, n)[:2] == (1, 33)


@pytest.mark.parametrize("field", list(FIELDS))
def test_minimum_and_priority(field):
    n, cols = 1 << 11, [0, 1, 2]
    t = distinct(n)
    f = shuffled(t, 4)
    tw = words(field, t)
    lo, hi = 300, 1900                                                           # table rows n + 300 and n + 1900: different workgroups
    g = [list(r) for r in f]
    g[lo][0] += 2000000
    g[hi][0] += 2000000
    for mode in (L, M):
        assert check(field, mode, words(field, g), cols, tw, cols, n) == (1, lo, NONE, 1, 0)
    one = [list(r) for r in f]
    one[hi][0] += 2000000
    assert check(field, M, words(field, one), cols, tw, cols, n) == (1, hi, NONE, 1, 0)
    # kind 2 at the smaller row against kind 1 at the larger, and the other way round: the smaller row wins whatever its kind
    a = [list(r) for r in f]
    a[hi] = list(a[lo])                                                          # the tuple of row lo twice: kind 2 at lo; t's tuple of old row hi: kind 3, not reported
    assert check(field, M, words(field, a), cols, tw, cols, n) == (2, lo, t.index(f[lo]), 2, 1)
    a[100][0] += 2000000                                                         # kind 1 at row 100 < lo
    assert check(field, M, words(field, a), cols, tw, cols, n) == (1, 100, NONE, 1, 0)
    b = [list(r) for r in f]
    b[lo][0] += 2000000                                                          # kind 1 at lo
    b[hi] = list(b[50])                                                          # kind 2 at 50 < lo
    assert check(field, M, words(field, b), cols, tw, cols, n) == (2, 50, t.index(f[50]), 2, 1)
    # kind 3 only when no row of f fails: f short of one tuple by deselecting its row
    sel = words(field, [[0 if i == hi else 1] for i in range(n)])
    assert check(field, M, words(field, f), cols, tw, cols, n, sel_f=(sel, 0)) == (3, t.index(f[hi]), NONE, 0, 1)
    assert check(field, L, words(field, f), cols, tw, cols, n, sel_f=(sel, 0)) == CLEAN


@pytest.mark.parametrize("field", list(FIELDS))
def test_three_tuples_that_share_a_home_slot(field):
    n, k = 8, 3
    cap = 1 << pilcheck.tuple_check_plan(n, k, field)["capBits"]
    assert cap == 32
    ew = 1 if field == "gl" else 4
    homes = {}
    for i in range(4096):                                                        # among any 2 cap + 1 candidates three share a slot
        tup = np.zeros((k, ew), np.uint64)
        tup[0, 0] = i
        homes.setdefault(pilcheck.tuple_home(tup, k, field, cap), []).append(i)
    three = next((v[:3] for v in homes.values() if len(v) >= 3), None)
    assert three is not None, "no three candidates share a home slot"
    rows = [[three[i % 3], 0, 0] for i in range(n)]                              # t: three each of the first two, two of the third
    fw = words(field, [[three[j], 0, 0] for j in (0, 0, 0, 0, 1, 1, 2, 2)])     # f: four of the first
    for mode in (L, M):
        got = check(field, mode, fw, [0, 1, 2], words(field, rows), [0, 1, 2], n)
        assert pilcheck.tuple_check_probe() >= 2, "three tuples, one home: one of them lies two slots on"
        assert got == (CLEAN if mode == L else (2, 0, 0, 4, 3))
    g = [list(r) for r in rows]
    g[5] = [4096, 0, 0]
    assert check(field, L, words(field, g), [0, 1, 2], words(field, rows), [0, 1, 2], n) == (1, 5, NONE, 1, 0)


@pytest.mark.parametrize("field", list(FIELDS))
def test_a_probe_run_that_wraps_past_the_last_slot(field):
    n, k, cols = 4, 3, [0, 1, 2]
    cap = 1 << pilcheck.tuple_check_plan(n, k, field)["capBits"]
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
    f = [t[2], t[3], t[0], t[1]]
    g = [list(r) for r in f]
    g[2] = [last[3], 0, 0]                                                       # in no row of t, and its search walks the wrapped run to its end
    for mode in (L, M):
        assert check(field, mode, words(field, f), cols, words(field, t), cols, n) == CLEAN
        assert pilcheck.tuple_check_probe() >= 2, "three tuples at home in the last slot: one of them lies in slot 1"
        assert check(field, mode, words(field, g), cols, words(field, t), cols, n) == (1, 2, NONE, 1, 0)


def test_python_resident_forms_and_refusals_with_a_device():
    lib = _lib.load()
    t = distinct(64, 2)
    tw = words("gl", t)
    d = to_dev(tw)
    assert pilcheck.lookup_check_dev(d, [0, 1], d, [0, 1], 64) == CLEAN
    assert pilcheck.perm_check_dev(d, [0, 1], d, [1, 0], 64)[0] == 1, "(a, b) against (b, a)"
    fr = to_dev(words("bn128", t))
    assert pilcheck.perm_check_dev(fr, [1], fr, [1], 64, field="bn128", sel_f=(fr, 0), sel_t=(fr, 0)) == CLEAN
    with pytest.raises(pil2gl.Pil2glError):
        pilcheck.lookup_check_dev(tw, [0, 1], d, [0, 1], 64)
    need = pilcheck.tuple_check_plan(64, 2)["scratchBytes"]
    work = torch.empty(need // 8, dtype=torch.int64, device="cuda")
    cols = np.array([0, 1], np.uint64)
    rep = (C.c_uint64 * 5)()
    ok = [d.data_ptr(), 2, cols.ctypes.data, d.data_ptr(), 2, cols.ctypes.data, None, 0, 0, None, 0, 0, 64, 2, 1, work.data_ptr(), need, rep, None]

    def call(**kw):
        args = list(ok)
        for key, v in kw.items():
            args[int(key[1:])] = v
        return lib.pil2gl_tuple_check_dev(*args)
    assert call() == 0 and tuple(rep) == CLEAN
    assert call(a15=d.data_ptr() + 16) == -1 and b"overlaps" in lib.pil2gl_last_error()
    assert call(a16=need - 16) == -1 and b"scratch" in lib.pil2gl_last_error()
    assert call(a1=1) == -1 and b"stride" in lib.pil2gl_last_error()
    assert call(a14=2) == -1 and call(a13=17) == -1 and call(a12=(1 << 28) + 1) == -1
    assert call(a12=0, a15=None) == 0 and tuple(rep) == CLEAN
