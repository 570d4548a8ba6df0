"""The range-check multiplicities on the device (csrc/range_mult.hip) against the checker over Python integers (tests/range_mult_ref.py):
every element of m and all four words of the report, both fields, the resident and the host forms.  Every case goes through run(): the
resident form with the caller's working buffer followed by guard words, the host form on copies, and the checker on the same words; the
guard words, every input matrix and every column of m's matrix other than m must come back unchanged.  Elements are given as bit
patterns (rref.pattern makes an integer's).  The shapes are the smallest at which each piece can go wrong: one row, the wave and workgroup
edges, both sides of the planner's threshold, several workgroups that flush into the same counters, 2^17 rows on one counter."""
import ctypes as C

import numpy as np
import pytest

import range_mult_ref as rref
import conn_pols_ref as ref
from conn_pols_ref import P, R

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from pil2gl import _lib, pilcheck  # noqa: E402
import pil2gl  # noqa: E402

FIELDS = {"gl": P, "bn128": R}
NONE = rref.NONE
GUARD = 0x6B6B6B6B6B6B6B6B
POISON = {"gl": 0xDEADBEEFDEADBEEF, "bn128": (1 << 256) - 0x1234567}


def threshold():
    """the largest size that takes the LDS path, from the planner alone"""
    lo, hi = 0, 1 << 28
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if pilcheck.range_mult_plan(1 << 28, mid)["path"] == 0 else (lo, mid)
    return lo


T = threshold()


def words(field, rows):
    """rows of integer bit patterns -> the library's matrix: (n, stride) uint64, or (n, stride, 4)"""
    if field == "gl":
        return np.array(rows, np.uint64).reshape(len(rows), -1)
    return ref.fr_words([v for row in rows for v in row]).reshape(len(rows), -1, 4)


def to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


def column(field, values, stride=1, col=0, fill=None):
    """the integers `values` as the patterns of column col of a matrix `stride` wide; the other columns hold poison"""
    q = FIELDS[field]
    return [[rref.pattern(v, q) if c == col else (POISON[field] - c if fill is None else fill) for c in range(stride)] for v in values]


def run(field, mats, fs, lo, size, m, n, row0=0, order=None, path=None, host=True):
    """mats: name -> rows of bit patterns (a matrix); fs: sides (name, col) or (name, col, (selector's name, col)); m: (name, col), a name
    that mats lacks being a matrix of its own, 3 wide and poisoned; order: the f sides as the call gets them; path: the count kernel forced
    -> (m as counts, the report), which the resident form, the host form and the checker all give"""
    q, ew = FIELDS[field], 1 if field == "gl" else 4
    mats = dict(mats)
    if m[0] not in mats:
        mats[m[0]] = [[POISON[field] - i - j for j in range(3)] for i in range(n)]
    hostm = {name: words(field, rows) for name, rows in mats.items()}
    fs = [fs[i] for i in order] if order else list(fs)
    col = lambda name, c: [row[c] for row in mats[name]]                         # noqa: E731
    sels = [None if len(s) < 3 or s[2] is None else col(*s[2]) for s in fs]
    want_m, want = rref.multiplicities([col(s[0], s[1]) for s in fs], lo, size, n, q, sels, row0)
    lib = _lib.load()
    need = pilcheck.range_mult_plan(n, size, len(fs), field, path)["scratchBytes"]
    assert need == (64 + 4 * size + 15) // 16 * 16
    work = torch.full((need // 8 + 8,), GUARD, dtype=torch.int64, device="cuda")
    dev = {name: to_dev(w) for name, w in hostm.items()}
    keep = []

    def struct(s):
        cols = np.array([s[1]], np.uint64)
        keep.append(cols)
        sel = s[2] if len(s) > 2 and s[2] is not None else None
        return _lib.TupleSide(dev[s[0]].data_ptr(), hostm[s[0]].shape[1], cols.ctypes.data, None if sel is None else dev[sel[0]].data_ptr(),
                              0 if sel is None else hostm[sel[0]].shape[1], 0 if sel is None else sel[1])
    F = (_lib.TupleSide * len(fs))(*[struct(s) for s in fs])
    rep = (C.c_uint64 * 4)()
    args = [F, len(fs), lo, size, row0, dev[m[0]].data_ptr(), hostm[m[0]].shape[1], m[1], n, work.data_ptr(), need, rep, None]
    if path is None:
        rc = (lib.pil2gl_range_mult_dev if ew == 1 else lib.pil2gl_bn128_range_mult_dev)(*args)
    else:
        rc = lib.pil2gl_debug_range_mult_dev(*(args + [ew, path]))
    assert rc == 0, lib.pil2gl_last_error()
    got = tuple(int(x) for x in rep)
    assert (work[need // 8:].cpu().numpy().view(np.uint64) == GUARD).all(), "a write past scratchBytes"
    expect = {name: w.copy() for name, w in hostm.items()}
    expect[m[0]][:n, m[1]] = words(field, [[rref.element(c, q)] for c in want_m])[:, 0]
    for name, w in expect.items():
        back = dev[name].cpu().numpy().view(np.uint64).reshape(w.shape)
        assert (back == w).all(), "matrix %s: an input changed, or m differs from the checker at rows %s" % (
            name, np.argwhere((back != w).reshape(len(w), -1).any(1)).ravel()[:8])
    assert got == want, (got, want)
    assert sum(want_m) == got[3], "the sum of m is `matched`"
    if host:                                          # the host form, on copies; one array a name
        hc = {name: w.copy() for name, w in hostm.items()}
        side = lambda s: (hc[s[0]], [s[1]], None if len(s) < 3 or s[2] is None else (hc[s[2][0]], s[2][1]))      # noqa: E731
        assert pilcheck.range_mult([side(s) for s in fs], lo, size, (hc[m[0]], m[1]), n, field, row0) == want
        for name, w in expect.items():
            assert (hc[name] == w).all(), "host form, matrix " + name
    return want_m, got


def spread(n, lo, size, seed):
    """n integers of the range, every value of a small range at least once where n allows"""
    r = ref.rng(seed)
    return [lo + (i if i < size else r.randrange(size)) for i in range(n)]


SHAPES = sorted({(1, 1), (1, 63), (2, 65), (256, 1000), (256, (1 << 13) + 3), (max(T - 1, 1), (1 << 13) + 3), (max(T, 1), (1 << 13) + 3),
                 (T + 1, (1 << 13) + 3), (1 << 14, (1 << 14) + 5)})


@pytest.mark.parametrize("field", list(FIELDS))
@pytest.mark.parametrize("size,n", SHAPES)
def test_range_shapes_on_the_planners_path(field, size, n):
    lo = 1000
    f = spread(n, lo, size, size + n)
    f[n - 1] = lo + size - 1                                                     # the last lane's row counts, at the last counter
    m, rep = run(field, {"F": column(field, f, 2, 1)}, [("F", 1)], lo, size, ("M", 1), n)
    assert rep == (0, NONE, NONE, n) and m[size - 1] >= 1 and not any(m[size:])
    if n > 1:
        f[n - 1] = lo + size                                                     # the last row fails, the rest still count
        m, rep = run(field, {"F": column(field, f, 2, 1)}, [("F", 1)], lo, size, ("M", 0), n, host=False)
        assert rep == (1, 0, n - 1, n - 1)


@pytest.mark.parametrize("field", list(FIELDS))
@pytest.mark.parametrize("path", [0, 1])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_wave_edges_on_each_count_kernel(field, path, n):
    """the end of a count kernel is wave-level (csrc/mult_column.cuh): one lane, a wave less one, a whole wave, a wave and one, a workgroup of
    path 1 and one, each with its only failing row in the last lane that has one"""
    size, lo = min(3, n), -1
    f = [lo + i % size for i in range(n)]
    f[n - 1] = lo + size
    m, rep = run(field, {"F": column(field, f)}, [("F", 0)], lo, size, ("M", 1), n, path=path, host=False)
    assert rep == (1, 0, n - 1, n - 1) and sum(m) == n - 1


@pytest.mark.parametrize("field", list(FIELDS))
@pytest.mark.parametrize("path", [0, 1])
def test_several_workgroups_flush_into_the_same_counters(field, path):
    n, size = (1 << 13) + 3, 256
    assert pilcheck.range_mult_plan(n, size, 1, field, path)["blocks"] >= 3 and pilcheck.range_mult_plan(n, size, 1, field, path)["path"] == path
    f = [-128 + (i * 7) % size for i in range(n)]
    m, rep = run(field, {"F": column(field, f)}, [("F", 0)], -128, size, ("M", 2), n, path=path, host=False)
    assert rep == (0, NONE, NONE, n) and min(m[:size]) >= n // size


@pytest.mark.parametrize("field", list(FIELDS))
def test_negative_lo_straddles_zero(field):
    q, n, size = FIELDS[field], 300, 256
    f = [q - 128 + i for i in range(128)] + list(range(128)) + [q - 1, 0, -128, 127] * 11      # p - 128 .. p - 1, 0 .. 127, and again
    m, rep = run(field, {"F": column(field, f)}, [("F", 0)], -128, size, ("M", 0), n)
    assert rep == (0, NONE, NONE, n) and m[0] == 12 and m[127] == 12 and m[128] == 12 and m[255] == 12 and m[5] == 1 and not any(m[256:])
    g = list(f)
    g[17], g[200] = -129, 128
    m, rep = run(field, {"F": column(field, g)}, [("F", 0)], -128, size, ("M", 0), n, host=False)
    assert rep == (1, 0, 17, n - 2)


@pytest.mark.parametrize("field", list(FIELDS))
def test_values_just_outside(field):
    q, n = FIELDS[field], 70
    lo, size = 5000, 64
    for row, (v, why) in enumerate(((lo - 1, "lo - 1"), (lo + size, "lo + size"), (lo + (1 << 32), "lo + 2^32: a difference truncated to 32 bits"),
                                    (lo + 3 + (1 << 32) * 7, "a multiple of 2^32 above a value in range"), (lo + (1 << 64), "lo + 2^64: lo + 2^32 - 1 mod p"))):
        f = spread(n, lo, size, 3)
        f[row + 2] = v
        m, rep = run(field, {"F": column(field, f)}, [("F", 0)], lo, size, ("M", 0), n, host=False)
        assert rep == (1, 0, row + 2, n - 1), why
    f = [0] * n
    f[9] = q - 1                                                                 # -1 against [0, 64)
    assert run(field, {"F": column(field, f)}, [("F", 0)], 0, size, ("M", 0), n)[1] == (1, 0, 9, n - 1)
    if field == "bn128":                                                         # a VALUE with only limb 3 set, and one with only limb 1
        for v in (1 << 192, 5 << 192, 1 << 64, (1 << 128) + 3):
            f = [3] * n
            f[33] = v
            assert run(field, {"F": column(field, f)}, [("F", 0)], 0, size, ("M", 0), n, host=False)[1] == (1, 0, 33, n - 1), hex(v)
    # lo at the ends of the signed range
    for lo in (-(1 << 63), (1 << 63) - size):
        f = spread(n, lo, size, 4)
        f[7] = lo - 1
        f[8] = lo + size
        assert run(field, {"F": column(field, f)}, [("F", 0)], lo, size, ("M", 0), n, host=False)[1] == (1, 0, 7, n - 2), lo


@pytest.mark.parametrize("field", list(FIELDS))
def test_non_canonical_inputs_count_as_their_residue(field):
    q, n, size = FIELDS[field], 66, 16
    if field == "gl":
        rows = [[P + 5], [(1 << 64) - 1], [P], [5]] + [[P + (i % 16)] for i in range(n - 4)]      # 5, 2^32 - 2, 0, 5, ..
        m, rep = run(field, {"F": rows}, [("F", 0)], 0, size, ("M", 0), n)
        assert rep == (1, 0, 1, n - 1), "2^64 - 1 is 2^32 - 2: outside [0, 16)"
        assert run(field, {"F": rows}, [("F", 0)], (1 << 32) - 2, 1, ("M", 0), n, host=False)[1][3] == 1, "... and inside [2^32 - 2, 2^32 - 2]"
    else:
        pat = lambda v: rref.pattern(v, R)                                       # noqa: E731
        lifts = [k for k in range(1, 6)]                                         # pattern + k r stays below 2^256 for k <= 4 always, 5 for small patterns
        rows = [[pat(i % 16) + R * lifts[i % 4]] for i in range(n)]
        assert all(R <= r[0] < 1 << 256 for r in rows)
        rows[3] = [(1 << 256) - 1]                                               # the largest pattern: some value far outside
        rows[4] = [pat(7) + 5 * R] if pat(7) + 5 * R < 1 << 256 else [pat(7) + 4 * R]
        m, rep = run(field, {"F": rows}, [("F", 0)], 0, size, ("M", 0), n)
        assert rep == (1, 0, 3, n - 1)


@pytest.mark.parametrize("field", list(FIELDS))
def test_selectors(field):
    q, n, size = FIELDS[field], 130, 10
    f = spread(n, 20, size, 8)
    f[5], f[70], f[129] = 19, 30, 1 << 40                                        # out of range, in unselected rows
    sel = [1 + i for i in range(n)]
    sel[5], sel[70], sel[129], sel[6] = 0, q, 0, q                               # 0 and the non-canonical zero unselect; row 6 is in range and does not count
    rows = [[rref.pattern(v, q), s] for v, s in zip(f, sel)]
    m, rep = run(field, {"F": rows}, [("F", 0, ("F", 1))], 20, size, ("M", 1), n)
    assert rep == (0, NONE, NONE, n - 4)
    rows[70][1] = 2 * q if field == "bn128" else 7                                # selected now (2 r is zero too: it stays unselected over Fr)
    m, rep = run(field, {"F": rows}, [("F", 0, ("F", 1))], 20, size, ("M", 1), n, host=False)
    assert rep == ((1, 0, 70, n - 4) if field == "gl" else (0, NONE, NONE, n - 4))
    # the selector in a matrix of its own, shared by two sides of which one has none
    mats = {"F": [r[:1] for r in rows], "S": [[POISON[field], s] for s in sel]}
    m, rep = run(field, mats, [("F", 0, ("S", 1)), ("F", 0)], 20, size, ("M", 0), n)
    assert rep == (1, 1, 5, 2 * (n - 4) + 1)


@pytest.mark.parametrize("field", list(FIELDS))
@pytest.mark.parametrize("size", [256, 1 << 14])
def test_every_row_of_eight_sides_on_one_counter(field, size):
    n = 1 << 14
    path = pilcheck.range_mult_plan(n, size, 8, field)["path"]
    assert path == (0 if size <= T else 1)
    hot = 77
    mats = {"F": column(field, [-50 + hot] * n)}
    m, rep = run(field, mats, [("F", 0)] * 8, -50, size, ("M", 1), n, host=False)
    assert rep == (0, NONE, NONE, 1 << 17) and m[hot] == 1 << 17 and sum(m) == 1 << 17
    other = 1 - path                                                             # and the other count kernel on the same input, where it can run
    if size <= 8192:
        assert run(field, mats, [("F", 0)] * 8, -50, size, ("M", 1), n, path=other, host=False) == (m, rep)


@pytest.mark.parametrize("field", list(FIELDS))
def test_offset_table_and_rows_outside_it(field):
    n, size = 333, 100
    row0 = n - size
    f = spread(n, 7, size, 5)
    m, rep = run(field, {"F": column(field, f)}, [("F", 0)], 7, size, ("M", 2), n, row0=row0)      # M is pre-filled with poison
    assert rep == (0, NONE, NONE, n) and not any(m[:row0]) and all(c >= 1 for c in m[row0:])
    m2, rep = run(field, {"F": column(field, f)}, [("F", 0)], 7, size, ("M", 2), n, row0=17, host=False)
    assert m2[17:117] == m[row0:] and not any(m2[:17]) and not any(m2[117:])
    m3, rep = run(field, {"F": column(field, f)}, [("F", 0)], 7 + size - 1, 1, ("M", 0), n, row0=n - 1, host=False)
    assert m3[n - 1] == m[n - 1] and rep[:3] == (1, 0, 0)


@pytest.mark.parametrize("field", list(FIELDS))
def test_several_failures_twice_and_permuted(field):
    n, size = 1100, 50
    mats, fs = {}, []
    for s in range(3):
        f = spread(n, -10, size, 20 + s)
        for i in ((), (1090, 64, 129), (5, 200))[s]:
            f[i] = 40 + i
        mats["F%d" % s] = column(field, f)
        fs.append(("F%d" % s, 0))
    a = run(field, mats, fs, -10, size, ("M", 2), n)
    assert a[1] == (1, 1, 64, 3 * n - 5), "side 1 before side 2 whatever the rows; within side 1 the smallest row"
    assert run(field, mats, fs, -10, size, ("M", 2), n, host=False) == a
    b = run(field, mats, fs, -10, size, ("M", 2), n, order=[2, 0, 1], host=False)
    assert b[0] == a[0] and b[1] == (1, 0, 5, 3 * n - 5), "the sides permuted: the same m, the same matched, side 2 is side 0 now"
    for path in (0, 1):
        assert run(field, mats, fs, -10, size, ("M", 2), n, path=path, host=False) == a


@pytest.mark.parametrize("field", list(FIELDS))
@pytest.mark.parametrize("size,n,lo", [(1, 5, -3), (256, 700, -128), (max(T, 1) + 1, (1 << 13) + 3, (1 << 63) - (1 << 14))])
def test_equivalence_with_lookup_mult_on_the_materialised_column(field, size, n, lo):
    q, ew = FIELDS[field], 1 if field == "gl" else 4
    f = spread(n, lo, size, 11)
    f[n // 2], f[n - 1] = lo + size, lo - 1                                      # two failures
    sel = [i % 5 for i in range(n)]                                              # every fifth row unselected; the last row is selected for these n
    F = to_dev(words(field, [[rref.pattern(v, q), s] for v, s in zip(f, sel)]))
    t = to_dev(words(field, [[v, POISON[field]] for v in rref.table_column(lo, size, n, q)]))
    out = to_dev(words(field, [[POISON[field]] * 2 for _ in range(n)]))
    want = pilcheck.lookup_mult_dev([(F, [0], (F, 1))], (t, [0]), (t, 1), n, field)
    got = pilcheck.range_mult_dev([(F, [0], (F, 1))], lo, size, (out, 0), n, field)
    assert got == want and got[0] == 1
    a = t.cpu().numpy().view(np.uint64).reshape(n, 2 * ew)[:, ew:]
    b = out.cpu().numpy().view(np.uint64).reshape(n, 2 * ew)[:, :ew]
    assert (a == b).all(), "m differs from lookup_mult's at rows %s" % np.argwhere((a != b).any(1)).ravel()[:8]
    ref_m, ref_rep = rref.multiplicities([[rref.pattern(v, q) for v in f]], lo, size, n, q, [sel])
    assert ref_rep == got and (b == words(field, [[rref.element(c, q)] for c in ref_m])[:, 0].reshape(n, ew)).all()


@pytest.mark.parametrize("field", list(FIELDS))
def test_m_as_a_spare_column_of_an_f_matrix(field):
    q, n, size, stride = FIELDS[field], 200, 30, 5
    f0, f1 = spread(n, 100, size, 1), spread(n, 100, size, 2)
    rows = [[POISON[field], rref.pattern(a, q), 1 + i % 2, rref.pattern(b, q), POISON[field] - i] for i, (a, b) in enumerate(zip(f0, f1))]
    first = run(field, {"B": rows}, [("B", 1), ("B", 3, ("B", 2))], 100, size, ("B", 4), n)
    assert first[1] == (0, NONE, NONE, 2 * n)
    assert run(field, {"B": rows}, [("B", 1), ("B", 3, ("B", 2))], 100, size, ("B", 0), n, row0=n - size)[1] == first[1]
    assert run(field, {"B": rows}, [("B", 1), ("B", 3, ("B", 2))], 100, size, ("M", 1), n) == first


def test_python_resident_forms_and_refusals_with_a_device():
    lib = _lib.load()
    n = 64
    d = to_dev(words("gl", [[i % 16, P - 3 + i % 5, 1, 7] for i in range(n)]))
    assert pilcheck.range_mult_dev([(d, [0]), (d, [1], (d, 2))], -3, 19, (d, 3), n) == (0, NONE, NONE, 2 * n)
    back = d.cpu().numpy().view(np.uint64).reshape(n, 4)[:, 3]
    assert back.sum() == 2 * n and back[0] == 13 and back[3] == 4 + 13 and not back[19:].any()
    assert pilcheck.range_mult_dev([(d, [0])], 0, 15, (d, 3), n, path=1)[:3] == (1, 0, 15)
    fr = to_dev(words("bn128", [[rref.pattern(i % 4, R), 1, 0] for i in range(n)]))
    assert pilcheck.range_mult_dev([(fr, [0], (fr, 1))], 0, 4, (fr, 2), n, field="bn128", row0=60) == (0, NONE, NONE, n)
    with pytest.raises(pil2gl.Pil2glError):
        pilcheck.range_mult_dev([(np.zeros((n, 4), np.uint64), [0])], 0, 4, (d, 3), n)
    with pytest.raises(pil2gl.Pil2glError, match="m overlaps"):
        pilcheck.range_mult_dev([(d, [0])], 0, 16, (d, 0), n)
    with pytest.raises(pil2gl.Pil2glError, match="row0"):
        pilcheck.range_mult_dev([(d, [0])], 0, 16, (d, 3), n, row0=49)
    need = pilcheck.range_mult_plan(n, 16)["scratchBytes"]
    work = torch.empty(need // 8, dtype=torch.int64, device="cuda")
    cols = np.array([0], np.uint64)
    side = _lib.TupleSide(d.data_ptr(), 4, cols.ctypes.data, None, 0, 0)
    rep = (C.c_uint64 * 4)()
    ok = [C.byref(side), 1, 0, 16, 0, d.data_ptr(), 4, 3, n, work.data_ptr(), need, rep, None]

    def call(**kw):
        args = list(ok)
        for key, v in kw.items():
            args[int(key[1:])] = v
        return lib.pil2gl_range_mult_dev(*args)
    assert call() == 0 and tuple(rep) == (0, NONE, NONE, n)
    assert call(a9=d.data_ptr() + 16) == -1 and b"overlaps" in lib.pil2gl_last_error()
    assert call(a10=need - 16) == -1 and b"scratch" in lib.pil2gl_last_error()
    assert call(a7=0) == -1 and b"m overlaps" in lib.pil2gl_last_error()
    assert call(a6=1) == -1 and b"stride" in lib.pil2gl_last_error()
    assert call(a1=9) == -1 and call(a3=0) == -1 and call(a4=n - 15) == -1 and call(a8=(1 << 28) + 1) == -1
    assert tuple(rep) == (0, NONE, NONE, 0), "a refused call leaves a clean report"
    assert call(a8=0, a9=None) == 0 and tuple(rep) == (0, NONE, NONE, 0)
