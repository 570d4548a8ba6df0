"""The connection check on the device (csrc/conn_check.hip) against the dictionary checker (tests/conn_check_ref.py): all three words of
the report, both fields, the resident and the host forms.  S comes from conn_pols_dev and the trace from gather_dev on one random sMap
(a signal that fills half the table, groups of a few cells, singletons, zero cells), made once per shape and never changed: every test
alters copies.  The shapes are the smallest at which the kernels can still go wrong: one column, fewer cells than a wave (16), cells
across the wave edge (flat 63 | 64), more than one workgroup and keys past their home slot (2^10 x 12), the widest row (64 columns)."""
import ctypes as C
import functools

import numpy as np
import pytest

import conn_check_ref as cref
import conn_pols_ref as ref
from conn_pols_ref import P, R

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from pil2gl import _lib, wtns  # noqa: E402
import pil2gl  # noqa: E402

FIELDS = {"gl": P, "bn128": R}
CLEAN = (cref.NONE, cref.NONE, 0)
HEAVY_VALUE = 12345                      # the heavy signal's value: small, so that value + p fits a Goldilocks word


def exec_of(flat, n_rows, n_cols, n_w, field):
    """an exec without additions whose sMap is the table: what prepare() needs"""
    e = {"field": field, "nWitness": n_w, "nAdds": 0, "nSMap": n_rows, "nCols": n_cols, "sMap": np.array(flat, np.uint64)}
    if field == "gl":
        e["adds"] = np.zeros(0, np.uint64)
    else:
        e["addsIdx"], e["addsCoef"] = np.zeros(0, np.uint64), np.zeros((0, 4), np.uint64)
    return e


def to_dev(words):
    return torch.from_numpy(np.array(words, np.uint64).view(np.int64)).cuda()      # a copy: the shared arrays are read-only


@functools.lru_cache(maxsize=None)
def base(field, N, n_cols):
    """sMap, witness, the device-made trace and S as host words (read-only) and as values, the constants"""
    q = FIELDS[field]
    rng = ref.rng(100 * N + n_cols + (q == R))
    cells = N * n_cols
    pool, single, flat = max(cells // 16, 1), 2 + max(cells // 16, 1), []
    for _ in range(cells):
        x = rng.random()
        if x < 0.5:
            flat.append(1)
        elif x < 0.6:
            flat.append(0)
        elif x < 0.8:
            flat.append(single)
            single += 1
        else:
            flat.append(2 + rng.randrange(pool))
    for c in (63, 64, cells - 1):                                              # the wave's and the grid's edges lie in the heavy group
        if 0 < c < cells:
            flat[c] = 1
    n_w = single
    wit = [0, HEAVY_VALUE] + [rng.randrange(q) for _ in range(n_w - 2)]
    w, ks = ref.root(q, N.bit_length() - 1), ref.get_ks(q, n_cols - 1)
    consts = ref.consts(w, ks, q)
    prep = wtns.prepare(exec_of(flat, N, n_cols, n_w, field))
    w_dev = to_dev(np.array(wit, np.uint64) if q == P else ref.fr_words(wit))
    trace = wtns.gather_dev(prep, w_dev)
    S = wtns.conn_pols_dev(prep, N, *consts)
    torch.cuda.synchronize()
    a_w, S_w = trace.cpu().numpy().view(np.uint64), S.cpu().numpy().view(np.uint64)
    a_w.setflags(write=False)
    S_w.setflags(write=False)
    groups = {}
    for c, s in enumerate(flat):
        if s:
            groups.setdefault(s, []).append(c)
    return {"field": field, "q": q, "N": N, "nCols": n_cols, "flat": flat, "groups": groups, "w": w, "ks": ks, "consts": consts, "a": a_w, "S": S_w}


def put(arr, c, value, q):
    """cell c of a copy of the words <- the field value"""
    flat = arr.reshape(-1) if q == P else arr.reshape(-1, 4)
    flat[c] = value % P if q == P else ref.fr_words([ref.to_mont(value)])[0]


def value_at(arr, c, q):
    return cref.values((arr.reshape(-1) if q == P else arr.reshape(-1, 4))[c:c + 1], q)[0]


def want(b, a_w, S_w, w=None, ks=None):
    w, ks = b["w"] if w is None else w, b["ks"] if ks is None else ks
    return cref.check(cref.values(a_w, b["q"]), cref.values(S_w, b["q"]), b["nCols"], b["N"], w, [1] + list(ks), b["q"])


def as_words(rep):
    return CLEAN if rep is None else (rep["cell"], cref.NONE if rep["partner"] is None else rep["partner"], rep["kind"])


def got(b, a_w, S_w, consts=None, **kw):
    return as_words(wtns.conn_check_dev(to_dev(a_w), to_dev(S_w), b["nCols"], b["N"], *(consts or b["consts"]), field=b["field"], **kw))


def succ(group, c):
    """the cell whose S names c: the next of its group, the first for the last"""
    return group[(group.index(c) + 1) % len(group)]


SHAPES = [("gl", 16, 1), ("bn128", 16, 1), ("gl", 64, 3), ("bn128", 64, 3), ("gl", 1024, 12), ("bn128", 1024, 12), ("gl", 64, 64), ("bn128", 64, 6)]


@pytest.mark.parametrize("field,N,n_cols", SHAPES)
def test_trace_and_connections_of_one_smap_are_clean(field, N, n_cols):
    b = base(field, N, n_cols)
    assert want(b, b["a"], b["S"]) == CLEAN, "the checker itself accepts the device-made pair"
    assert got(b, b["a"], b["S"]) == CLEAN
    assert len(b["groups"][1]) >= N * n_cols // 3 and any(len(g) == 1 for g in b["groups"].values()) and 0 in b["flat"]


def wide(b, arr, stride, offset, fill):
    """the columns as a range of a wider row-major matrix whose other columns hold `fill`"""
    tail = (4,) if b["q"] == R else ()
    m = np.full((b["N"], stride) + tail, fill, np.uint64)
    m[:, offset:offset + b["nCols"]] = arr
    return m


@pytest.mark.parametrize("field,N,n_cols", [("gl", 64, 3), ("bn128", 64, 3), ("gl", 1024, 12), ("bn128", 64, 6)])
def test_columns_of_wider_matrices(field, N, n_cols):
    b = base(field, N, n_cols)
    q = b["q"]
    a_w = b["a"].copy()
    args = (n_cols, N) + tuple(b["consts"])
    am, sm = wide(b, a_w, n_cols + 5, 2, 0x5A5A5A5A5A5A5A5A), wide(b, b["S"], n_cols + 3, 3, 7)
    assert wtns.conn_check_dev(to_dev(am), to_dev(sm), *args, field=field, a_stride=n_cols + 5, a_offset=2, s_stride=n_cols + 3, s_offset=3) is None
    x = b["groups"][1][2]
    put(a_w, x, value_at(a_w, x, q) + 1, q)                                      # one altered cell: the partner is read through the stride too
    expected = want(b, a_w, b["S"])
    assert expected[2] == 2
    am = wide(b, a_w, n_cols + 5, 2, 0x5A5A5A5A5A5A5A5A)
    assert as_words(wtns.conn_check_dev(to_dev(am), to_dev(sm), *args, field=field, a_stride=n_cols + 5, a_offset=2, s_stride=n_cols + 3, s_offset=3)) == expected
    # both in ONE matrix: a in columns [0, nCols), S in [nCols + 1, 2 nCols + 1)
    stride = 2 * n_cols + 1
    both = wide(b, a_w, stride, 0, 3)
    both[:, n_cols + 1:] = b["S"]
    t = to_dev(both)
    assert as_words(wtns.conn_check_dev(t, t, *args, field=field, a_stride=stride, a_offset=0, s_stride=stride, s_offset=n_cols + 1)) == expected


@pytest.mark.parametrize("field,N,n_cols", [("gl", 64, 3), ("bn128", 64, 3), ("gl", 1024, 12), ("bn128", 1024, 12)])
def test_one_altered_trace_cell(field, N, n_cols):
    b = base(field, N, n_cols)
    q, heavy = b["q"], b["groups"][1]
    some = next(g for s, g in sorted(b["groups"].items()) if s != 1 and len(g) >= 3)
    cells = N * n_cols
    assert {63, 64, cells - 1} <= set(heavy)
    for group, x in [(some, some[0]), (some, some[len(some) // 2]), (some, some[-1]), (heavy, 63), (heavy, 64), (heavy, cells - 1)]:
        a_w = b["a"].copy()
        put(a_w, x, value_at(a_w, x, q) + 1, q)
        expected = want(b, a_w, b["S"])
        first = min(x, succ(group, x))
        pred = group[group.index(first) - 1]
        assert expected == (first, pred, 2), "the checker: the smaller of the altered cell and the cell that names it"
        assert got(b, a_w, b["S"]) == expected, (x, expected)


@pytest.mark.parametrize("field", list(FIELDS))
def test_two_failures_in_different_workgroups_report_the_smaller(field):
    b = base(field, 1024, 12)
    q, heavy = b["q"], b["groups"][1]
    lo = next(c for c in heavy if c > 300)
    hi = next(c for c in heavy if c > 9000)
    assert hi // 256 != lo // 256 and hi // 128 != lo // 128                     # a workgroup walks 256 cells (Fr: 128) of a pass
    a_w = b["a"].copy()
    put(a_w, lo, 77, q)
    put(a_w, hi, 78, q)
    expected = want(b, a_w, b["S"])
    assert expected == (lo, heavy[heavy.index(lo) - 1], 2)
    assert got(b, a_w, b["S"]) == expected
    a_w = b["a"].copy()
    put(a_w, hi, 78, q)
    assert got(b, a_w, b["S"]) == want(b, a_w, b["S"]) == (hi, heavy[heavy.index(hi) - 1], 2)


@pytest.mark.parametrize("field,N,n_cols", [("gl", 64, 3), ("bn128", 64, 3), ("gl", 1024, 12), ("bn128", 64, 6)])
def test_an_s_value_that_names_no_cell(field, N, n_cols):
    b = base(field, N, n_cols)
    q = b["q"]
    ids = {pow(b["w"], i, q) * k % q for i in range(N) for k in [1] + b["ks"]}
    c = N * n_cols // 2 + 1
    g = next(g for g in range(3, 50) if all(v * g % q not in ids for v in ids))      # outside every coset: id g is no identity for any id
    for bad in (value_at(b["S"], c, q) * g % q, 0):
        assert bad not in ids
        S_w = b["S"].copy()
        put(S_w, c, bad, q)
        expected = want(b, b["a"], S_w)
        assert expected == (c, cref.NONE, 1)
        assert got(b, b["a"], S_w) == expected


def test_goldilocks_s_word_past_p_whose_residue_is_an_identity_passes():
    b = base("gl", 64, 3)
    S_w = b["S"].copy()
    flat = S_w.reshape(-1)
    c = int(np.flatnonzero(flat == 1)[0])                                        # id(0, 0) = 1 lies somewhere: S is a permutation of the ids
    flat[c] = 1 + P
    assert want(b, b["a"], S_w) == CLEAN and got(b, b["a"], S_w) == CLEAN


@pytest.mark.parametrize("field", list(FIELDS))
def test_identities_that_are_not_distinct(field):
    """ks'[2] = ks'[1] w^5: id(i, 2) = id(i + 5, 1), first met at row 5, column 1 = cell 16, whose twin is cell 2"""
    b = base(field, 64, 3)
    q = b["q"]
    ks = [b["ks"][0], b["ks"][0] * pow(b["w"], 5, q) % q]
    expected = want(b, b["a"], b["S"], ks=ks)
    assert expected == (16, 2, 3)
    assert got(b, b["a"], b["S"], consts=ref.consts(b["w"], ks, q)) == expected


@pytest.mark.parametrize("field", list(FIELDS))
def test_a_swap_between_signals_of_equal_value_is_clean(field):
    b = base(field, 64, 3)
    q = b["q"]
    c1, c2 = [g[0] for s, g in sorted(b["groups"].items()) if len(g) == 1][:2]
    a_w, S_w = b["a"].copy(), b["S"].copy()
    s1, s2 = value_at(S_w, c1, q), value_at(S_w, c2, q)
    put(S_w, c1, s2, q)
    put(S_w, c2, s1, q)
    assert want(b, a_w, S_w)[2] == 2, "swapped S over different values fails"
    assert got(b, a_w, S_w) == want(b, a_w, S_w)
    put(a_w, c2, value_at(a_w, c1, q), q)
    assert want(b, a_w, S_w) == CLEAN and got(b, a_w, S_w) == CLEAN


def test_trace_words_past_the_modulus_compare_as_their_residues():
    # Goldilocks: every second heavy cell holds value + p
    b = base("gl", 64, 3)
    a_w = b["a"].copy()
    flat = a_w.reshape(-1)
    for c in b["groups"][1][::2]:
        assert int(flat[c]) == HEAVY_VALUE
        flat[c] = HEAVY_VALUE + P
    assert want(b, a_w, b["S"]) == CLEAN and got(b, a_w, b["S"]) == CLEAN
    # Fr: the Montgomery pattern + r and + 4 r (r < 2^254: both fit 256 bits) in two cells of the heavy group
    b = base("bn128", 64, 3)
    a_w = b["a"].copy()
    rows = a_w.reshape(-1, 4)
    for c, k in ((b["groups"][1][1], 1), (b["groups"][1][3], 4)):
        pat = sum(int(rows[c][i]) << (64 * i) for i in range(4)) + k * R
        assert R <= pat < 1 << 256
        rows[c] = ref.fr_words([pat])[0]
    assert want(b, a_w, b["S"]) == CLEAN and got(b, a_w, b["S"]) == CLEAN
    x = b["groups"][1][3]
    rows[x] = ref.fr_words([sum(int(rows[x][i]) << (64 * i) for i in range(4)) - R + 1])[0]      # still past r, now another residue
    assert got(b, a_w, b["S"]) == want(b, a_w, b["S"]) and want(b, a_w, b["S"])[2] == 2


@pytest.mark.parametrize("field", list(FIELDS))
def test_some_key_lies_past_its_home_slot(field):
    """12288 keys in 32768 slots: without a collision the probing past the home slot would be untested"""
    b = base(field, 1024, 12)
    assert got(b, b["a"], b["S"]) == CLEAN
    assert wtns.conn_check_probe() >= 1
    small = base(field, 16, 1)
    assert got(small, small["a"], small["S"]) == CLEAN
    assert wtns.conn_check_probe() < 16, "the figure is the last call's"


@pytest.mark.parametrize("field,N,n_cols", [("gl", 64, 3), ("bn128", 64, 3), ("gl", 1024, 12), ("bn128", 64, 6)])
def test_host_forms_equal_the_resident_forms(field, N, n_cols):
    b = base(field, N, n_cols)
    q = b["q"]
    host = lambda a_w, S_w: as_words(wtns.conn_check(a_w, S_w, n_cols, N, *b["consts"], field=field))      # noqa: E731
    assert host(b["a"], b["S"]) == CLEAN
    a_w = b["a"].copy()
    x = b["groups"][1][len(b["groups"][1]) // 2]
    put(a_w, x, 5, q)
    assert host(a_w, b["S"]) == got(b, a_w, b["S"]) == want(b, a_w, b["S"])
    S_w = b["S"].copy()
    put(S_w, 1, 0, q)
    assert host(a_w, S_w) == got(b, a_w, S_w) == (1, cref.NONE, 1)


def test_refusals_with_a_device():
    lib = _lib.load()
    b = base("gl", 64, 3)
    a, S = to_dev(b["a"]), to_dev(b["S"])
    need = wtns.conn_check_plan(64, 3)["scratchBytes"]
    work = torch.empty(need // 8 + 64, dtype=torch.int64, device="cuda")
    w, ks1 = wtns._conn_consts(*b["consts"], 3, 1)
    rep = (C.c_uint64 * 3)()
    pw, pk = w.ctypes.data, ks1.ctypes.data
    ok = [a.data_ptr(), 3, 0, S.data_ptr(), 3, 0, 64, 3, pw, pk, work.data_ptr(), need, rep, None]

    def call(**kw):
        args = list(ok)
        for k, v in kw.items():
            args[int(k[1:])] = v
        return lib.pil2gl_conn_check_dev(*args)
    assert call() == 0 and tuple(rep) == CLEAN
    assert call(a10=a.data_ptr() + 16) == -1 and b"overlaps" in lib.pil2gl_last_error()
    assert call(a10=S.data_ptr() - need + 16) == -1 and b"overlaps" in lib.pil2gl_last_error()
    assert call(a11=need - 16) == -1 and b"scratch" in lib.pil2gl_last_error()
    assert call(a1=2) == -1 and call(a4=3, a5=1) == -1 and b"stride" in lib.pil2gl_last_error()
    assert call(a7=65) == -1 and b"columns" in lib.pil2gl_last_error()
    assert call(a6=48) == -1 and b"power of two" in lib.pil2gl_last_error()
    with pytest.raises(pil2gl.Pil2glError):
        wtns.conn_check_dev(a, S, 3, 48, *b["consts"])
    assert wtns.conn_check_dev(a, S, 0, 64, b["consts"][0], np.zeros(0, np.uint64)) is None
