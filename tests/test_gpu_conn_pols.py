"""The connection polynomials on the device (csrc/conn_pols.hip) against the checker's sequential swaps (tests/conn_pols_ref.py): exact
equality of words, both fields, the host and the resident forms.  The shapes are the smallest at which the kernels can still go wrong:
rows around the wave (63, 64, 65), more than one wave and workgroup of the grid-stride kernels (257, 1024 rows), more than one sort
workgroup (above 4096 cells), more than two digit passes (nW above 2^16), rows past the table (N twice the next power of two)."""
import json
import os

import numpy as np
import pytest

import conn_pols_ref as ref
import wtns_exec_ref as xref
from conn_pols_ref import P, R

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from pil2gl import wtns  # noqa: E402
from conftest import ROOT  # noqa: E402

FIELDS = {"gl": P, "bn128": R}
GOLDEN = os.path.join(ROOT, "tests", "golden", "conn_pols.json")


def next_pow2(n):
    return 1 << max(n - 1, 0).bit_length()


def exec_of(flat, n_rows, n_cols, n_w, field):
    """an exec without additions whose sMap is the table: what prepare() needs"""
    e = {"field": field, "nWitness": n_w, "nAdds": 0, "nSMap": n_rows, "nCols": n_cols, "sMap": np.array(flat, np.uint64)}
    if field == "gl":
        e["adds"] = np.zeros(0, np.uint64)
    else:
        e["addsIdx"], e["addsCoef"] = np.zeros(0, np.uint64), np.zeros((0, 4), np.uint64)
    return e


def expected(flat, n_rows, n_cols, N, field, w=None, ks=None):
    q = FIELDS[field]
    w = ref.root(q, N.bit_length() - 1) if w is None else w
    ks = ref.get_ks(q, n_cols - 1) if ks is None else ks
    return ref.words(ref.conn_pols(flat, n_rows, n_cols, N, w, ks, q), q), ref.consts(w, ks, q)


def resident(flat, n_rows, n_cols, n_w, N, field, consts, **kw):
    prep = wtns.prepare(exec_of(flat, n_rows, n_cols, n_w, field))
    out = wtns.conn_pols_dev(prep, N, *consts, **kw)
    torch.cuda.synchronize()
    return out


def host_of(t):
    return t.cpu().numpy().view(np.uint64)


def mixed_table(rng, n_rows, n_cols, n_w, zeros=0.2):
    """a few heavy signals (long groups), many light ones, zeros, 1 and nW - 1 among them"""
    heavy = [1, n_w - 1] + [rng.randrange(1, n_w) for _ in range(3)]
    flat = []
    for _ in range(n_rows * n_cols):
        x = rng.random()
        flat.append(0 if x < zeros else rng.choice(heavy) if x < 0.6 else rng.randrange(1, n_w))
    return flat


def setup_shape(flat, n_rows, n_cols, N):
    """the setups' own sMap: nCols arrays of N u32"""
    a = np.zeros((n_cols, N), np.uint32)
    a[:, :n_rows] = np.array(flat, np.uint32).reshape(n_rows, n_cols).T
    return a


@pytest.mark.parametrize("n_rows", [1, 63, 64, 65, 257, 1024])
@pytest.mark.parametrize("n_cols", [1, 3, 12, 18])
def test_shapes_against_the_sequential_swaps(n_cols, n_rows):
    rng = ref.rng(1000 * n_cols + n_rows)
    n_w = max(n_rows * n_cols // 3, 3)
    flat = mixed_table(rng, n_rows, n_cols, n_w)
    N = next_pow2(n_rows)
    for field in FIELDS:
        want, consts = expected(flat, n_rows, n_cols, N, field)
        assert np.array_equal(host_of(resident(flat, n_rows, n_cols, n_w, N, field, consts)), want), (field, "resident, N = %d" % N)
        want, consts = expected(flat, n_rows, n_cols, 2 * N, field)                             # rows past the table
        got = wtns.conn_pols(setup_shape(flat, n_rows, n_cols, 2 * N), n_cols, 2 * N, *consts, field=field, n_w=n_w)
        assert np.array_equal(got, want), (field, "host, setup-shaped sMap, N = %d" % (2 * N))


@pytest.mark.parametrize("field", list(FIELDS))
def test_three_digit_passes_and_groups_across_workgroups(field):
    """12 x 6000 = 72000 cells (18 sort workgroups), nW = 70001: the plan takes three passes; the heavy signals' groups span every workgroup"""
    n_rows, n_cols, n_w, N = 6000, 12, 70001, 8192
    assert wtns.conn_plan(n_rows, n_cols, n_w, N, field)["passes"] == 3
    flat = mixed_table(ref.rng(7), n_rows, n_cols, n_w, zeros=0.05)
    assert sum(1 for s in flat if s) > 1 << 16 and max(flat) == n_w - 1 and len(set(flat)) > 20000
    want, consts = expected(flat, n_rows, n_cols, N, field)
    assert np.array_equal(host_of(resident(flat, n_rows, n_cols, n_w, N, field, consts)), want)
    assert np.array_equal(wtns.conn_pols(np.array(flat, np.uint64), n_cols, N, *consts, field=field, n_w=n_w), want), "the exec-shaped host form"


def structures():
    n_rows, n_cols = 400, 12                                                                     # 4800 cells: two sort workgroups
    n = n_rows * n_cols
    yield "one signal in every cell", [5] * n, n_rows, n_cols, 9
    yield "one signal in every second cell, the rest singletons", [7 if c % 2 == 0 else 100 + c for c in range(n)], n_rows, n_cols, 100 + n
    yield "all zeros", [0] * n, n_rows, n_cols, 9
    yield "signals 1 and nW - 1 only", [(1, 299)[(c * c + c // 7) % 2] for c in range(n)], n_rows, n_cols, 300
    yield "a group from the first cell to the last", [3] + [0 if c % 3 else 10 + c % 50 for c in range(1, n - 1)] + [3], n_rows, n_cols, 70
    yield "two signals that differ in a high digit only", [(5, 5 + (1 << 16), 0, 5 + (1 << 17))[(c * 7 + c // 11) % 4] for c in range(n)], n_rows, n_cols, (1 << 18)
    yield "a signal past nW's low digits next to its low twin", [(2, 2 + (1 << 8), 2 + (1 << 16))[c % 3] for c in range(70)], 70, 1, (1 << 16) + 3


@pytest.mark.parametrize("case", list(structures()), ids=lambda c: c[0])
def test_group_structures(case):
    _, flat, n_rows, n_cols, n_w = case
    N = 2 * next_pow2(n_rows)
    for field in FIELDS:
        want, consts = expected(flat, n_rows, n_cols, N, field)
        assert np.array_equal(host_of(resident(flat, n_rows, n_cols, n_w, N, field, consts)), want), field


def test_constants_at_the_fields_edges():
    """w and ks the library is given are multiplied as they are; words past the modulus count as their value mod it"""
    rng = ref.rng(3)
    n_rows, n_cols, N = 37, 5, 64
    flat = mixed_table(rng, n_rows, n_cols, 40)
    # Goldilocks: p - 1, and representatives in [p, 2^64)
    w_word, ks_words = P + 2, [P - 1, (1 << 64) - 1, 1, 0]
    want = ref.gl_words(ref.conn_pols(flat, n_rows, n_cols, N, w_word % P, [k % P for k in ks_words], P))
    got = wtns.conn_pols(np.array(flat, np.uint64), n_cols, N, np.array([w_word], np.uint64), np.array(ks_words, np.uint64), n_w=40)
    assert np.array_equal(got, want)
    want = ref.gl_words(ref.conn_pols(flat, n_rows, n_cols, N, P - 1, [P - 1, 1 << 32, (1 << 32) - 1, P - 2], P))
    got = wtns.conn_pols(np.array(flat, np.uint64), n_cols, N, np.array([P - 1], np.uint64), np.array([P - 1, 1 << 32, (1 << 32) - 1, P - 2], np.uint64), n_w=40)
    assert np.array_equal(got, want)
    # Fr: Montgomery words at the edges -- r - 1, 2^256 - 1 (a pattern past r), 1, 0, values just below r's top limb
    inv_mont = pow(ref.MONT, -1, R)
    pats = [R - 1, (1 << 256) - 1, 1, 0, int("2" + "f" * 63, 16), sum(0x80000000 << (32 * i) for i in range(7))]
    for w_pat, ks_pats in ((pats[0], pats[1:5]), (pats[4], [pats[5], pats[0], pats[1], R - 2])):
        val = lambda x: x % R * inv_mont % R                                                       # noqa: E731  the value Montgomery words stand for
        want = ref.fr_mont_words(ref.conn_pols(flat, n_rows, n_cols, N, val(w_pat), [val(k) for k in ks_pats], R))
        got = wtns.conn_pols(np.array(flat, np.uint64), n_cols, N, ref.fr_words([w_pat]), ref.fr_words(ks_pats), field="bn128", n_w=40)
        assert np.array_equal(got, want)


@pytest.mark.parametrize("field", list(FIELDS))
def test_columns_of_a_wider_matrix_and_the_host_form_agree(field):
    rng = ref.rng(11)
    n_rows, n_cols, n_w, N = 300, 7, 500, 512
    flat = mixed_table(rng, n_rows, n_cols, n_w)
    want, consts = expected(flat, n_rows, n_cols, N, field)
    host = wtns.conn_pols(np.array(flat, np.uint64), n_cols, N, *consts, field=field, n_w=n_w)
    assert np.array_equal(host, want)
    stride, offset, sentinel = n_cols + 5, 2, 0x5A5A5A5A5A5A5A5A
    tail = (4,) if field == "bn128" else ()
    dst = torch.full((N, stride) + tail, sentinel, dtype=torch.int64, device="cuda")
    out = resident(flat, n_rows, n_cols, n_w, N, field, consts, dst=dst, dst_stride=stride, dst_offset=offset)
    assert out is dst
    got = host_of(dst)
    assert np.array_equal(got[:, offset:offset + n_cols], host), "the resident form in place equals the host form"
    assert (got[:, :offset] == sentinel).all() and (got[:, offset + n_cols:] == sentinel).all(), "the matrix's other columns survive"


@pytest.mark.parametrize("field", list(FIELDS))
def test_check_reports_the_first_index_that_names_no_signal(field):
    """the table stays inside its allocation; only the VALUES of two cells are at or past nW, and those cells come out as identity"""
    rng = ref.rng(13)
    n_rows, n_cols, n_w, N = 130, 6, 90, 256
    flat = mixed_table(rng, n_rows, n_cols, n_w)
    prep = wtns.prepare(exec_of(flat, n_rows, n_cols, n_w, field))
    want, consts = expected(flat, n_rows, n_cols, N, field)
    out, bad = wtns.conn_pols_dev(prep, N, *consts, check=True)
    assert bad is None and np.array_equal(host_of(out), want)
    broken = list(flat)
    broken[401], broken[77] = n_w, 0xFFFFFFFF
    table = wtns._to_dev(np.array(broken, np.uint32))
    out, bad = wtns.conn_pols_dev(prep, N, *consts, check=True, s_map=table)
    assert bad == 77
    zeroed = list(broken)
    zeroed[401] = zeroed[77] = 0
    want, _ = expected(zeroed, n_rows, n_cols, N, field)
    assert np.array_equal(host_of(out), want)
    out = wtns.conn_pols_dev(prep, N, *consts, s_map=table)                                      # unchecked: the same values, nothing reported
    torch.cuda.synchronize()
    assert np.array_equal(host_of(out), want)


def test_golden_through_the_device():
    if not os.path.exists(GOLDEN):
        pytest.skip("tests/golden/conn_pols.json is not shipped: node could not load the reference's polutils.js / f3g.js when the change was made")
    for c in json.load(open(GOLDEN))["cases"]:
        n_rows, n_cols, N = c["nRows"], c["nCols"], 1 << c["nBits"]
        s_map = np.zeros((n_cols, N), np.uint32)
        s_map[:, :n_rows] = np.array(c["sMap"], np.uint32)
        want = np.array([[int(c["S"][j][i]) for j in range(n_cols)] for i in range(N)], np.uint64)
        consts = (np.array([int(c["w"])], np.uint64), np.array([int(k) for k in c["ks"]], np.uint64))
        assert np.array_equal(wtns.conn_pols(s_map, n_cols, N, *consts), want), c["name"]
        flat = [int(s_map[j][i]) for i in range(n_rows) for j in range(n_cols)]
        assert np.array_equal(host_of(resident(flat, n_rows, n_cols, max(flat) + 1, N, "gl", consts)), want), c["name"]


@pytest.mark.parametrize("field", list(FIELDS))
def test_trace_and_connections_from_one_resident_table_satisfy_the_copy_constraint(field):
    """prepare once; exec_dev fills the trace and conn_pols_dev the S columns from the same sMap.  The permutation argument holds: the
    multiset of (value, identity) pairs equals that of (value, S) pairs, and every cell's value equals the value at the cell S points to."""
    q = FIELDS[field]
    rng = xref.rng(21)
    n_rows, n_cols, N = 200, 12, 256
    w = [rng.randrange(q) for _ in range(30)]
    adds = xref.random_dag(rng, len(w), 40, q)
    n_w = len(w) + len(adds)
    flat = [rng.choice((0, 1 + rng.randrange(n_w - 1))) for _ in range(n_rows * n_cols)]
    e = exec_of(flat, n_rows, n_cols, len(w), field)
    e["nAdds"] = len(adds)
    if field == "gl":
        e["adds"] = np.array([x for r in adds for x in r], np.uint64)
        w_dev = torch.from_numpy(np.array(w + [0] * len(adds), np.uint64).view(np.int64)).cuda()
    else:
        e["addsIdx"] = np.array([x for a, b, _, _ in adds for x in (a, b)], np.uint64)
        e["addsCoef"] = xref.fr_words([xref.to_mont(c) for _, _, ca, cb in adds for c in (ca, cb)])
        w_dev = torch.from_numpy(xref.fr_words(w + [0] * len(adds)).view(np.int64)).cuda()
    prep = wtns.prepare(e)
    assert prep["nW"] == n_w
    trace = wtns.exec_dev(prep, w_dev)
    root, ks = ref.root(q, 8), ref.get_ks(q, n_cols - 1)
    S = wtns.conn_pols_dev(prep, N, *ref.consts(root, ks, q))
    torch.cuda.synchronize()
    cell = lambda a, c: tuple(int(x) for x in np.atleast_1d(a[c // n_cols, c % n_cols]))          # noqa: E731
    trace, S = host_of(trace), host_of(S)
    ident = ref.words(ref.conn_pols([], 0, n_cols, N, root, ks, q), q)                           # no connections: the identity columns
    cells = range(n_rows * n_cols)
    where = {cell(ident, c): c for c in range(N * n_cols)}
    assert len(where) == N * n_cols, "the identity values are distinct"
    assert {(cell(trace, c), cell(ident, c)) for c in cells} == {(cell(trace, c), cell(S, c)) for c in cells}
    moved = 0
    for c in cells:
        src = where[cell(S, c)]
        assert src < n_rows * n_cols and cell(trace, src) == cell(trace, c), c
        moved += src != c
    assert moved > 1000, "most cells of this table are connected"
    for c in range(n_rows * n_cols, N * n_cols):
        assert where[cell(S, c)] == c
