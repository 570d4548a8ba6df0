"""The plookup argument on the device against the integer checker (tests/plookup_ref.py), bit-exact, both fields.  Every product case goes
through run(): f, t, the selectors, h1, h2 and z as columns of ONE strided matrix; the resident form on a non-default stream, twice, into a
dirtied column, with guard words behind the matrix; the host form on a copy; the checker on the same bit patterns; and the promise --
gprod_dev / bn128_gprod_dev on the checker's materialised num and den columns, uploaded, give the same words.  Every word of the matrix
outside z's column and the guard words must come back unchanged.  Elements are bit patterns: the checker and the device both take them
mod the modulus (Goldilocks words in [p, 2^64) are drawn on purpose); over Fr a pattern X stands for the value X / 2^256 mod r.  Shapes
are the smallest at which the kernels can still go wrong: the lane edge (8 rows) and the block edge (2048 rows) of the Goldilocks first
pass, where the ninth row a lane reads changes its source, n = 1 (its own neighbour), k = 1, 3, 16 and unequal k."""
import random

import numpy as np
import pytest

import plookup_ref as pref
import logup_sum_ref as lref
import bn128_hints_ref as bref
import conn_pols_ref as cref
from hints_ref import P

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from pil2gl import pilcheck, bn128  # noqa: E402
import pil2gl  # noqa: E402

R, MONT = bref.R, bref.MONT
GUARD = 0x6B6B6B6B6B6B6B6B
FIELDS = ("gl", "bn128")
EDGES = (1, 2, 7, 8, 9, 2047, 2048, 2049, 4097)
SHAPES = ((1, 1), (3, 3), (2, 5), (16, 16))


# ---- bit patterns <-> the library's words <-> the checker's values ----
def rand_pat(rng, field):
    """a bit pattern of one element; a Goldilocks word lies in [p, 2^64) one time in four, an Fr pattern anywhere below 2^256"""
    if field == "gl":
        return rng.randrange(P, 1 << 64) if rng.random() < 0.25 else rng.randrange(P)
    return rng.randrange(1 << 256) if rng.random() < 0.25 else rng.randrange(R)


def value(field, pat):
    return pat % P if field == "gl" else bref.unmont(pat % R)


def pat_of(field, v):
    """the canonical pattern of a base value"""
    return v % P if field == "gl" else v % R * MONT % R


def words(field, rows):
    if field == "gl":
        return np.array(rows, np.uint64).reshape(len(rows), -1)
    return cref.fr_words([v for row in rows for v in row]).reshape(len(rows), -1, 4)


def rand_chal(rng, field, raw=True):
    """a challenge as (the words the call takes, the checker's value); raw: not canonical now and then"""
    if field == "gl":
        w = [rng.randrange(P, 1 << 64) if raw and rng.random() < 0.3 else rng.randrange(P) for _ in range(3)]
        return w, tuple(x % P for x in w)
    pat = rng.randrange(1 << 256) if raw and rng.random() < 0.3 else rng.randrange(R)
    return [int(x) for x in cref.fr_words([pat])[0]], value(field, pat)


def ext_words(field, vals):
    """field elements (triples / integers) as the words a column holds: (n, 3) or (n, 4)"""
    if field == "gl":
        return np.array(vals, np.uint64).reshape(len(vals), 3)
    return cref.fr_words([v * MONT % R for v in vals])


def to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


_STREAM = []


def side_stream():
    if not _STREAM:
        _STREAM.append(torch.cuda.Stream())
    return _STREAM[0]


def gprod_on_columns(field, num, den):
    """the promise's other side: the parent's entries on two ready extension columns"""
    if field == "gl":
        d_num, d_den = to_dev(np.array(num, np.uint64)), to_dev(np.array(den, np.uint64))
        z = pil2gl.calculateZ(d_num.reshape(-1), d_den.reshape(-1), 3, 3)
        torch.cuda.synchronize()
        return z.cpu().numpy().view(np.uint64).reshape(len(num), 3)
    d_num, d_den = to_dev(bref.mont_words(num)), to_dev(bref.mont_words(den))
    z = bn128.gprod(d_num, d_den, len(num))
    torch.cuda.synchronize()
    return z.cpu().numpy().view(np.uint64).reshape(len(num), 4)


class Layout:
    """the columns of the one matrix: f, selF, t, selT, h1, h2, z, and two spare ones that nothing touches (one of them first)"""

    def __init__(self, field, k_f, k_t, h_dim):
        self.hw = h_dim if field == "gl" else 1
        self.zw = 3 if field == "gl" else 1
        at = 1
        self.f = list(range(at, at + k_f))[::-1]; at += k_f                     # f's columns in falling order: the order is the call's, not the matrix's
        self.sel_f = at; at += 1
        self.t = list(range(at, at + k_t)); at += k_t
        self.sel_t = at; at += 1
        self.h1 = at; at += self.hw
        self.h2 = at; at += self.hw
        self.z = at; at += self.zw
        self.stride = at + 1


def build(rng, field, n, k_f, k_t, h_dim, wild):
    """a random matrix of bit patterns; selectors 0 / 1, or with `wild` any pattern now and then"""
    L = Layout(field, k_f, k_t, h_dim)
    rows = [[rand_pat(rng, field) for _ in range(L.stride)] for _ in range(n)]
    for row in rows:
        for c in (L.sel_f, L.sel_t):
            row[c] = rand_pat(rng, field) if wild and rng.random() < 0.5 else pat_of(field, rng.randrange(2))
    return L, rows


def sides_of(field, L, rows, sel_f, sel_t):
    f = ([[value(field, r[c]) for c in L.f] for r in rows], [value(field, r[L.sel_f]) for r in rows] if sel_f else None)
    t = ([[value(field, r[c]) for c in L.t] for r in rows], [value(field, r[L.sel_t]) for r in rows] if sel_t else None)
    return f, t


def h_of(field, L, rows, col):
    if field == "gl" and L.hw == 3:
        return [tuple(value(field, r[col + w]) for w in range(3)) for r in rows]
    return [value(field, r[col]) for r in rows]


def run(field, L, rows, sel_f, sel_t, h_dim, chs, check_host=True):
    """-> (z, num, den) as the checker gives them, which the resident form (twice), the host form and gprod on num and den gave too"""
    n = len(rows)
    host = words(field, rows)
    f, t = sides_of(field, L, rows, sel_f, sel_t)
    h1, h2 = h_of(field, L, rows, L.h1), h_of(field, L, rows, L.h2)
    vals = [c[1] for c in chs]
    num, den = pref.num_den(field, f, t, h1, h2, *vals)
    want = pref.z_of(field, num, den)
    expect = host.copy()
    expect[:n, L.z:L.z + L.zw] = ext_words(field, want).reshape((n, L.zw) + expect.shape[2:])

    def call(fn, m):
        fn((m, L.f, (m, L.sel_f) if sel_f else None), (m, L.t, (m, L.sel_t) if sel_t else None), (m, L.h1), (m, L.h2), *[c[0] for c in chs], (m, L.z), n,
           field=field, h_dim=h_dim)
    held = torch.full((host.size + 16,), GUARD, dtype=torch.int64, device="cuda")
    fresh = to_dev(host).reshape(-1)
    m = held[:host.size].view(host.shape)
    stream = side_stream()
    got = []
    for _ in range(2):
        held[:host.size] = fresh
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            call(pilcheck.plookup_prod_dev, m)
        stream.synchronize()
        got.append(held.cpu().numpy().view(np.uint64))
    assert (got[0] == got[1]).all(), "two calls give identical words"
    assert (got[0][host.size:] == np.uint64(GUARD)).all(), "the guard words behind the matrix"
    bad = np.argwhere(got[0][:host.size].reshape(host.shape) != expect)
    assert bad.size == 0, "the resident form: z is the checker's and every other word as it was; first difference at %s" % (bad[0],)
    if check_host:
        h = host.copy()
        call(pilcheck.plookup_prod, h)
        assert (h == expect).all(), "the host form gives the same words"
    assert (gprod_on_columns(field, num, den) == ext_words(field, want)).all(), "gprod_dev on the materialised num and den gives other words"
    return want, num, den


def four_challenges(rng, field, raw=True):
    return [rand_chal(rng, field, raw) for _ in range(4)]


@pytest.mark.parametrize("field,n", [(f, n) for f in FIELDS for n in EDGES])
def test_row_edges(field, n):
    """the lane edge and the block edge, the shape and the selectors cycling with n; z[0] = 1 whatever row 0 holds"""
    i = EDGES.index(n)
    rng = random.Random(1000 + n)
    k_f, k_t = SHAPES[i % 4]
    sel_f, sel_t = bool(i & 1), bool(i & 2)
    h_dim = 3 if field == "gl" else 1
    L, rows = build(rng, field, n, k_f, k_t, h_dim, wild=i % 3 == 0)
    z, _, _ = run(field, L, rows, sel_f, sel_t, h_dim, four_challenges(rng, field), check_host=n <= 2049)
    assert z[0] == lref.FIELDS[field].one


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("k_f,k_t", SHAPES)
def test_shapes_and_selectors(field, k_f, k_t):
    """every selector combination at a size with a partial lane and a second block; selector values outside {0, 1}"""
    rng = random.Random(16 * k_f + k_t)
    n = 2049 if (k_f, k_t) == (3, 3) else 9
    h_dim = 3 if field == "gl" else 1
    L, rows = build(rng, field, n, k_f, k_t, h_dim, wild=True)
    for sel_f, sel_t in ((False, False), (True, False), (False, True), (True, True)):
        run(field, L, rows, sel_f, sel_t, h_dim, four_challenges(rng, field), check_host=sel_f and sel_t)


@pytest.mark.parametrize("n", [1, 8, 9, 2049])
def test_base_field_h_over_goldilocks(n):
    """hDim = 1: the range-check shape (k = 1, no selT), and the product taking hDim = 1 as given with k = 3"""
    rng = random.Random(n)
    L, rows = build(rng, "gl", n, 1, 1, 1, wild=True)
    run("gl", L, rows, True, False, 1, four_challenges(rng, "gl"))
    run("gl", L, rows, False, False, 1, four_challenges(rng, "gl"), check_host=False)
    L, rows = build(rng, "gl", n, 3, 3, 1, wild=False)
    run("gl", L, rows, True, True, 1, four_challenges(rng, "gl"), check_host=False)


def plant_zero_den(field, L, rows, i, which, chs):
    """make one factor of den[i] zero: h1[i] = -(delta h2[i] + g) (which = 0) or h2[i] = -(delta h1[i+1] + g) (which = 1)"""
    F = lref.FIELDS[field]
    n = len(rows)
    gamma, delta = chs[2][1], chs[3][1]
    g = F.mul(gamma, F.add(F.one, delta))
    other = h_of(field, L, rows, L.h2)[i] if which == 0 else h_of(field, L, rows, L.h1)[(i + 1) % n]
    v = F.add(F.mul(delta, pref.elem(field, other)), g)
    v = tuple((P - x) % P for x in v) if field == "gl" else (R - v) % R
    col = L.h1 if which == 0 else L.h2
    if field == "gl":
        rows[i][col:col + 3] = list(v)
    else:
        rows[i][col] = v * MONT % R


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("n", [9, 2049])
def test_zero_den_factor(field, n):
    """a zero den factor at row 0, a middle row and row n - 2: every z up to it as without it, every later z 0"""
    F = lref.FIELDS[field]
    h_dim = 3 if field == "gl" else 1
    for at, which in ((0, 0), (n // 2, 1), (n - 2, 0)):
        rng = random.Random(n + at)
        L, rows = build(rng, field, n, 2, 3, h_dim, wild=False)
        chs = four_challenges(rng, field)
        clean, _, _ = run(field, L, rows, True, True, h_dim, chs, check_host=False)
        plant_zero_den(field, L, rows, at, which, chs)
        z, _, den = run(field, L, rows, True, True, h_dim, chs, check_host=at == 0)
        assert den[at] == F.zero
        # planting h1[at] also changes den[at - 1] (its h1'), so z is compared up to at - 1 only in that case
        same = at if which == 1 else max(at - 1, 0)
        assert z[:same + 1] == clean[:same + 1] and all(v == F.zero for v in z[at + 1:]) and all(v != F.zero for v in z[:at + 1])


@pytest.mark.parametrize("field", FIELDS)
def test_zero_num_factor(field):
    """F[i] + gamma = 0 is plain arithmetic: z is 0 from row i + 1 on, through the ordinary product"""
    F = lref.FIELDS[field]
    rng = random.Random(5)
    n, at = 17, 6
    h_dim = 3 if field == "gl" else 1
    L, rows = build(rng, field, n, 1, 1, h_dim, wild=False)
    chs = four_challenges(rng, field)
    g0 = rng.randrange(P if field == "gl" else R)                                # a base-valued gamma, so that a base f can cancel it
    if field == "gl":
        chs[2] = ([g0, 0, 0], (g0, 0, 0))
    else:
        chs[2] = ([int(x) for x in cref.fr_words([g0 * MONT % R])[0]], g0)
    rows[at][L.f[0]] = pat_of(field, -g0)
    z, num, _ = run(field, L, rows, False, True, h_dim, chs)
    assert num[at] == F.zero and z[at] != F.zero and all(v == F.zero for v in z[at + 1:])


def valid_matrix(rng, field, n, k_f, k_t, sel_f, sel_t, h_dim, chs):
    """a lookup that holds, laid out in the one matrix with h1 and h2 from the checker's h1h2"""
    f, t, h1, h2, _, _ = pref.valid_lookup(rng, field, n, k_f, k_t, sel_f, sel_t, alpha=chs[0][1], beta=chs[1][1])
    L, rows = build(rng, field, n, k_f, k_t, h_dim, wild=False)
    for i, row in enumerate(rows):
        for j, c in enumerate(L.f):
            row[c] = pat_of(field, f[0][i][j])
        for j, c in enumerate(L.t):
            row[c] = pat_of(field, t[0][i][j])
        row[L.sel_f] = pat_of(field, f[1][i] if sel_f else 0)
        row[L.sel_t] = pat_of(field, t[1][i] if sel_t else 0)
        for col, h in ((L.h1, h1), (L.h2, h2)):
            if field == "gl":
                row[col:col + L.hw] = list(h[i])[:L.hw]
            else:
                row[col] = h[i] * MONT % R
    return L, rows, (f, t, h1, h2)


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("n", [1, 2, 9, 100, 2049])
def test_valid_lookups_close(field, n):
    """for a lookup that holds, the device's z[n-1] times the checker's last ratio is 1: the only place the neighbour of row n - 1 shows"""
    F = lref.FIELDS[field]
    for k_f, k_t, sel_f, sel_t, h_dim in ((1, 1, False, False, 1), (3, 3, True, True, 3), (2, 5, True, False, 3)):
        if n == 2049 and k_f != 3:
            continue
        rng = random.Random(7 * n + k_t)
        h_dim = h_dim if field == "gl" else 1
        chs = four_challenges(rng, field, raw=False)
        L, rows, _ = valid_matrix(rng, field, n, k_f, k_t, sel_f, sel_t, h_dim, chs)
        z, num, den = run(field, L, rows, sel_f, sel_t, h_dim, chs, check_host=False)
        assert F.mul(z[-1], pref.ratios(field, num, den)[-1]) == F.one, "the product closes"


@pytest.mark.parametrize("field", FIELDS)
def test_fold_and_h1h2(field):
    """the fold word for word against the checker's F and T, resident (into the matrix and dense) and host; then plookup_h1h2_dev against the
    h1h2 checker; a value of f that is not in t comes back as the field's h1h2 reports it"""
    rng = random.Random(21)
    for n, k_f, k_t, sel_f, sel_t, h_dim in ((9, 1, 1, True, False, 1), (2049, 3, 3, True, True, 3), (100, 2, 5, True, False, 3), (9, 16, 16, False, True, 3)):
        h_dim = h_dim if field == "gl" else 1
        chs = four_challenges(rng, field)
        L, rows, (f, t, h1, h2) = valid_matrix(rng, field, n, k_f, k_t, sel_f, sel_t, h_dim, chs)
        for row in rows:                                                         # the selectors' field values: any pattern on an unused one
            if not sel_f:
                row[L.sel_f] = rand_pat(rng, field)
        host = words(field, rows)
        Fx, T = pref.fold(field, f, t, chs[0][1], chs[1][1])
        expect = host.copy()
        hw = L.hw
        for col, v in ((L.h1, Fx), (L.h2, T)):                                   # the fold writes where h1 and h2 will lie
            expect[:n, col:col + hw] = ext_words(field, v).reshape((n, -1) + expect.shape[2:])[:, :hw]
        spec = lambda m: ((m, L.f, (m, L.sel_f) if sel_f else None), (m, L.t, (m, L.sel_t) if sel_t else None))   # noqa: E731
        d = to_dev(host)
        with torch.cuda.stream(side_stream()):
            pilcheck.plookup_fold_dev(*spec(d), chs[0][0], chs[1][0], (d, L.h1), (d, L.h2), n, field=field, h_dim=h_dim)
        side_stream().synchronize()
        assert (d.cpu().numpy().view(np.uint64) == expect).all(), "the resident fold: F and T are the checker's, every other word as it was"
        h = host.copy()
        pilcheck.plookup_fold(*spec(h), chs[0][0], chs[1][0], (h, L.h1), (h, L.h2), n, field=field, h_dim=h_dim)
        assert (h == expect).all(), "the host fold gives the same words"
        d = to_dev(host)
        g1, g2 = pilcheck.plookup_h1h2_dev(*spec(d), chs[0][0], chs[1][0], n, field=field, h_dim=h_dim)
        torch.cuda.synchronize()
        for got, want in ((g1, h1), (g2, h2)):
            w = ext_words(field, want)
            w = w[:, :hw] if field == "gl" else w
            assert (got.cpu().numpy().view(np.uint64).reshape(w.shape) == w).all(), "h1 and h2 are the h1h2 checker's on the folded columns"
        if n == 9:
            a1, a2 = pilcheck.plookup_h1h2(*spec(host.copy()), chs[0][0], chs[1][0], n, field=field, h_dim=h_dim)
            assert (np.asarray(a1).reshape(-1) == g1.cpu().numpy().view(np.uint64).reshape(-1)).all(), "the host composition gives the same words"
            assert (np.asarray(a2).reshape(-1) == g2.cpu().numpy().view(np.uint64).reshape(-1)).all()
    # a missing value: row 5 of f selected and set to a tuple no t row holds
    n = 9
    chs = four_challenges(rng, field)
    h_dim = 3 if field == "gl" else 1
    L, rows, (f, t, _, _) = valid_matrix(rng, field, n, 2, 2, True, False, h_dim, chs)
    rows[5][L.sel_f] = pat_of(field, 1)
    rows[5][L.f[0]] = pat_of(field, max(r[0] for r in t[0]) + 1)
    d = to_dev(words(field, rows))
    with pytest.raises(pil2gl.Pil2glError, match="Number not included: w:5"):
        pilcheck.plookup_h1h2_dev((d, L.f, (d, L.sel_f)), (d, L.t), chs[0][0], chs[1][0], n, field=field, h_dim=h_dim)


@pytest.mark.parametrize("field", FIELDS)
def test_the_resident_product_only_enqueues(field):
    """the plan's launch count; and the call returns before its work is done: after one warm-up (the working slots grow with a device
    synchronise on first use), four calls over 2^22 (Goldilocks) / 2^20 (Fr) rows -- a millisecond of device work each -- are sent on a side
    stream and an event recorded behind them has not completed when the last call returns; nothing is compared here but that and the two
    runs' words"""
    n = 1 << (22 if field == "gl" else 20)
    plan = pilcheck.plookup_plan(n, 3, 3, field)
    assert plan["launches"] == (3 if field == "gl" else 4 * plan["depth"] - 1)
    g = torch.Generator(device="cuda").manual_seed(43)
    mat = torch.randint(0, 1 << 62, (n, 8) if field == "gl" else (n, 8, 4), dtype=torch.int64, device="cuda", generator=g)     # below both moduli
    out = torch.zeros((n, 3) if field == "gl" else (n, 1, 4), dtype=torch.int64, device="cuda")
    c = rand_chal(random.Random(3), field)[0]
    args = ((mat, [0, 1, 2], (mat, 6)), (mat, [3, 4, 5], (mat, 7)), (mat, 6), (mat, 7), c, c, c, c, (out, 0), n)
    stream = side_stream()
    with torch.cuda.stream(stream):
        pilcheck.plookup_prod_dev(*args, field=field, h_dim=1)
    stream.synchronize()
    first = out.clone()
    torch.cuda.synchronize()
    done = torch.cuda.Event()
    with torch.cuda.stream(stream):
        for _ in range(4):
            pilcheck.plookup_prod_dev(*args, field=field, h_dim=1)
        done.record(stream)
        pending = not done.query()
    stream.synchronize()
    assert pending, "plookup_prod_dev waited for the device"
    assert done.query() and torch.equal(out, first)
