"""The grand product of a permutation or a connection on the device against the integer checker (tests/grand_prod_ref.py), bit-exact, both
fields.  Every case goes through run(): the resident form on a non-default stream, twice, with guard words behind out's matrix; the host
form on copies; the checker on the same bit patterns; and the promise -- gprod_dev / bn128_gprod_dev on the checker's materialised num
and den columns, uploaded, give the same words.  Every input matrix, the guard words and every word of out's matrix outside the column
must come back unchanged.  Elements are bit patterns: the checker and the device both take them mod the modulus; over Fr a pattern X
stands for the value X / 2^256 mod r.  Shapes are the smallest at which the kernels can still go wrong: the lane (8 rows), wave and block
(2048 rows) edges of the Goldilocks scan, bnscan's level thresholds over Fr, k = 1, 3, 16, 1 to 40 terms, sum k = 64."""
import random

import numpy as np
import pytest

import grand_prod_ref as gref
import logup_sum_ref as lref
import bn128_hints_ref as bref
import conn_pols_ref as cref
from hints_ref import P

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from pil2gl import pilcheck, bn128, wtns  # noqa: E402
import pil2gl  # noqa: E402

R, MONT = bref.R, bref.MONT
Q = {"gl": P, "bn128": R}
GUARD = 0x6B6B6B6B6B6B6B6B
FIELDS = ("gl", "bn128")


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


def chal(field, v, raw=False):
    """an extension element as the call takes it: three words, or four Montgomery words (raw: v is the Fr bit pattern itself)"""
    if field == "gl":
        return [int(x) for x in v]
    return [int(x) for x in cref.fr_words([v if raw else v % R * MONT % R])[0]]


def chal_value(field, v, raw):
    return value(field, v) if raw and field == "bn128" else v


def z_words(field, z):
    """the checker's z as the words the column must hold: (n, 3) or (n, 4)"""
    if field == "gl":
        return np.array(z, np.uint64).reshape(len(z), 3)
    return cref.fr_words([v * MONT % R for v in z])


def to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


def rand_rows(rng, field, n, stride):
    return [[rng.randrange(Q[field]) for _ in range(stride)] for _ in range(n)]


def rand_chal(rng, field):
    return tuple(rng.randrange(P) for _ in range(3)) if field == "gl" else rng.randrange(R)


def neg(field, a):
    return tuple((P - x) % P for x in a) if field == "gl" else (R - a) % R


def base_chal(field, v):
    """a base-field value as an extension element"""
    return (v % P, 0, 0) if field == "gl" else v % R


_STREAM = []


def side_stream():
    """one non-default stream for the whole module"""
    if not _STREAM:
        _STREAM.append(torch.cuda.Stream())
    return _STREAM[0]


def ref_terms_of(field, pats, terms, n, raw=False):
    out = []
    for name, cols, sel, den, idc, coef in terms:
        tuples = [[value(field, row[c]) for c in cols] for row in pats[name][:n]]
        s = None if sel is None else [value(field, row[sel[1]]) for row in pats[sel[0]][:n]]
        ids = None if idc is None else [value(field, row[idc[1]]) for row in pats[idc[0]][:n]]
        out.append((tuples, s, den, ids, None if idc is None else chal_value(field, coef, raw)))
    return out


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


def run(field, mats, terms, alpha, beta, gamma, n, out=None, raw=False):
    """mats: name -> rows of bit patterns; terms: (name, cols, (selector's name, col) or None, den, (id's name, col) or None, idCoef);
    alpha, beta, gamma and idCoef: values (a triple / an integer), or with raw the Fr bit patterns; out: (name, col), default a matrix of
    its own with stride gaps -> z as the checker gives it, which the resident form (twice), the host form and gprod on num and den gave too"""
    width = 3 if field == "gl" else 1
    mats = dict(mats)
    if out is None:
        out = ("$out", 1)
        mats["$out"] = [[(0xD00D << 32) + 7 * i + j for j in range(width + 2)] for i in range(n)]
    host = {name: words(field, rows) for name, rows in mats.items()}
    pats = {name: patterns(w) for name, w in host.items()}
    ref_terms = ref_terms_of(field, pats, terms, n, raw)
    a_v, b_v, g_v = (chal_value(field, c, raw) for c in (alpha, beta, gamma))
    want = gref.grand_prod(field, ref_terms, a_v, b_v, g_v, n)
    call_ch = [chal(field, c, raw) for c in (alpha, beta, gamma)]
    expect = host[out[0]].copy()
    expect[:n, out[1]:out[1] + width] = z_words(field, want).reshape((n, width) + expect.shape[2:])

    def spec(bufs):
        return [(bufs[name], cols, None if sel is None else (bufs[sel[0]], sel[1]), den, None if idc is None else (bufs[idc[0]], idc[1]),
                 None if idc is None else chal(field, coef, raw)) for name, cols, sel, den, idc, coef in terms]
    # the resident form: out's matrix followed by guard words in one allocation, a non-default stream, twice
    dev = {name: to_dev(w) for name, w in host.items() if name != out[0]}
    own = host[out[0]]
    held = torch.full((own.size + 16,), GUARD, dtype=torch.int64, device="cuda")
    fresh = to_dev(own).reshape(-1)
    held[:own.size] = fresh
    dev[out[0]] = held[:own.size].view(own.shape)
    stream = side_stream()
    torch.cuda.synchronize()
    got = []
    for _ in range(2):
        held[:own.size] = fresh
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            pilcheck.grand_prod_dev(spec(dev), *call_ch, (dev[out[0]], out[1]), n, field)
        stream.synchronize()
        got.append(held.cpu().numpy().view(np.uint64))
    assert (got[0] == got[1]).all(), "two calls give identical words"
    assert (got[0][own.size:] == np.uint64(GUARD)).all(), "the guard words behind out's matrix"
    assert (got[0][:own.size].reshape(own.shape) == expect).all(), "the resident form: the column is the checker's, every other word as it was"
    for name, w in host.items():
        if name != out[0]:
            assert (dev[name].cpu().numpy().view(np.uint64) == w).all(), name + " is only read"
    # the host form on copies
    h = {name: w.copy() for name, w in host.items()}
    pilcheck.grand_prod(spec(h), *call_ch, (h[out[0]], out[1]), n, field)
    for name, w in host.items():
        assert (h[name] == (expect if name == out[0] else w)).all(), "the host form: " + name
    # the promise: gprod on the two materialised product columns
    num, den = gref.num_den(field, ref_terms, a_v, b_v, g_v, n)
    assert (gprod_on_columns(field, num, den) == z_words(field, want)).all(), "gprod_dev on the materialised num and den gives other words"
    return want


GL_EDGES = (1, 2, 7, 8, 9, 255, 256, 257, 2047, 2048, 2049, 4097)           # SCAN_ITEMS, a wave, SCAN_CHUNK
FR_EDGES = (1, 2, 63, 64, 65, 1024, 1025, 16385)                            # bnscan's level thresholds


@pytest.mark.parametrize("field,n", [("gl", n) for n in GL_EDGES] + [("bn128", n) for n in FR_EDGES])
def test_row_edges_one_num_one_den(field, n):
    rng = random.Random(n)
    a = rand_rows(rng, field, n, 3)
    z = run(field, {"a": a}, [("a", [0, 1], None, 0, None, None), ("a", [2, 1], None, 1, None, None)], rand_chal(rng, field), rand_chal(rng, field),
            rand_chal(rng, field), n)
    assert z[0] == lref.FIELDS[field].one, "z[0] = 1 whatever the row holds"


def perm_terms(k, sel_f, sel_t):
    """f = columns 0 .. k-1 of `f`, t = of `t`; a selector is column k of its matrix"""
    return [("f", list(range(k)), ("f", k) if sel_f else None, 0, None, None), ("t", list(range(k)), ("t", k) if sel_t else None, 1, None, None)]


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("k", [1, 3, 16])
def test_permutation_shapes(field, k):
    rng = random.Random(k)
    n = 257
    f, t = rand_rows(rng, field, n, k + 1), rand_rows(rng, field, n, k + 1)
    for sel_f, sel_t in ((False, False), (True, False), (False, True), (True, True)):
        run(field, {"f": f, "t": t}, perm_terms(k, sel_f, sel_t), rand_chal(rng, field), rand_chal(rng, field), rand_chal(rng, field), n)


@pytest.mark.parametrize("field", FIELDS)
def test_one_sided_forty_terms_and_sum_k_64(field):
    rng = random.Random(3)
    n = 257
    a = rand_rows(rng, field, n, 18)
    ch = lambda: (rand_chal(rng, field), rand_chal(rng, field), rand_chal(rng, field))       # noqa: E731
    for den in (0, 1):                                                           # one side empty: its product is 1
        run(field, {"a": a}, [("a", [0, 5], ("a", 16), den, ("a", 17), rand_chal(rng, field)), ("a", [3], None, den, None, None)], *ch(), n)
    forty = [("a", [u % 16], ("a", 16) if u % 3 == 0 else None, u % 2, ("a", 17) if u % 5 == 0 else None, rand_chal(rng, field)) for u in range(40)]
    run(field, {"a": a}, forty, *ch(), n)
    ks = [16, 16, 16, 1, 1, 1, 1, 3, 3, 6]                                       # sum k = 64 exactly, ten terms
    assert sum(ks) == 64
    terms = [("a", [rng.randrange(16) for _ in range(k)], ("a", 16) if u % 2 else None, u % 2, None, None) for u, k in enumerate(ks)]
    run(field, {"a": a}, terms, *ch(), n)
    with pytest.raises(pil2gl.Pil2glError, match="add up to"):
        pilcheck.grand_prod([(np.zeros((8, 18), np.uint64), list(range(13)), None, 0, None, None)] * 5, [1, 0, 0], [1, 0, 0], [1, 0, 0],
                            (np.zeros((8, 3), np.uint64), 0), 8)


def conn_mats(field, n_bits, n_cols, seed, n_w=20):
    """a trace filled from a small sMap, S from the library's own conn_pols, the x column, and the shifts"""
    rng = random.Random(seed)
    q, N = Q[field], 1 << n_bits
    s_map = [rng.randrange(n_w) for _ in range(N * n_cols)]                      # signal 0: an unconnected cell
    wit = [rng.randrange(q) for _ in range(n_w)]
    a = [[wit[s_map[i * n_cols + j]] if s_map[i * n_cols + j] else rng.randrange(q) for j in range(n_cols)] for i in range(N)]
    w, ks = cref.root(q, n_bits), cref.get_ks(q, n_cols - 1)
    cw, cks = cref.consts(w, ks, q)
    S = wtns.conn_pols(np.array(s_map, np.uint64), n_cols, N, cw, cks, field)   # (N, nCols[, 4]) words
    to_pat = (lambda v: v) if field == "gl" else (lambda v: v * MONT % R)
    mats = {"a": [[to_pat(v) for v in row] for row in a], "S": patterns(S), "x": [[to_pat(pow(w, i, q))] for i in range(N)]}
    return mats, ks


def conn_terms(field, n_cols, ks, delta):
    q, F = Q[field], lref.FIELDS[field]
    terms = []
    for j in range(n_cols):
        k1 = 1 if j == 0 else ks[j - 1]
        terms.append(("a", [j], None, 0, ("x", 0), F.mul(F.ext(delta), F.base(k1)) if field == "gl" else delta * k1 % q))
        terms.append(("a", [j], None, 1, ("S", j), delta))
    return terms


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("n_cols", [1, 2, 12, 18])
def test_connection_closes_and_a_broken_cell_does_not(field, n_cols):
    rng = random.Random(n_cols)
    n_bits = 6
    n, F = 1 << n_bits, lref.FIELDS[field]
    mats, ks = conn_mats(field, n_bits, n_cols, 100 + n_cols)
    gamma, delta = rand_chal(rng, field), rand_chal(rng, field)
    terms = conn_terms(field, n_cols, ks, delta)
    run(field, mats, terms, gamma, gamma, gamma, n)
    pats = {k: v for k, v in mats.items()}
    ref = ref_terms_of(field, pats, terms, n)
    assert gref.closing(field, ref, F.ext(gamma), F.ext(gamma), F.ext(gamma), n) == F.one, "the connection's product closes"
    # the spelling: conn_prod_dev builds the same terms, delta ks' included
    dev = {k: to_dev(words(field, v)) for k, v in mats.items()}
    out = torch.zeros((n, 3) if field == "gl" else (n, 1, 4), dtype=torch.int64, device="cuda")
    pilcheck.conn_prod_dev([(dev["a"], j) for j in range(n_cols)], [(dev["S"], j) for j in range(n_cols)], (dev["x"], 0), ks, chal(field, gamma),
                           chal(field, delta), (out, 0), n, field)
    torch.cuda.synchronize()
    want = gref.grand_prod(field, ref, F.ext(gamma), F.ext(gamma), F.ext(gamma), n)
    assert (out.cpu().numpy().view(np.uint64).reshape(n, -1) == z_words(field, want)).all(), "conn_prod_dev"
    # one cell of a connected signal changed: the product no longer closes (the device's z is the checker's, by run())
    broken = {k: [list(r) for r in v] for k, v in mats.items()}
    broken["a"][n // 2][0] = (broken["a"][n // 2][0] + 1) % Q[field]
    z = run(field, broken, terms, gamma, gamma, gamma, n)
    ref_b = ref_terms_of(field, broken, terms, n)
    last = gref.ratios(field, ref_b, F.ext(gamma), F.ext(gamma), F.ext(gamma), n)[n - 1]
    assert F.mul(z[n - 1], last) != F.one, "a broken cell"


@pytest.mark.parametrize("field", FIELDS)
def test_permutation_closes(field):
    """t is a row permutation of f and the selectors choose equal multisets: z[n-1] R[n-1] = 1; perm_prod_dev is the same two terms"""
    rng = random.Random(31)
    n, q, F = 300, Q[field], lref.FIELDS[field]
    one = 1 if field == "gl" else MONT
    f = [[rng.randrange(q), rng.randrange(q), one * rng.randrange(2) % q] for _ in range(n)]
    t = [list(r) for r in f]
    rng.shuffle(t)
    alpha, beta, gamma = rand_chal(rng, field), rand_chal(rng, field), rand_chal(rng, field)
    terms = perm_terms(2, True, True)
    z = run(field, {"f": f, "t": t}, terms, alpha, beta, gamma, n)
    ref = ref_terms_of(field, {"f": f, "t": t}, terms, n)
    assert F.mul(z[n - 1], gref.ratios(field, ref, alpha, beta, gamma, n)[n - 1]) == F.one
    dev = {"f": to_dev(words(field, f)), "t": to_dev(words(field, t))}
    out = torch.zeros((n, 3) if field == "gl" else (n, 1, 4), dtype=torch.int64, device="cuda")
    pilcheck.perm_prod_dev((dev["f"], [0, 1], (dev["f"], 2)), (dev["t"], [0, 1], (dev["t"], 2)), chal(field, alpha), chal(field, beta), chal(field, gamma),
                           (out, 0), n, field)
    torch.cuda.synchronize()
    assert (out.cpu().numpy().view(np.uint64).reshape(n, -1) == z_words(field, z)).all(), "perm_prod_dev"


@pytest.mark.parametrize("field", FIELDS)
def test_selector_values_and_non_canonical_patterns(field):
    """selectors that are field values other than 0 and 1 pin the blend (H - beta) sel + beta; patterns in [q, 2^64) / [r, 2^256) in tuple,
    id and selector columns, and over Fr in the challenges and idCoef"""
    rng = random.Random(11)
    n, q = 257, Q[field]
    top = (1 << 64) if field == "gl" else (1 << 256)
    a = rand_rows(rng, field, n, 5)
    for i in range(n):
        a[i][3] = rng.choice((0, 1, 2, q - 1, rng.randrange(q)))                 # the selector column: values, not flags
        for j in range(5):
            if rng.randrange(3) == 0:
                a[i][j] = rng.choice((q, q + 1, top - 1, top - 1 - rng.randrange(1 << 20), q + rng.randrange(top - q)))
    terms = [("a", [0, 1], ("a", 3), 0, ("a", 4), None), ("a", [2, 0, 1], ("a", 3), 1, ("a", 4), None)]
    raw = field == "bn128"
    pat = (lambda: rng.choice((q + rng.randrange(top - q), top - 1, rng.randrange(q)))) if raw else (lambda: rand_chal(rng, field))
    for _ in range(3):
        ts = [t[:5] + (pat(),) for t in terms]
        run(field, {"a": a}, ts, pat(), pat(), pat(), n, raw=raw)
    zero = (0, 0, 0) if field == "gl" else 0
    run(field, {"a": a}, [t[:5] + (zero,) for t in terms], zero, rand_chal(rng, field), rand_chal(rng, field), n)      # alpha = 0: H = the last column
    run(field, {"a": a}, [t[:5] + (rand_chal(rng, field),) for t in terms], rand_chal(rng, field), zero, zero, n)      # beta = gamma = 0


@pytest.mark.parametrize("field", FIELDS)
def test_zero_factors(field):
    """gamma chosen from the checker so that one den factor vanishes at row r: z[r+1 ..] is 0 and z[.. r] untouched; two den factors zero
    in one row; a zero num factor is plain arithmetic (every later z is 0 as well, but through the product, not the convention)"""
    rng = random.Random(13)
    F = lref.FIELDS[field]
    n = 2050 if field == "gl" else 1100
    a = rand_rows(rng, field, n, 4)
    alpha, beta = rand_chal(rng, field), rand_chal(rng, field)
    terms = [("a", [0, 1], None, 0, None, None), ("a", [2], None, 1, None, None), ("a", [3], None, 1, None, None)]
    for r in (0, 9, n - 2, 2047 if field == "gl" else 1024):
        gamma = neg(field, base_chal(field, value(field, a[r][2])))             # D of the first den term at row r: a[r][2] + gamma = 0
        z = run(field, {"a": a}, terms, alpha, beta, gamma, n)
        assert all(v == F.zero for v in z[r + 1:]) and all(v != F.zero for v in z[:r + 1])
        plain = gref.grand_prod(field, ref_terms_of(field, {"a": a}, terms, r + 1), alpha, beta, gamma, r + 1)
        assert z[:r + 1] == plain
    b = [list(row) for row in a]
    b[40][3] = b[40][2]                                                          # both den factors of row 40
    z = run(field, {"a": b}, terms, alpha, beta, neg(field, base_chal(field, value(field, b[40][2]))), n)
    assert z[40] != F.zero and z[41] == F.zero
    num_zero = [("a", [2], None, 0, None, None), ("a", [0, 1], None, 1, None, None)]
    z = run(field, {"a": a}, num_zero, alpha, beta, neg(field, base_chal(field, value(field, a[17][2]))), n)
    assert z[17] != F.zero and z[18] == F.zero


@pytest.mark.parametrize("field", FIELDS)
def test_out_as_spare_columns_of_t(field):
    rng = random.Random(17)
    n = 300
    width = 3 if field == "gl" else 1
    t = rand_rows(rng, field, n, 3 + width + 1)                                  # t0, t1, selT, then z, then one more column that must survive
    f = rand_rows(rng, field, n, 3)
    terms = [("f", [0, 1], ("f", 2), 0, None, None), ("t", [0, 1], ("t", 2), 1, None, None)]
    run(field, {"t": t, "f": f}, terms, rand_chal(rng, field), rand_chal(rng, field), rand_chal(rng, field), n, out=("t", 3))


@pytest.mark.parametrize("field,n", [("gl", 2048 * 256 + 1), ("bn128", 262145)])
def test_deep_scans_periodic_inputs(field, n):
    """257 block totals (a lane of the second pass walks two) / five levels; period 64 keeps the checker cheap.  The resident form only."""
    rng = random.Random(23)
    per = 64
    width = 3 if field == "gl" else 1
    base = rand_rows(rng, field, per, 4)
    mat = words(field, base)
    full = np.concatenate([mat] * (n // per + 1))[:n]
    dev = to_dev(full)
    out = torch.zeros((n, width) if field == "gl" else (n, 1, 4), dtype=torch.int64, device="cuda")
    alpha, beta, gamma, coef = (rand_chal(rng, field) for _ in range(4))
    terms = [(dev, [0, 1], (dev, 2), 0, (dev, 3), chal(field, coef)), (dev, [1], None, 1, None, None)]
    pilcheck.grand_prod_dev(terms, chal(field, alpha), chal(field, beta), chal(field, gamma), (out, 0), n, field)
    torch.cuda.synchronize()
    vals = [[value(field, v) for v in row] for row in patterns(mat)]
    ref = [([r[:2] for r in vals], [r[2] for r in vals], 0, [r[3] for r in vals], coef), ([r[1:2] for r in vals], None, 1, None, None)]
    want = gref.grand_prod(field, ref, alpha, beta, gamma, n, period=per)
    got = out.cpu().numpy().view(np.uint64).reshape(n, -1)
    assert (got == z_words(field, want)).all()


@pytest.mark.parametrize("field", FIELDS)
def test_resident_call_only_enqueues(field):
    """the call returns before its work is done: after one warm-up (the working slots grow with a device synchronise on first use), four
    calls of 36 terms over 2^22 (Goldilocks) / 2^20 (Fr) rows -- milliseconds of device work each -- are sent on a side stream and an
    event recorded behind them has not completed when the last call returns; nothing is compared here but that and the two runs' words"""
    n = 1 << (22 if field == "gl" else 20)
    g = torch.Generator(device="cuda").manual_seed(41)
    mat = torch.randint(0, 1 << 62, (n, 4) if field == "gl" else (n, 4, 4), dtype=torch.int64, device="cuda", generator=g)     # below both moduli
    out = torch.zeros((n, 3) if field == "gl" else (n, 1, 4), dtype=torch.int64, device="cuda")
    c = chal(field, rand_chal(random.Random(3), field))
    terms = [(mat, [u % 3], None, u % 2, (mat, 3), c) for u in range(36)]
    stream = side_stream()
    with torch.cuda.stream(stream):
        pilcheck.grand_prod_dev(terms, c, c, c, (out, 0), n, field)
    stream.synchronize()
    first = out.clone()
    torch.cuda.synchronize()
    done = torch.cuda.Event()
    with torch.cuda.stream(stream):
        for _ in range(4):
            pilcheck.grand_prod_dev(terms, c, c, c, (out, 0), n, field)
        done.record(stream)
        pending = not done.query()
    stream.synchronize()
    assert pending, "grand_prod_dev waited for the device"
    assert done.query() and torch.equal(out, first)
