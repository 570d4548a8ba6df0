"""The lookup grand sum and the column-numerator gsum on the device against the integer checker (tests/logup_sum_ref.py), bit-exact, both
fields.  Every logup_sum case goes through run(): the resident form on a non-default stream, twice, with guard words behind out's matrix;
the host form on copies; the checker on the same bit patterns.  Every input matrix, the guard words and every word of out's matrix outside
the column must come back unchanged.  Elements are bit patterns: the checker and the device both take them mod the modulus; over Fr a
pattern X stands for the value X / 2^256 mod r.  Shapes are the smallest at which the kernels can still go wrong: the lane (8 rows), wave
and block (2048 rows) edges of the Goldilocks scan, bnscan's level thresholds over Fr, k = 1, 3, 16, 1, 2 and 9 terms."""
import random

import numpy as np
import pytest

import logup_sum_ref as lref
import lookup_mult_ref as mref
import bn128_hints_ref as bref
import conn_pols_ref as cref
from hints_ref import P

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from pil2gl import pilcheck, bn128  # noqa: E402
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


def elem(field, v):
    """a base-field value as the call takes coef / busId"""
    return v % P if field == "gl" else [int(x) for x in cref.fr_words([v % R * MONT % R])[0]]


def chal(field, v):
    """a challenge as the call takes it: three words, or four Montgomery words"""
    return [int(x) for x in v] if field == "gl" else elem(field, v)


def s_words(field, s):
    """the checker's s as the words the column must hold: (n, 3) or (n, 4)"""
    if field == "gl":
        return np.array(s, np.uint64).reshape(len(s), 3)
    return cref.fr_words([v * MONT % R for v in s])


def to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


def rand_rows(rng, field, n, stride):
    return [[rng.randrange(Q[field]) for _ in range(stride)] for _ in range(n)]


def rand_chal(rng, field):
    return tuple(rng.randrange(P) for _ in range(3)) if field == "gl" else rng.randrange(R)


def neg(field, a):
    return tuple((P - x) % P for x in a) if field == "gl" else (R - a) % R


def zero_beta(field, row, alpha, bus):
    """the beta that makes D zero for this tuple and bus id"""
    F = lref.FIELDS[field]
    return neg(field, lref.denominator(F, [value(field, v) for v in row], F.ext(alpha), F.zero, bus))


_STREAM = []


def side_stream():
    """one non-default stream for the whole module"""
    if not _STREAM:
        _STREAM.append(torch.cuda.Stream())
    return _STREAM[0]


def run(field, mats, terms, alpha, beta, n, out=None, period=None):
    """mats: name -> rows of bit patterns; terms: (name, cols, (numerator's name, col) or None, coef, bus) with coef and bus VALUES;
    alpha, beta: values (a triple / an integer); out: (name, col), default a matrix of its own with stride gaps
    -> s as the checker gives it, which the resident form (twice) and the host form gave too"""
    width = 3 if field == "gl" else 1
    mats = dict(mats)
    if out is None:
        out = ("$out", 1)
        mats["$out"] = [[(0xD00D << 32) + 7 * i + j for j in range(width + 2)] for i in range(n)]
    host = {name: words(field, rows) for name, rows in mats.items()}
    pats = {name: patterns(w) for name, w in host.items()}
    ref_terms = []
    for name, cols, num, coef, bus in terms:
        tuples = [[value(field, row[c]) for c in cols] for row in pats[name][:n]]
        w = None if num is None else [value(field, row[num[1]]) for row in pats[num[0]][:n]]
        ref_terms.append((tuples, w, coef, bus))
    want = lref.logup_sum(field, ref_terms, alpha, beta, n, period)
    call_terms = [(name, cols, num, elem(field, coef), elem(field, bus)) for name, cols, num, coef, bus in terms]
    expect = host[out[0]].copy()
    if n:
        expect[:n, out[1]:out[1] + width] = s_words(field, want).reshape((n, width) + expect.shape[2:])

    def spec(bufs):
        return [(bufs[name], cols, None if num is None else (bufs[num[0]], num[1]), c, b) for name, cols, num, c, b in call_terms]
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
            pilcheck.logup_sum_dev(spec(dev), chal(field, alpha), chal(field, beta), (dev[out[0]], out[1]), n, field)
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
    pilcheck.logup_sum(spec(h), chal(field, alpha), chal(field, beta), (h[out[0]], out[1]), n, field)
    for name, w in host.items():
        assert (h[name] == (expect if name == out[0] else w)).all(), "the host form: " + name
    return want


GL_EDGES = (1, 2, 7, 8, 9, 255, 256, 257, 2047, 2048, 2049, 4097)           # SCAN_ITEMS, a wave, SCAN_CHUNK
FR_EDGES = (1, 2, 63, 64, 65, 1024, 1025, 16385)                            # bnscan's level thresholds


@pytest.mark.parametrize("field,n", [("gl", n) for n in GL_EDGES] + [("bn128", n) for n in FR_EDGES])
def test_row_edges_one_term(field, n):
    rng = random.Random(n)
    a = rand_rows(rng, field, n, 2)
    run(field, {"a": a}, [("a", [1], None, 1, rng.randrange(Q[field]))], rand_chal(rng, field), rand_chal(rng, field), n)


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("ks", [(1,), (3,), (16,), (3, 3), (1, 16), (3,) * 9, (1, 2, 3, 16, 5, 1, 7, 16, 4)])
def test_term_and_tuple_shapes(field, ks):
    """k in {1, 3, 16}, 1, 2 and 9 terms, a k of its own per term; the matrix `a` serves every term but the last, which has its numerator there"""
    rng = random.Random(sum(ks) + len(ks))
    n, q = 257, Q[field]
    a, b = rand_rows(rng, field, n, 19), rand_rows(rng, field, n, 17)
    terms = []
    for u, k in enumerate(ks):
        cols = [rng.randrange(16) for _ in range(k)]                             # any order, repeats allowed
        last = u == len(ks) - 1
        terms.append(("b" if last else "a", cols, ("a", 16 + u % 3) if u % 2 == 0 else None, rng.choice((1, q - 1, 5, rng.randrange(q))), rng.randrange(q)))
    run(field, {"a": a, "b": b}, terms, rand_chal(rng, field), rand_chal(rng, field), n)


@pytest.mark.parametrize("field", FIELDS)
def test_non_canonical_patterns_numerators_coefficients_and_challenges(field):
    rng = random.Random(11)
    n, q = 257, Q[field]
    top = (1 << 64) if field == "gl" else (1 << 256)
    a = rand_rows(rng, field, n, 4)
    for i in range(n):                                                           # patterns in [q, 2^64) / [r, 2^256): tuple and numerator columns alike
        for j in range(4):
            if rng.randrange(3) == 0:
                a[i][j] = rng.choice((q, q + 1, top - 1, top - 1 - rng.randrange(1 << 20), q + rng.randrange(top - q)))
    num = [[rng.choice((0, 0, 1, 2, 3, q - 1, rng.randrange(q)))] for _ in range(n)]     # zeros and values >= 2
    mats = {"a": a, "w": num}
    one = (0, 1, 0) if field == "gl" else 1
    for coef in (0, 1, q - 1, 5):
        run(field, mats, [("a", [0, 1], ("w", 0), coef, 9), ("a", [2], ("a", 3), q - 1, 0)], rand_chal(rng, field), rand_chal(rng, field), n)
    run(field, mats, [("a", [0, 1, 2], None, 1, 3), ("a", [3], None, 5, 4)], rand_chal(rng, field), rand_chal(rng, field), n)        # numerator NULL
    zero = (0, 0, 0) if field == "gl" else 0
    unit = (1, 0, 0) if field == "gl" else 1
    for alpha in (zero, unit, one):                                              # alpha 0: D = busId + beta; (0, 1, 0): the extension's x
        run(field, mats, [("a", [0, 1, 2], ("w", 0), 1, 3), ("a", [3, 0], None, q - 1, 4)], alpha, rand_chal(rng, field), n)
    run(field, mats, [("a", [0, 1, 2], ("w", 0), 1, 3), ("a", [3, 0], None, q - 1, 4)], rand_chal(rng, field), zero, n)              # beta = 0
    run(field, mats, [("a", [0], ("w", 0), 1, 0)], zero, zero, n)                # D = 0 everywhere: the whole column is 0


@pytest.mark.parametrize("field", FIELDS)
def test_zero_denominators(field):
    """beta and the bus ids are chosen from the checker so that D vanishes at chosen rows: row 0, row n - 1, 2047 and 2048, all eight rows
    of one lane -- for one term of three, the other two still counting -- and every term at once in rows 5 and 2048"""
    rng = random.Random(13)
    n, q, F = 2050, Q[field], lref.FIELDS[field]
    a, b, c = (rand_rows(rng, field, n, 3) for _ in range(3))
    alpha = rand_chal(rng, field)
    hit = [0, n - 1, 2047, 2048] + list(range(16, 24))
    for i in hit:
        b[i][:2] = b[0][:2]                                                       # term b: the tuple of row 0 at every hit row
    for i in (5, 2048):
        a[i][:2] = b[0][:2]
        c[i][:2] = b[0][:2]                                                       # every term of rows 5 and 2048 (b's row 5 too)
    b[5][:2] = b[0][:2]
    beta = zero_beta(field, b[0][:2], alpha, 77)
    terms = [("a", [0, 1], ("a", 2), 1, 77), ("b", [0, 1], None, 5, 77), ("c", [0, 1], ("c", 2), q - 1, 77)]
    s = run(field, {"a": a, "b": b, "c": c}, terms, alpha, beta, n)
    ref_terms = lambda names: [([[value(field, v) for v in row[:2]] for row in m], None if w is None else [value(field, row[2]) for row in m], co, 77)      # noqa: E731
                               for m, w, co in names]
    rows = lambda ts, i: lref.row_fraction(F, ts, F.ext(alpha), F.ext(beta), i)[2]    # noqa: E731
    two = ref_terms([(a, 1, 1), (c, 1, q - 1)])
    step = lambda i: F.add(s[i], neg(field, s[i - 1] if i else F.zero))              # noqa: E731
    for i in hit:
        if i != 2048:
            assert step(i) == rows(two, i) != F.zero, "one term of three is zero, the other two still count"
    assert step(5) == F.zero and step(2048) == F.zero, "every term of the row is zero: the row adds 0"
    assert step(6) != F.zero and step(2049) != F.zero


@pytest.mark.parametrize("field", FIELDS)
def test_out_as_spare_columns_of_t(field):
    rng = random.Random(17)
    n, q = 300, Q[field]
    width = 3 if field == "gl" else 1
    t = rand_rows(rng, field, n, 3 + width + 1)                                  # t0, t1, m, then s, then one more column that must survive
    f = rand_rows(rng, field, n, 2)
    terms = [("f", [0, 1], None, 1, 2), ("t", [0, 1], ("t", 2), q - 1, 2)]
    run(field, {"t": t, "f": f}, terms, rand_chal(rng, field), rand_chal(rng, field), n, out=("t", 3))


@pytest.mark.parametrize("field", FIELDS)
def test_with_lookup_mult(field):
    """two f sides with selectors, a selT, duplicate tuples in t: lookup_mult writes m, logup_sum runs with coef +1, +1, -1 and the sum
    closes exactly when the lookup holds"""
    rng = random.Random(19)
    n, q = 257, Q[field]
    width = 3 if field == "gl" else 1
    uniq = [[rng.randrange(q), rng.randrange(q)] for _ in range(40)]
    t = [list(uniq[rng.randrange(40)]) + [rng.randrange(3) != 0, 0] + [0] * width for _ in range(n)]      # t0 t1 selT m s..
    live = [row[:2] for row in t if row[2]]
    fs = [[list(live[rng.randrange(len(live))]) + [rng.randrange(2)] for _ in range(n)] for _ in range(2)]   # f0 f1 selF
    alpha, beta = rand_chal(rng, field), rand_chal(rng, field)
    one = 1 if field == "gl" else MONT
    for alter in (False, True):
        f0 = [list(r) for r in fs[0]]
        if alter:
            f0[100] = [q - 3, q - 4, 1]                                          # a selected row of f 0 that t does not hold
        enc = lambda rows, sel_cols: [[(one * v % q if j in sel_cols else v) for j, v in enumerate(r)] for r in rows]   # noqa: E731  selectors as field 0 / 1
        host = {"t": words(field, enc(t, (2,))), "f0": words(field, enc(f0, (2,))), "f1": words(field, enc(fs[1], (2,)))}
        dev = {k: to_dev(v) for k, v in host.items()}
        rep = pilcheck.lookup_mult_dev([(dev["f0"], [0, 1], (dev["f0"], 2)), (dev["f1"], [0, 1], (dev["f1"], 2))], (dev["t"], [0, 1], (dev["t"], 2)),
                                       (dev["t"], 3), n, field)
        assert rep[0] == (1 if alter else 0)
        minus = elem(field, q - 1)
        terms = [(dev["f0"], [0, 1], (dev["f0"], 2), elem(field, 1), elem(field, 0)), (dev["f1"], [0, 1], (dev["f1"], 2), elem(field, 1), elem(field, 0)),
                 (dev["t"], [0, 1], (dev["t"], 3), minus, elem(field, 0))]
        pilcheck.logup_sum_dev(terms, chal(field, alpha), chal(field, beta), (dev["t"], 4), n, field)
        torch.cuda.synchronize()
        got = dev["t"].cpu().numpy().view(np.uint64)
        last = got[n - 1, 4:4 + width].reshape(-1)
        # the checker on the same words, m taken from its own dictionary
        pat = {k: patterns(v) for k, v in host.items()}
        sel = lambda name: [row[2] for row in pat[name]]                         # noqa: E731
        tup = lambda name: [row[:2] for row in pat[name]]                        # noqa: E731
        m, _ = mref.multiplicities([tup("f0"), tup("f1")], tup("t"), q, [sel("f0"), sel("f1")], sel("t"))
        val = lambda name: [[value(field, v) for v in row[:2]] for row in pat[name]]     # noqa: E731
        ref_terms = [(val("f0"), [value(field, v) for v in sel("f0")], 1, 0), (val("f1"), [value(field, v) for v in sel("f1")], 1, 0), (val("t"), m, q - 1, 0)]
        want = lref.logup_sum(field, ref_terms, alpha, beta, n)
        assert (got[:n, 4:4 + width].reshape(n, -1) == s_words(field, want)).all()
        closed = want[n - 1] == lref.FIELDS[field].zero
        assert closed == (not alter) and bool(last.any()) == alter, "s[n-1] is 0 exactly when the lookup holds"


@pytest.mark.parametrize("field,n", [("gl", 2048 * 256 + 1), ("bn128", 262145)])
def test_deep_scans_periodic_inputs(field, n):
    """257 block totals (a lane of the second pass walks two) / five levels; period 64 keeps the checker cheap.  The resident form only."""
    rng = random.Random(23)
    q, per = Q[field], 64
    width = 3 if field == "gl" else 1
    base = rand_rows(rng, field, per, 3)
    mat = words(field, base)
    full = np.concatenate([mat] * (n // per + 1))[:n]
    dev = to_dev(full)
    out = torch.zeros((n, width) if field == "gl" else (n, 1, 4), dtype=torch.int64, device="cuda")
    alpha, beta = rand_chal(rng, field), rand_chal(rng, field)
    terms = [(dev, [0, 1], (dev, 2), elem(field, 1), elem(field, 3)), (dev, [1], None, elem(field, q - 1), elem(field, 4))]
    pilcheck.logup_sum_dev(terms, chal(field, alpha), chal(field, beta), (out, 0), n, field)
    torch.cuda.synchronize()
    vals = [[value(field, v) for v in row] for row in patterns(mat)]
    ref_terms = [([r[:2] for r in vals], [r[2] for r in vals], 1, 3), ([r[1:2] for r in vals], None, q - 1, 4)]
    want = lref.logup_sum(field, ref_terms, alpha, beta, n, period=per)
    got = out.cpu().numpy().view(np.uint64).reshape(n, -1)
    at = [0, 1, 63, 64, 2047, 2048, 2049, n // 2, n - 2, n - 1] + [rng.randrange(n) for _ in range(2000)]
    assert (got[at] == s_words(field, [want[i] for i in at])).all()
    assert (got == s_words(field, want)).all()


# ---- gsum with a column numerator ----
@pytest.mark.parametrize("dn,dd", [(1, 1), (1, 3), (3, 1), (3, 3)])
def test_gsum_col_goldilocks(dn, dd):
    rng = random.Random(dn * 4 + dd)
    for n in GL_EDGES:
        num = [[rng.randrange(P) for _ in range(dn)] for _ in range(n)]
        den = [[rng.randrange(P) for _ in range(dd)] for _ in range(n)]
        for i in {0, n - 1, n // 2, 2047 % n, 2048 % n} | set(range(8, 16)) & set(range(n)):
            den[i] = [0] * dd                                                     # zero denominators: the edges and one whole lane
        e3 = lambda r: tuple(r) + (0,) * (3 - len(r))                            # noqa: E731
        want = lref.gsum_col("gl", [e3(r) for r in num], [e3(r) for r in den])
        dim = max(dn, dd)
        d_num, d_den = to_dev(np.array(num, np.uint64)), to_dev(np.array(den, np.uint64))
        got = pil2gl.calculateS_col(d_num, d_den, dn, dd).cpu().numpy().view(np.uint64).reshape(n, dim)
        assert (got == np.array([w[:dim] for w in want], np.uint64)).all(), (n, dn, dd)
        assert (d_num.cpu().numpy().view(np.uint64) == np.array(num, np.uint64)).all() and (d_den.cpu().numpy().view(np.uint64) == np.array(den, np.uint64)).all()
    # a constant column gives the words gsum gives for that constant
    const = to_dev(np.array([num[0]] * n, np.uint64))
    a = pil2gl.calculateS_col(const, d_den, dn, dd).cpu().numpy()
    b = pil2gl.calculateS(to_dev(np.array(num[0], np.uint64)), d_den, dn, dd).cpu().numpy()
    assert (a == b).all()


@pytest.mark.parametrize("stride", [1, 3])
def test_gsum_col_fr(stride):
    rng = random.Random(stride)
    for n in FR_EDGES:
        num = [rng.randrange(R) for _ in range(n)]
        den = [rng.randrange(R) for _ in range(n)]
        for i in {0, n - 1, n // 2, 63 % n, 64 % n}:
            den[i] = 0
        want = bref.mont_words(lref.gsum_col("bn128", num, den))

        def col(vals):
            m = np.full((n, stride, 4), GUARD, np.uint64)
            m[:, 0] = bref.mont_words(vals)
            return m
        h_num, h_den, h_out = col(num), col(den), col([0] * n)
        d_num, d_den, d_out = to_dev(h_num), to_dev(h_den), to_dev(h_out)
        bn128.gsum_col(d_num, d_den, n, stride, stride, d_out, stride)
        got = d_out.cpu().numpy().view(np.uint64)
        assert (got[:, 0] == want).all() and (got[:, 1:] == np.uint64(GUARD)).all(), (n, stride)
        assert (d_num.cpu().numpy().view(np.uint64) == h_num).all() and (d_den.cpu().numpy().view(np.uint64) == h_den).all()
        assert (bn128.gsum_col(h_num, h_den, n, stride, stride, h_out, stride)[:, 0] == want).all(), "the host form"
    c = rng.randrange(R)
    a = bn128.gsum_col(to_dev(col([c] * n)), d_den, n, stride, stride).cpu().numpy()
    b = bn128.gsum(bref.mont_words([c])[0], d_den, n, stride).cpu().numpy()
    assert (a == b).all(), "a constant column gives gsum's words"


def test_stark_resolve_hints_info_gsum_with_a_column_numerator():
    """a gsum hint whose numerator is a cm column (a multiplicity) writes the checker's column and `result`"""
    from pil2gl import stark
    n_bits = 6
    N = 1 << n_bits
    rng = random.Random(29)
    m = [rng.choice((0, 1, 2, 7)) for _ in range(N)]
    d = [[rng.randrange(1, P) for _ in range(3)] for _ in range(N)]
    cm1 = np.array([[m[i]] + d[i] for i in range(N)], np.uint64)
    cmap = [{"stage": 1, "dim": 1, "stagePos": 0}, {"stage": 1, "dim": 3, "stagePos": 1}, {"stage": 2, "dim": 3, "stagePos": 0}]
    info = {"cmPolsMap": cmap, "mapSectionsN": {"cm1": 4, "cm2": 3}}
    exprs = {"expressionsCode": [], "hintsInfo": [
        {"name": "gsum", "fields": [{"name": "numerator", "op": "cm", "id": 0}, {"name": "denominator", "op": "cm", "id": 1}, {"name": "reference", "op": "cm", "id": 2},
                                    {"name": "result", "op": "subproofValue", "id": 0}]}]}
    be = stark.GpuBackend(0)
    bufs = {"cm1_n": be.from_host(cm1), "cm2_n": be.zeros(3 * N)}
    ctx = {"pilInfo": info, "publics": [], "challenges": [[], []], "evals": []}
    stark.resolve_hints_info(be, info, exprs, 2, bufs, {"cm1_n": 4, "cm2_n": 3}, n_bits, ctx)
    want = lref.gsum_col("gl", [(v, 0, 0) for v in m], [tuple(r) for r in d])
    got = be.to_host(bufs["cm2_n"]).reshape(N, 3)
    assert (got == np.array(want, np.uint64)).all()
    assert ctx["subproofValues"][0] == [int(v) for v in want[N - 1]]

    class NoCol:                                                                  # a backend without the method keeps today's refusal
        def __getattr__(self, name):
            if name == "gsum_col":
                raise AttributeError(name)
            return getattr(be, name)
    with pytest.raises(ValueError, match="constant numerator"):
        stark.resolve_hints_info(NoCol(), info, exprs, 2, bufs, {"cm1_n": 4, "cm2_n": 3}, n_bits, ctx)


@pytest.mark.parametrize("field", FIELDS)
def test_resident_call_only_enqueues(field):
    """the call returns before its work is done: after one warm-up (the working slots grow with a device synchronise on first use), four
    calls of nine terms over 2^22 (Goldilocks) / 2^20 (Fr) rows -- milliseconds of device work each -- are sent on a side stream and an
    event recorded behind them has not completed when the last call returns; nothing is compared here but that and the two runs' words"""
    n = 1 << (22 if field == "gl" else 20)
    g = torch.Generator(device="cuda").manual_seed(41)
    mat = torch.randint(0, 1 << 62, (n, 4) if field == "gl" else (n, 4, 4), dtype=torch.int64, device="cuda", generator=g)     # below both moduli
    out = torch.zeros((n, 3) if field == "gl" else (n, 1, 4), dtype=torch.int64, device="cuda")
    terms = [(mat, [u % 3, (u + 1) % 3, 2], (mat, 3), elem(field, 1 + u), elem(field, 9)) for u in range(9)]
    a, b = chal(field, rand_chal(random.Random(1), field)), chal(field, rand_chal(random.Random(2), field))
    stream = side_stream()
    with torch.cuda.stream(stream):
        pilcheck.logup_sum_dev(terms, a, b, (out, 0), n, field)
    stream.synchronize()
    first = out.clone()
    torch.cuda.synchronize()
    done = torch.cuda.Event()
    with torch.cuda.stream(stream):
        for _ in range(4):
            pilcheck.logup_sum_dev(terms, a, b, (out, 0), n, field)
        done.record(stream)
        pending = not done.query()
    stream.synchronize()
    assert pending, "logup_sum_dev waited for the device"
    assert done.query() and torch.equal(out, first)
