"""The clustered logUp sum on the device, bit-exact in both fields against the integer checker (tests/logup_cluster_ref.py) AND against the
statement's two promises, computed with logup_sum_dev / range_sum_dev in the same test:
  1. s is what logup_sum_dev (no range) or range_sum_dev gives on the same terms;
  2. im_c[i] = s_c[i] - s_c[i-1], s_c being that call on cluster c's terms alone.
Every case goes through run(), test_gpu_range_sum.py's discipline (its bit-pattern helpers are imported): the resident form on a non-default
stream, twice, with guard words behind EVERY output matrix; the host form on copies.  Every input matrix, the guards and every word of the
output matrices outside the written columns must come back unchanged.  The m columns are non-canonical, non-zero poison outside the windows.
Shapes are the smallest at which the kernels can still go wrong: cluster_scan1 takes 8 rows a lane and 2048 a block, as logup_scan1 does,
so the lane and block edges are logup_sum's; over Fr bnscan's level thresholds."""
import random

import numpy as np
import pytest

import logup_sum_ref as lref
import range_sum_ref as rref
import logup_cluster_ref as cref
import test_gpu_range_sum as rs
from hints_ref import P

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from pil2gl import pilcheck  # noqa: E402

R, Q, FIELDS, GUARD = rs.R, rs.Q, rs.FIELDS, rs.GUARD
DIRECT = cref.DIRECT
D = DIRECT


def diff_words(field, s):
    """s[i] - s[i-1] (s[-1] = 0) on the words of a column: (n, 3) canonical Goldilocks words, or (n, 4) canonical Montgomery words, whose
    difference mod r is the difference's Montgomery form"""
    if field == "gl":
        v = [[int(x) for x in row] for row in s]
        return np.array([[(a - b) % P for a, b in zip(row, v[i - 1] if i else (0, 0, 0))] for i, row in enumerate(v)], np.uint64).reshape(len(v), 3)
    v = [sum(int(e[k]) << (64 * k) for k in range(4)) for e in s]
    return rs.cref.fr_words([(a - (v[i - 1] if i else 0)) % R for i, a in enumerate(v)])


def run(field, mats, terms, ranges, cluster, im, alpha, beta, n, out, raw=False, host_form=True):
    """mats: name -> rows of bit patterns, the output matrices among them; terms, ranges: test_gpu_range_sum.run's; cluster: an entry a term;
    im: (name, col) a cluster; out: (name, col); alpha, beta: values, or with raw bit patterns -> (s, im) as the checker gives them"""
    width = 3 if field == "gl" else 1
    n_im = len(im)
    host = {name: rs.words(field, rows) for name, rows in mats.items()}
    pats = {name: rs.patterns(w) for name, w in host.items()}
    a_pat, b_pat = (alpha, beta) if raw else (rs.chal_pattern(field, alpha), rs.chal_pattern(field, beta))
    a_val, b_val = rs.chal_value(field, a_pat), rs.chal_value(field, b_pat)
    ref_terms = []
    for name, cols, num, coef, bus in terms:
        tuples = [[rs.value(field, row[c]) for c in cols] for row in pats[name][:n]]
        w = None if num is None else [rs.value(field, row[num[1]]) for row in pats[num[0]][:n]]
        ref_terms.append((tuples, w, coef, bus))
    ref_ranges = [([rs.value(field, pats[name][i][col]) if row0 <= i < row0 + size else None for i in range(n)], lo, size, row0, coef, bus)
                  for name, col, lo, size, row0, coef, bus in ranges]
    want_s, want_im = cref.cluster_sum(field, ref_terms, ref_ranges, cluster, n_im, a_val, b_val, n)
    call_terms = [(name, cols, num, rs.elem(field, coef), rs.elem(field, bus)) for name, cols, num, coef, bus in terms]
    call_ranges = [(name, col, lo, size, row0, rs.elem(field, coef), rs.elem(field, bus)) for name, col, lo, size, row0, coef, bus in ranges]
    a_w, b_w = rs.chal_words(field, a_pat), rs.chal_words(field, b_pat)
    outputs = [(out, want_s)] + list(zip(im, want_im))
    written = {name for (name, _), _ in outputs}
    expect = {name: host[name].copy() for name in written}
    for (name, col), want in outputs:
        e = expect[name]
        e[:n, col:col + width] = rs.s_words(field, want).reshape((n, width) + e.shape[2:])

    def spec(bufs, which=None):
        keep = range(len(cluster)) if which is None else which
        return ([(bufs[name], cols, None if num is None else (bufs[num[0]], num[1]), c, b) for u, (name, cols, num, c, b) in enumerate(call_terms) if u in keep],
                [((bufs[name], col), lo, size, row0, c, b) for v, (name, col, lo, size, row0, c, b) in enumerate(call_ranges) if len(call_terms) + v in keep])
    # the resident form: every output matrix followed by guard words in one allocation, a non-default stream, twice
    dev = {name: rs.to_dev(w) for name, w in host.items() if name not in written}
    held, fresh = {}, {}
    for name in written:
        own = host[name]
        held[name] = torch.full((own.size + 16,), GUARD, dtype=torch.int64, device="cuda")
        fresh[name] = rs.to_dev(own).reshape(-1)
        dev[name] = held[name][:own.size].view(own.shape)
    stream = rs.side_stream()
    got = []
    for _ in range(2):
        for name in written:
            held[name][:host[name].size] = fresh[name]
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            pilcheck.logup_cluster_dev(*spec(dev), cluster, [(dev[name], col) for name, col in im], a_w, b_w, (dev[out[0]], out[1]), n, field)
        stream.synchronize()
        got.append({name: held[name].cpu().numpy().view(np.uint64) for name in written})
    for name in written:
        size = host[name].size
        assert (got[0][name] == got[1][name]).all(), "two calls give identical words: " + name
        assert (got[0][name][size:] == np.uint64(GUARD)).all(), "the guard words behind " + name
        bad = np.argwhere(got[0][name][:size].reshape(host[name].shape) != expect[name])
        assert bad.size == 0, "the resident form: %s, first differing (row, word ..) %s" % (name, bad[0])
    for name, w in host.items():
        if name not in written:
            assert (dev[name].cpu().numpy().view(np.uint64) == w).all(), name + " is only read"

    def plain_sum(which):
        """logup_sum_dev / range_sum_dev on the terms `which` -> the words of its s"""
        t, r = spec(dev, which)
        o = torch.zeros((n, width) if field == "gl" else (n, 1, 4), dtype=torch.int64, device="cuda")
        if r:
            pilcheck.range_sum_dev(t, r, a_w, b_w, (o, 0), n, field)
        else:
            pilcheck.logup_sum_dev(t, a_w, b_w, (o, 0), n, field)
        torch.cuda.synchronize()
        return o.cpu().numpy().view(np.uint64).reshape(n, -1)
    # promise 1: s against the unclustered call on the same terms
    assert (plain_sum(range(len(cluster))) == rs.s_words(field, want_s)).all(), "s is logup_sum_dev's / range_sum_dev's on the same terms"
    # promise 2: im_c against the differences of that call on cluster c's terms alone
    for c in range(n_im):
        sc = plain_sum([u for u, g in enumerate(cluster) if g == c])
        assert (diff_words(field, sc) == rs.s_words(field, want_im[c])).all(), "im_%d is s_c[i] - s_c[i-1]" % c
    # the host form on copies
    if host_form:
        h = {name: w.copy() for name, w in host.items()}
        pilcheck.logup_cluster(*spec(h), cluster, [(h[name], col) for name, col in im], a_w, b_w, (h[out[0]], out[1]), n, field)
        for name, w in host.items():
            assert (h[name] == expect.get(name, w)).all(), "the host form: " + name
    return want_s, want_im


def out_matrix(field, n, n_im, tag=0xD00D):
    """a matrix for s and n_im im columns with a gap word before, between and behind the elements"""
    width = 3 if field == "gl" else 1
    stride = (n_im + 1) * (width + 1) + 1
    rows = [[(tag << 32) + 7 * i + j for j in range(stride)] for i in range(n)]
    return rows, [1 + o * (width + 1) for o in range(n_im + 1)]


def one_matrix_case(field, rng, n, terms, ranges, cluster, mats, **kw):
    n_im = 1 + max(c for c in cluster if c != D)
    rows, cols = out_matrix(field, n, n_im)
    mats = dict(mats, **{"$o": rows})
    return run(field, mats, terms, ranges, cluster, [("$o", c) for c in cols[1:]], rs.rand_chal(rng, field), rs.rand_chal(rng, field), n, ("$o", cols[0]), **kw)


GL_EDGES = (1, 7, 8, 9, 2047, 2048, 2049, 4097)                             # SCAN_ITEMS and SCAN_CHUNK: cluster_scan1 keeps logup_scan1's geometry
FR_EDGES = rs.FR_EDGES                                                      # bnscan's level thresholds


@pytest.mark.parametrize("field,n", [("gl", n) for n in GL_EDGES] + [("bn128", n) for n in FR_EDGES])
def test_row_edges(field, n):
    """a k = 1 term, a k = 3 term with a numerator column and a range over all rows: one cluster of two and a DIRECT term; non-canonical words"""
    rng = random.Random(n)
    q = Q[field]
    f = rs.poison_rows(rng, field, n, 5)
    m = rs.poison_rows(rng, field, n, 2)
    terms = [("f", [0], None, 1, 3), ("f", [3, 1, 2], ("f", 4), q - 1, rng.randrange(q))]
    ranges = [("m", 1, rng.randrange(1 << 20), n, 0, q - 1, 3)]
    one_matrix_case(field, rng, n, terms, ranges, [0, D, 0], {"f": f, "m": m}, host_form=n <= 2049)


def nine(field, rng, n, n_f, n_r):
    """n_f f terms with k = 1, 3, 16 in turn, every other one with a numerator column, and n_r ranges with windows inside the rows"""
    q = Q[field]
    f = rs.poison_rows(rng, field, n, 20)
    m = rs.poison_rows(rng, field, n, 8)
    terms = []
    for u in range(n_f):
        k = (1, 3, 16)[u % 3]
        terms.append(("f", [(u + 5 * j) % 19 for j in range(k)], ("f", 19) if u % 2 else None, rng.choice((1, q - 1, 5)), rng.randrange(q)))
    ranges = []
    for r in range(n_r):
        row0 = rng.randrange(n // 2)
        ranges.append(("m", r, rng.randrange(-50, 1 << 30), rng.randrange(1, n - row0 + 1), row0, rng.choice((q - 1, 1)), rng.randrange(q)))
    return {"f": f, "m": m}, terms, ranges


SHAPES = {
    "nine singletons": (8, 1, [0, 1, 2, 3, 4, 5, 6, 7, 8]),
    "one cluster of nine": (5, 4, [0] * 9),
    "pairs and one direct": (6, 3, [0, 0, 1, 1, 2, 2, 3, 3, D]),
    "all but one direct": (5, 4, [D, D, D, D, D, D, 0, D, D]),
    "out of order, interleaved": (5, 4, [2, 0, D, 1, 0, 1, 2, D, 0]),
    "the range table's AIR": (0, 8, [0, 0, 1, 1, 2, 2, 3, 3]),
    "eight f and a range": (8, 1, [0, 1, 0, 1, D, 2, 2, 2, 1]),
}


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_cluster_shapes(field, shape):
    """more than one lane and wave of rows, not a multiple of the lane's eight"""
    n_f, n_r, cluster = SHAPES[shape]
    rng = random.Random(shape)
    n = 77
    mats, terms, ranges = nine(field, rng, n, n_f, n_r)
    one_matrix_case(field, rng, n, terms, ranges, cluster, mats)


@pytest.mark.parametrize("field,n", [("gl", 2049), ("bn128", 1025)])
def test_many_groups_across_blocks(field, n):
    """out-of-order, interleaved ids with a DIRECT part past a block's edge: the im stores of a second block (a further level over Fr)
    together with many groups"""
    n_f, n_r, cluster = SHAPES["out of order, interleaved"]
    rng = random.Random(n)
    mats, terms, ranges = nine(field, rng, n, n_f, n_r)
    one_matrix_case(field, rng, n, terms, ranges, cluster, mats, host_form=False)


@pytest.mark.parametrize("field", FIELDS)
def test_zero_denominators(field):
    """base-valued challenges, so that chosen column values give D = 0: one term of cluster 0 zero at rows where its other terms are not --
    a lane's first and last row among them; every term of cluster 1 zero at a row, so im_1 = 0 there; a zero in the DIRECT term; a zero E
    inside a window"""
    rng = random.Random(field)
    n, q = 41, Q[field]
    a0, b0 = 1 + rng.randrange(q - 1), rng.randrange(q)
    alpha, beta = ((a0, 0, 0), (b0, 0, 0)) if field == "gl" else (a0, b0)
    buses = [rng.randrange(q) for _ in range(5)]
    f = rs.rand_rows(rng, field, n, 6)
    zero_at = {0: (0, 7, 8, 15, 16, 30), 1: (30,), 2: (9, 23), 3: (9, 31), 4: (5, 16)}
    for u, rows in zero_at.items():
        for i in rows:
            f[i][u] = rs.pattern_of(field, -(buses[u] + b0) * pow(a0, q - 2, q))
    m = rs.poison_rows(rng, field, n, 1)
    lo, row0, j = 1000, 4, 12
    bus_r = -((lo + j) * a0 + b0) % q                                         # E zero at row row0 + j = 16, a lane's first row
    terms = [("f", [u], ("f", 5) if u % 2 else None, 1 + u, buses[u]) for u in range(5)]
    ranges = [("m", 0, lo, 30, row0, q - 1, bus_r)]
    cluster = [0, 0, 1, 1, D, 0]
    rows, cols = out_matrix(field, n, 2)
    s, im = run(field, {"f": f, "m": m, "$o": rows}, terms, ranges, cluster, [("$o", cols[1]), ("$o", cols[2])], alpha, beta, n, ("$o", cols[0]))
    zero = lref.FIELDS[field].zero
    assert im[1][9] == zero and im[1][8] != zero and im[0][16] != zero and im[0][30] != zero


WINDOWS = {"gl": (4097, ((8, 2048), (2048, 4097)), ((7, 2047), (2049, 4096))), "bn128": (1025, ((8, 256), (256, 1025)), ((7, 255), (257, 1024)))}


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("which", (1, 2))
def test_windows(field, which):
    """two ranges of ONE cluster with disjoint windows whose ends fall on lane and block edges (and one row off them), beside an f term"""
    rng = random.Random(which)
    q = Q[field]
    n = WINDOWS[field][0]
    (s0, e0), (s1, e1) = WINDOWS[field][which]
    m = rs.poison_rows(rng, field, n, 2)
    f = rs.rand_rows(rng, field, n, 1)
    ranges = [("m", 0, -5, e0 - s0, s0, q - 1, 7), ("m", 1, 1 << 40, e1 - s1, s1, q - 1, 8)]
    one_matrix_case(field, rng, n, [("f", [0], None, 1, 7)], ranges, [D, 0, 0], {"f": f, "m": m}, host_form=False)


@pytest.mark.parametrize("field", FIELDS)
@pytest.mark.parametrize("where", ("beside t", "apart", "descending"))
def test_placement(field, where):
    rng = random.Random(where)
    n, q = 19, Q[field]
    width = 3 if field == "gl" else 1
    t = rs.rand_rows(rng, field, n, 3 + 3 * width + 1)                         # the tuple columns 0 .. 2, then room for s and two im columns
    m = rs.poison_rows(rng, field, n, 1)
    terms = [("t", [0, 1], None, 1, 2), ("t", [2], None, q - 1, 2)]
    ranges = [("m", 0, 3, n - 2, 1, q - 1, 9)]
    mats = {"t": t, "m": m}
    if where == "beside t":                          # s and all im columns as neighbouring columns of t's matrix
        out, im = ("t", 3), [("t", 3 + width), ("t", 3 + 2 * width)]
    elif where == "descending":                      # one matrix, the im columns in descending column order, s between them
        mats["$o"] = out_matrix(field, n, 2)[0]
        cols = out_matrix(field, n, 2)[1]
        out, im = ("$o", cols[1]), [("$o", cols[2]), ("$o", cols[0])]
    else:                                            # each output in a matrix of its own with a different stride
        for o in range(3):
            mats["$%d" % o] = [[(0xA0 + o << 32) + 5 * i + j for j in range(width + 1 + o)] for i in range(n)]
        out, im = ("$0", 0), [("$1", 1), ("$2", 2)]
    run(field, mats, terms, ranges, [1, 0, 1], im, rs.rand_chal(rng, field), rs.rand_chal(rng, field), n, out)


@pytest.mark.parametrize("field", FIELDS)
def test_range_logup_clustered(field):
    """both halves of the prove side: range_mult_dev's m, then s and one im column; a clean check sums to zero"""
    n, lo, size = 64, -3, 40
    width = 3 if field == "gl" else 1
    rng = random.Random(5)
    vals = [[rs.pattern_of(field, lo + rng.randrange(size)) for _ in range(2)] for _ in range(n)]
    cm1 = rs.to_dev(rs.words(field, [row + [0] for row in vals]))
    cm2 = torch.zeros((n, 2 * width) if field == "gl" else (n, 2, 4), dtype=torch.int64, device="cuda")
    a, b = rs.chal_words(field, rs.chal_pattern(field, rs.rand_chal(rng, field))), rs.chal_words(field, rs.chal_pattern(field, rs.rand_chal(rng, field)))
    report, last = pilcheck.range_logup_clustered([(cm1, [0]), (cm1, [1])], lo, size, (cm1, 2), [0, 0, DIRECT], [(cm2, width)], a, b, (cm2, 0), n, field)
    assert report[0] == 0 and not last.any()
