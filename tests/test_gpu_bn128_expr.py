"""BN254 Fr expression evaluator on the device (pil2gl.bn128.eval_program / first_nonzero_row over csrc/bn_expr.hip) against the Python
checker (tests/bn128_expr_ref.py: Python integers mod r and a row loop written from the reference's compileCode / getRef / evalMap).
Every comparison is exact equality of the 64-bit words; nothing here has a tolerance.  Which kernel form ran, and the launch geometry,
are asked of the library's planner hook, never restated."""
import random

import numpy as np
import pytest

import bn128_expr_ref as ref
import bn128_fft_ref as fref
import bn128_g1_ref as g1
from bn128_expr_ref import R, ADD, SUB, MUL, COPY, tmp, sec, scalar

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def bn():
    import pil2gl
    from pil2gl import bn128
    pil2gl.init(0)
    return bn128


def dev(words):
    return torch.from_numpy(np.ascontiguousarray(words).view(np.int64)).cuda()


def host(t):
    return t.cpu().numpy().view(np.uint64)


def check(bn, ops, sections, scalars, n_bits, prime_shift=0, form=None, threads=None):
    """runs ops on copies of `sections` ([row][column] Montgomery integers) on the device and in the checker; every section must come out
    equal, the untouched ones included.  form / threads: what the planner hook must say ran."""
    sc = ref.words_of(scalars) if scalars else np.zeros((0, 4), np.uint64)
    plan = bn.plan_program(ops, [len(s[0]) for s in sections], sc, n_bits, prime_shift)
    if form is not None:
        assert plan["form"] == form, plan
    if threads is not None:
        assert plan["threads"] == threads, plan
    d = [dev(ref.section_words(s)) for s in sections]
    bn.eval_program(ops, d, sc, n_bits, prime_shift)
    want = [[list(row) for row in s] for s in sections]
    ref.evaluate(ops, want, scalars, n_bits, prime_shift)
    for k, (got, w) in enumerate(zip(d, want)):
        g = host(got)
        assert g.shape == (len(w), len(w[0]), 4)
        bad = np.argwhere((g != ref.section_words(w)).any(axis=2))
        assert bad.size == 0, "section %d differs first at (row, column) %s" % (k, bad[0])
    return plan


# ---- arithmetic: each op alone on the cross product of chosen stored values -------------------------------------------------------
MONT = 1 << 256
ALL_ONES_BELOW_TOP = (0x30644e71 << 224) | ((1 << 224) - 1)              # seven limbs of ones under a top limb one below r's: < r
X = random.Random(254).randrange(2, R - 2)
CHOSEN = [0, 1, R - 1, R - 2, (R - 1) // 2, (R + 1) // 2, MONT % R, MONT * MONT % R, ALL_ONES_BELOW_TOP,
          X, R - X, R - 1 - X, X + 1,                                    # with X: a + b = r, a + b = r - 1, a = b - 1; a = b is the diagonal
          2, R - ALL_ONES_BELOW_TOP, random.Random(255).randrange(R)]


def test_chosen_values_are_what_they_claim():
    """pins the test's own operands, not the library: it needs no new symbol (and no device work)"""
    assert len(CHOSEN) == 16 and len(set(CHOSEN)) == 16 and all(0 <= v < R for v in CHOSEN)
    limbs = [(ALL_ONES_BELOW_TOP >> (32 * k)) & 0xFFFFFFFF for k in range(8)]
    assert limbs[:7] == [0xFFFFFFFF] * 7
    assert X + (R - X) == R and X + (R - 1 - X) == R - 1 and X == (X + 1) - 1


@pytest.mark.parametrize("op", (ADD, SUB, MUL, COPY), ids=("add", "sub", "mul", "copy"))
def test_each_op_on_the_cross_product_of_chosen_values(bn, op):
    a = [[x] for x in CHOSEN for _ in CHOSEN]
    b = [[y] for _ in CHOSEN for y in CHOSEN]
    out = [[7] for _ in range(256)]
    check(bn, [(op, sec(2), sec(0), sec(1) if op != COPY else None)], [a, b, out], [], 8, form=0)


def test_outputs_are_canonical(bn):
    """sums and differences that land on r - 1, 0 and 1, and products of the largest elements: every output word below r"""
    a = [[R - 1, R - 1, 1, 0, (R + 1) // 2, R - 1]]
    b = [[0, 1, R - 1, 0, (R - 1) // 2, R - 1]]
    ops = [(ADD, sec(2, j), sec(0, j), sec(1, j)) for j in range(6)] + [(SUB, sec(3, j), sec(0, j), sec(1, j)) for j in range(6)] + \
          [(MUL, sec(4, j), sec(0, j), sec(1, j)) for j in range(6)]
    d = [dev(ref.section_words(s)) for s in (a, b, [[0] * 6], [[0] * 6], [[0] * 6])]
    bn.eval_program(ops, d, np.zeros((0, 4), np.uint64), 0)
    for t in d[2:]:
        assert all(v < R for v in ref.ints_of(host(t)))
    assert ref.ints_of(host(d[2])) == [R - 1, 0, 0, 0, 0, R - 2]


# ---- row offsets -----------------------------------------------------------------------------------------------------------------
def test_row_offsets_on_domain_n(bn):
    rng = random.Random(1)
    a, out, shifted = ref.random_section(rng, 8, 2), [[0, 0, 0] for _ in range(8)], [[0] for _ in range(8)]
    ops = [(SUB, sec(1, 0), sec(0, 0, -1), sec(0, 0, 1)),
           (MUL, sec(1, 1), sec(0, 1, 3), sec(0, 0)),
           (ADD, tmp(0), sec(0, 1, -1), sec(0, 1, 1)), (COPY, sec(1, 2), tmp(0), None),
           (ADD, sec(2, 0, 1), sec(0, 0), sec(0, 1, 3))]                              # a destination with prime = +1
    check(bn, ops, [a, out, shifted], [], 3)
    check(bn, [(COPY, sec(2, 0, -1), sec(0, 0, 3), None), (COPY, sec(1, 1, 3), sec(0, 1, -1), None)], [a, out, shifted], [], 3)


def test_row_offsets_on_domain_ext_wrap_at_both_ends(bn):
    rng = random.Random(2)
    a, out = ref.random_section(rng, 32, 1), [[0, 0, 0] for _ in range(32)]
    # nBits = 5, primeShift = 2: prime +1 reads four rows ahead (rows 28..31 wrap to 0..3), prime -1 four rows back (rows 0..3 wrap to 28..31)
    ops = [(COPY, sec(1, 0), sec(0, 0, 1), None), (COPY, sec(1, 1), sec(0, 0, -1), None), (SUB, sec(1, 2, -1), sec(0, 0, 1), sec(0, 0, -1))]
    check(bn, ops, [a, out], [], 5, 2)
    assert ref.row_index(30, 1, 5, 2) == 2 and ref.row_index(1, -1, 5, 2) == 29


@pytest.mark.parametrize("n_bits", (0, 1))
def test_smallest_domains(bn, n_bits):
    rng = random.Random(3 + n_bits)
    a, out = ref.random_section(rng, 1 << n_bits, 2), [[0, 0] for _ in range(1 << n_bits)]
    ops = [(MUL, sec(1, 0), sec(0, 0, 1), sec(0, 1, -1)), (ADD, sec(1, 1, 1), sec(0, 0), scalar(0))]
    check(bn, ops, [a, out], [rng.randrange(R)], n_bits)


# ---- operand kinds ---------------------------------------------------------------------------------------------------------------
def test_every_operand_kind_as_first_and_second_source(bn):
    rng = random.Random(4)
    one, five, out = ref.random_section(rng, 16, 1), ref.random_section(rng, 16, 5), [[0] * 4 for _ in range(16)]
    ops = [(SUB, tmp(0), sec(0), scalar(0)),               # section - scalar          (width 1)
           (SUB, tmp(1), scalar(1), sec(1, 4)),            # scalar - section          (width 5, column 4)
           (SUB, tmp(2), tmp(0), sec(1, 4)),               # tmp - section
           (SUB, tmp(3), sec(0), tmp(1)),                  # section - tmp
           (SUB, tmp(4), tmp(2), scalar(1)),               # tmp - scalar
           (SUB, tmp(5), scalar(0), tmp(3)),               # scalar - tmp
           (MUL, tmp(6), tmp(4), tmp(5)),                  # tmp * tmp, destination tmp
           (SUB, sec(2, 0), scalar(0), scalar(1)),         # scalar - scalar, destination section
           (COPY, sec(2, 1), tmp(6), None), (COPY, sec(2, 2), scalar(1), None), (COPY, sec(2, 3), sec(1, 4), None)]
    check(bn, ops, [one, five, out], [rng.randrange(R), rng.randrange(R)], 4)


def test_source_and_destination_in_one_section_and_in_place(bn):
    rng = random.Random(5)
    s = ref.random_section(rng, 16, 5)
    ops = [(MUL, sec(0, 3), sec(0, 0, 1), sec(0, 1, -1)),                   # other columns of the section it writes, with offsets
           (MUL, sec(0, 4), sec(0, 4), sec(0, 4)),                           # x = x * x in place
           (ADD, sec(0, 2), sec(0, 2), sec(0, 4)),                           # reads what the op before wrote
           (MUL, sec(0, 4), sec(0, 4), sec(0, 2))]                           # and writes it once more
    check(bn, ops, [s], [], 4)


# ---- the boundary between the two kernel forms -----------------------------------------------------------------------------------
def test_live_temporaries_at_the_lds_limit_and_one_above(bn):
    rng = random.Random(6)
    limit = bn.plan_program(ref.live_program(1), [1, 1], np.zeros((0, 4), np.uint64), 6)["ldsSlotLimit"]
    for k, form in ((limit, 0), (limit + 1, 1)):
        plan = check(bn, ref.live_program(k), [ref.random_section(rng, 64, k), [[0] for _ in range(64)]], [], 6, form=form)
        assert plan["slots"] == k


@pytest.mark.parametrize("seed", (11, 12))
@pytest.mark.parametrize("hold,form", ((0, 0), (40, 1)), ids=("lds", "global"))
def test_random_programs_through_both_forms(bn, seed, hold, form):
    rng = random.Random(seed)
    ops = ref.random_program(seed, 300, in_width=5, n_scalars=4, hold=hold, primes=(0, 0, 1, -1))
    assert 300 <= len(ops) <= 360
    a, out = ref.random_section(rng, 64, 5), [[0] for _ in range(64)]
    check(bn, ops, [a, out], [rng.randrange(R) for _ in range(4)], 6, form=form)


# ---- launch geometry -------------------------------------------------------------------------------------------------------------
THREE_OPS = [(MUL, tmp(0), sec(0, 0), sec(0, 1, 1)), (ADD, tmp(1), tmp(0), scalar(0)), (SUB, sec(1), tmp(1), sec(0, 0, -1))]


@pytest.mark.parametrize("n_bits", (5, 8, 9), ids=("below one workgroup", "exactly one workgroup", "twice one workgroup"))
def test_row_counts_around_one_workgroup(bn, n_bits):
    rng = random.Random(20 + n_bits)
    check(bn, THREE_OPS, [ref.random_section(rng, 1 << n_bits, 2), [[0] for _ in range(1 << n_bits)]], [rng.randrange(R)], n_bits, form=0, threads=256)


def test_one_workgroup_plus_one_wave(bn):
    """row counts are powers of two, so a workgroup and one wave more exist only where the workgroup is one wave: a program with 16 live
    temporaries runs in workgroups of 64 lanes, and 2^7 rows are one of them plus a wave"""
    rng = random.Random(23)
    check(bn, ref.live_program(16), [ref.random_section(rng, 128, 16), [[0] for _ in range(128)]], [], 7, form=0, threads=64)


def test_grid_stride_loop_takes_a_second_turn(bn):
    """the smallest power of two above the lanes of one launch: every lane evaluates two rows"""
    sc = [random.Random(24).randrange(R)]
    lanes = bn.plan_program(THREE_OPS, [2, 1], ref.words_of(sc), 4)["lanesPerLaunch"]
    n_bits = lanes.bit_length()
    assert (1 << n_bits) > lanes >= (1 << (n_bits - 1)) and n_bits <= 19
    n = 1 << n_bits
    # inputs with a structure the checker can afford: random words from numpy, canonical because the top word stays below r's
    rs = np.random.default_rng(25)
    w = rs.integers(0, 1 << 64, size=(n, 2, 4), dtype=np.uint64)
    w[:, :, 3] %= np.uint64(0x30644e72e131a029)
    a = ref.section_of(w)
    d = [dev(w), torch.zeros((n, 1, 4), dtype=torch.int64, device="cuda")]
    bn.eval_program(THREE_OPS, d, ref.words_of(sc), n_bits)
    want = [a, [[0] for _ in range(n)]]
    ref.evaluate(THREE_OPS, want, sc, n_bits)
    assert (host(d[1]) == ref.section_words(want[1])).all() and (host(d[0]) == w).all()


# ---- stream order and residency --------------------------------------------------------------------------------------------------
def test_ifft_eval_fft_msm_on_one_stream_without_synchronisation(bn):
    n_bits, n = 6, 64
    rng = random.Random(30)
    cols = [[rng.randrange(R) for _ in range(n)] for _ in range(2)]                # normal form, two polynomials by their evaluations
    blind = rng.randrange(R)
    points, logs = g1.known_log_bases(n, seed=31)
    ops = [(MUL, tmp(0), sec(0, 0), sec(0, 1, 1)), (ADD, sec(1, 1), tmp(0), scalar(0)), (COPY, sec(1, 0), sec(0, 1), None)]
    x = dev(fref.matrix_words(cols))
    bases = dev(g1.point_words(points))
    res = torch.zeros((n, 2, 4), dtype=torch.int64, device="cuda")
    sc = ref.words_of([ref.to_mont(blind)])
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        coefs = bn.ifft(x, 2, n_bits)
        bn.eval_program(ops, [coefs, res], sc, n_bits)
        evals = bn.fft(res, 2, n_bits)
        commit = bn.g1_msm(bases, evals.reshape(-1)[4:], n, stride=2)          # column 1 of the transformed result, by stride: no gather
    side.synchronize()
    # the same chain in the checker
    c = [fref.intt(col) for col in cols]
    secs = [[[ref.to_mont(c[0][j]), ref.to_mont(c[1][j])] for j in range(n)], [[0, 0] for _ in range(n)]]
    ref.evaluate(ops, secs, [ref.to_mont(blind)], n_bits)
    assert (host(res) == ref.section_words(secs[1])).all()
    out_cols = [fref.ntt([ref.from_mont(row[k]) for row in secs[1]]) for k in range(2)]
    assert (host(evals) == fref.matrix_words(out_cols)).all()
    assert (host(commit) == g1.point_words([g1.expected_from_logs(out_cols[1], logs)]).reshape(8)).all()


# ---- first non-zero row ------------------------------------------------------------------------------------------------------------
def column(n, width, col, values):
    rows = [[0] * width for _ in range(n)]
    for r, v in values.items():
        rows[r][col] = v
    return rows


@pytest.mark.parametrize("name,values,first,last,want", (
    ("none", {}, 0, 300, None),
    ("row 0", {0: 5}, 0, 300, 0),
    ("the last row", {299: 5}, 0, 300, 299),
    ("only outside the range", {3: 5, 290: 6}, 4, 290, None),
    ("two rows, the smaller wins", {200: 5, 70: 6}, 0, 300, 70),
    ("two rows in one wave", {131: 5, 129: 6}, 100, 300, 129),
    ("only the top 32-bit word", {17: 1 << 224}, 0, 300, 17),
    ("only the fifth 32-bit word", {18: 1 << 128}, 0, 300, 18),
))
def test_first_nonzero_row(bn, name, values, first, last, want):
    rows = column(300, 3, 1, values)
    for r in rows:                                       # the neighbouring columns are never zero: only the asked column decides
        r[0], r[2] = 9, 1 << 200
    got = bn.first_nonzero_row(dev(ref.section_words(rows)), 1, first, last)
    if want is None:
        assert got is None
    else:
        assert got[0] == want and ref.ints_of(got[1]) == [values[want]]


def test_first_failing_row_of_a_constraint(bn):
    """the debug path end to end: a constraint a' = a * a that row 41 breaks, evaluated into a column and searched on its boundary"""
    n_bits, n = 6, 64
    a = [[ref.to_mont(3)]]
    for _ in range(n - 1):
        a.append([ref.f_mul(a[-1][0], a[-1][0])])
    a[42][0] = (a[42][0] + 1) % R
    ops = [(MUL, tmp(0), sec(0), sec(0)), (SUB, sec(1), sec(0, 0, 1), tmp(0))]
    d = [dev(ref.section_words(a)), torch.zeros((n, 1, 4), dtype=torch.int64, device="cuda")]
    bn.eval_program(ops, d, np.zeros((0, 4), np.uint64), n_bits)
    row, val = bn.first_nonzero_row(d[1], 0, 0, n - 1)                      # everyFrame with offsetMax = 1: the wrap row is not checked
    assert row == 41 and ref.ints_of(val) == [1]
    assert bn.first_nonzero_row(d[1], 0, 0, 41) is None and bn.first_nonzero_row(d[1], 0, 43, n - 1) is None
