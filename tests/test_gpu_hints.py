"""The Goldilocks stage-2 hints on the device (csrc/hints.hip: pil2gl_gprod_dev, pil2gl_gsum_dev, pil2gl_h1h2_dev) at the places the random
columns of test_gpu_parity.py do not reach: the lane and block edges of the scan, a second pass whose lanes walk several block totals,
zero denominators wherever one can sit, extension denominators that only look like zero or like base elements, words at the 32-bit carry
edges of the reduction, a small call after a large one in the grow-only scratch, and for h1h2 forced probe chains, keys that differ in one
word, the row of a missing value, duplicates over a boundary of the scan of the group starts.
Every comparison is exact equality of words.  The reference is the C oracle (oracle/gl_oracle.c; h1h2: its literal restatement of the
reference); every case of at most 4096 rows is compared with tests/hints_ref.py as well, Python integers written from the definitions, so
that oracle and kernel cannot share a mistake.  Every call goes through scan() or lookup(): the C entries with caller-owned outputs
between guard words; the outputs equal the reference, are n or 3 n words long, the guard words and the inputs on the device come back
unchanged.  The thresholds are asked of the library (pil2gl.hint_plan), never typed in: C = rows a block, I = rows a lane."""
import numpy as np
import pytest

import hints_ref as href
from conftest import P, rand_field

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
from pil2gl import _lib  # noqa: E402
import pil2gl  # noqa: E402

GUARD = 0xFFFFFFFFDEADBEEF                            # above p: no output word
NG = 16                                               # guard words on either side of an output
EINVAL = -1
PLAN = pil2gl.hint_plan(1)
C_, I_, T_ = PLAN["chunk"], PLAN["items"], PLAN["threads"]
DIMS = [(1, 1), (1, 3), (3, 1), (3, 3)]
OPS = ("gprod", "gsum")
EDGE = [1, 2, P - 1, P - 2, (1 << 32) - 1, 1 << 32, (1 << 32) + 1, P - (1 << 32), 1 << 63]       # the 32-bit carry edges of the reduction


@pytest.fixture(scope="module")
def lib():
    pil2gl.init(0)
    return _lib.load()


def test_the_plan_is_the_one_these_shapes_assume():
    assert C_ == T_ * I_ and I_ >= 2 and C_ > 2 * I_ + 37
    assert all(pil2gl.hint_plan(n)["blocks"] == b for n, b in ((C_, 1), (C_ + 1, 2), (2 * C_ + 1, 3), (3 * C_ + 37, 4)))


# ---- the common call helpers ----
def to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).reshape(-1).view(np.int64)).cuda()


def to_host(d):
    return d.cpu().numpy().view(np.uint64)


def guarded(words):
    return to_dev(np.full(words + 2 * NG, GUARD, np.uint64))


def check_guarded(buf, want, what):
    got = to_host(buf)
    assert got.size == want.size + 2 * NG
    assert np.array_equal(got[NG:NG + want.size], want), what + ": the output differs from the reference"
    assert (got[:NG] == GUARD).all() and (got[NG + want.size:] == GUARD).all(), what + ": a guard word was written"


def stream():
    return torch.cuda.current_stream().cuda_stream


def nonzero(den):
    den[~den.any(axis=1)] = 1
    return den


def scan(lib, oracle, op, num, den, dim_num, dim_den, alias=False):
    """one call of pil2gl_gprod_dev / pil2gl_gsum_dev: num (n rows; ONE row for gsum) and den (n rows) as (rows, dim) arrays; alias: num is
    den's own device buffer -> the reference's words as (n, dimOut)"""
    n, dim_out = den.shape[0], max(dim_num, dim_den)
    assert num.shape == ((n if op == "gprod" else 1), dim_num) and den.shape == (n, dim_den)
    want = getattr(oracle, op)(num, den, dim_num, dim_den)
    assert want.size == n * dim_out, "n words for dimension 1, 3 n for dimension 3"
    if n <= 4096:
        assert want.tolist() == getattr(href, op)(num, dim_num, den, dim_den), "the oracle and the restatement disagree"
    d_den = to_dev(den)
    d_num = d_den if alias else to_dev(num)
    out = guarded(n * dim_out)
    rc = getattr(lib, "pil2gl_%s_dev" % op)(d_num.data_ptr(), dim_num, d_den.data_ptr(), dim_den, n, out.data_ptr() + 8 * NG, stream())
    assert rc == 0, lib.pil2gl_last_error()
    check_guarded(out, want, "%s n = %d dims (%d, %d)" % (op, n, dim_num, dim_den))
    assert np.array_equal(to_host(d_num), num.reshape(-1)) and np.array_equal(to_host(d_den), den.reshape(-1)), "an input was written"
    return want.reshape(n, dim_out)


def both(lib, oracle, num, den, dim_num, dim_den):
    """the product and, with num's first row as the one numerator, the sum"""
    return scan(lib, oracle, "gprod", num, den, dim_num, dim_den), scan(lib, oracle, "gsum", num[:1], den, dim_num, dim_den)


def keys_of(a, dim):
    return [int(r[0]) for r in a] if dim == 1 else [tuple(int(x) for x in r) for r in a]


def lookup(lib, oracle, f, t, dim, bufs=None, missing=None):
    """one call of pil2gl_h1h2_dev: f, t as (n, dim) arrays; bufs: the device buffers of an earlier call, used again; missing: the row the
    refusal must name -> the device buffers"""
    n = t.shape[0]
    assert f.shape == t.shape == (n, dim)
    kf, kt = keys_of(f, dim), keys_of(t, dim)
    if missing is None:
        w1, w2 = oracle.h1h2(kf, kt)
        if n <= 4096:
            assert href.h1h2(kf, kt) == (w1, w2), "the oracle and the restatement disagree"
        w1, w2 = (np.array(w, np.uint64).reshape(-1) for w in (w1, w2))
        assert w1.size == w2.size == n * dim
    else:
        for ref in (oracle.h1h2, href.h1h2):
            with pytest.raises(ValueError, match="Number not included: w:%d$" % missing):
                ref(kf, kt)
    if bufs is None:
        bufs = {"f": to_dev(f), "t": to_dev(t), "h1": guarded(n * dim), "h2": guarded(n * dim)}
    else:
        bufs["f"].copy_(to_dev(f)); bufs["t"].copy_(to_dev(t))
        bufs["h1"].copy_(guarded(n * dim)); bufs["h2"].copy_(guarded(n * dim))
    rc = lib.pil2gl_h1h2_dev(bufs["f"].data_ptr(), bufs["t"].data_ptr(), n, dim, bufs["h1"].data_ptr() + 8 * NG, bufs["h2"].data_ptr() + 8 * NG, stream())
    if missing is None:
        assert rc == 0, lib.pil2gl_last_error()
        check_guarded(bufs["h1"], w1, "h1 n = %d dim %d" % (n, dim))
        check_guarded(bufs["h2"], w2, "h2 n = %d dim %d" % (n, dim))
    else:
        msg = lib.pil2gl_last_error().decode()
        assert rc == EINVAL and "Number not included" in msg and msg.endswith("w:%d" % missing), (rc, msg)
        for h in ("h1", "h2"):
            got = to_host(bufs[h])
            assert (got[:NG] == GUARD).all() and (got[NG + n * dim:] == GUARD).all(), "a guard word was written"
    assert np.array_equal(to_host(bufs["f"]), f.reshape(-1)) and np.array_equal(to_host(bufs["t"]), t.reshape(-1)), "an input was written"
    return bufs


def columns(seed, n, dim_num, dim_den):
    rng = np.random.default_rng(seed)
    return rand_field(rng, (n, dim_num)), nonzero(rand_field(rng, (n, dim_den)))


def sub3(a, b):
    return tuple((int(x) - int(y)) % P for x, y in zip(a, b))


# ---- the running product and sum ----
@pytest.mark.parametrize("dim_num,dim_den", DIMS)
@pytest.mark.parametrize("n", [1, 2, I_ - 1, I_, I_ + 1, C_ - 1, C_, C_ + 1, 2 * C_ - 1, 2 * C_ + 1])
def test_lane_and_block_edges(lib, oracle, n, dim_num, dim_den):
    num, den = columns(n * 16 + dim_num * 4 + dim_den, n, dim_num, dim_den)
    both(lib, oracle, num, den, dim_num, dim_den)


TOTALS_PER_LANE = {T_: 1, T_ + 1: 2, 2 * T_: 2, 2 * T_ + 1: 3}
SEVERAL = [(nb, tail, dim) for nb in TOTALS_PER_LANE for tail in (1, C_) for dim in (3, 1) if dim == 3 or nb % T_ == 1]


@pytest.mark.parametrize("nb,tail,dim", SEVERAL)
def test_several_totals_per_lane(lib, oracle, nb, tail, dim):
    """the second pass with runs of 1, 2 and 3 block totals a lane, the last block one row or full; then one zero denominator in block
    nb - 2: the sum's later blocks still carry the prefix, the product's are 0"""
    n = (nb - 1) * C_ + tail
    plan = pil2gl.hint_plan(n)
    assert plan["blocks"] == nb and plan["totalsPerLane"] == TOTALS_PER_LANE[nb]
    num, den = columns(nb * 2 + dim + tail, n, dim, dim)
    z, s = both(lib, oracle, num, den, dim, dim)
    zero = (nb - 2) * C_ + 5
    dz = den.copy()
    dz[zero] = 0
    zz, sz = both(lib, oracle, num, dz, dim, dim)
    assert np.array_equal(zz[:zero + 1], z[:zero + 1]) and not zz[zero + 1:].any() and zz[zero].any(), "the reference: the product is 0 after the zero row"
    pad = (0,) * (3 - dim)
    ratio = sub3(tuple(s[zero]) + pad, tuple(s[zero - 1]) + pad)
    assert np.array_equal(sz[:zero], s[:zero]) and np.array_equal(sz[zero], sz[zero - 1])
    for row in ((nb - 1) * C_, n - 1):                   # the last block's first and last row
        assert tuple(int(v) for v in sz[row]) + pad == sub3(tuple(s[row]) + pad, ratio) and sz[row].any(), "the reference: the sum goes on without that ratio"


def zero_rows(n):
    j = C_ // I_ + 44                                    # a lane batch inside block 1
    return {"row 0": [0], "the last row": [n - 1], "first of a batch": [I_ * j], "last of a batch": [I_ * j + I_ - 1], "a block boundary": [C_ - 1, C_],
            "a whole batch": list(range(I_ * j, I_ * j + I_)), "a whole block": list(range(C_, 2 * C_)), "every row": list(range(n))}


@pytest.mark.parametrize("dim", [3, 1])
@pytest.mark.parametrize("where", list(zero_rows(3 * C_ + 37)))
def test_zero_placement(lib, oracle, where, dim):
    n = 3 * C_ + 37
    rows = zero_rows(n)[where]
    num, den = columns(77 + dim, n, dim, dim)
    z, s = oracle.gprod(num, den, dim, dim).reshape(n, dim), oracle.gsum(num[:1], den, dim, dim).reshape(n, dim)
    dz = den.copy()
    dz[rows] = 0
    zz, sz = both(lib, oracle, num, dz, dim, dim)
    first = rows[0]
    assert np.array_equal(zz[:first + 1], z[:first + 1]) and not zz[first + 1:].any(), "the reference: equal up to the first zero row, 0 after it"
    assert zz[first].any() and np.array_equal(sz[:first], s[:first])
    for r in rows[:3] + rows[-3:]:
        assert np.array_equal(sz[r], sz[r - 1]) if r else not sz[0].any(), "the reference: a zero denominator adds nothing"


@pytest.mark.parametrize("dim", [3, 1])
@pytest.mark.parametrize("n,rows", [(1, [0]), (5, [0, 4]), (I_, list(range(I_)))])
def test_zeros_in_a_one_block_column(lib, oracle, n, rows, dim):
    num, den = columns(n + dim, n, dim, dim)
    den[rows] = 0
    z, s = both(lib, oracle, num, den, dim, dim)
    assert z[0].tolist() == [1, 0, 0][:dim] and not z[1:].any() and not s[0].any()


@pytest.mark.parametrize("dim_num", [3, 1])
def test_extension_denominators_that_only_look_like_zero(lib, oracle, dim_num):
    """non-zero elements with zero words, v[0] = 0 among them, beside one true zero in the same lane batch and on a block boundary"""
    n = C_ + 37
    num, den = columns(31 + dim_num, n, dim_num, 3)
    x = P - 5
    b = 3 * I_
    den[b], den[b + 1], den[b + 2] = (0, x, 0), (0, 0, x), (x, 0, 0)
    den[C_ - 1], den[C_] = (0, 0, 7), (0, 1 << 32, 0)
    _, s0 = both(lib, oracle, num, den, dim_num, 3)
    den[b + 3] = 0
    z, s = both(lib, oracle, num, den, dim_num, 3)
    assert z[b + 3].any() and not z[b + 4:].any(), "the reference: only the true zero ends the product"
    assert np.array_equal(s[b + 3], s[b + 2]) and np.array_equal(s[:b + 3], s0[:b + 3])
    for r in (b, b + 1, b + 2, C_ - 1, C_):
        assert not np.array_equal(s[r], s[r - 1]), "the reference: row %d adds a ratio" % r


@pytest.mark.parametrize("dim_num", [3, 1])
def test_extension_column_of_base_values(lib, oracle, dim_num):
    """every lane batch's product is a base element: the base inversion; then one true extension element, whose batch alone takes the
    extension inversion; then a zero beside it"""
    n = C_ + 37
    num, den = columns(41 + dim_num, n, dim_num, 3)
    den[:, 1:] = 0
    den[den[:, 0] == 0, 0] = 1
    z, _ = both(lib, oracle, num, den, dim_num, 3)
    assert dim_num == 3 or not z[:, 1:].any()
    den[5 * I_ + 3] = (3, P - 1, 1 << 32)
    both(lib, oracle, num, den, dim_num, 3)
    den[5 * I_ + 4] = 0
    den[6 * I_] = 0
    both(lib, oracle, num, den, dim_num, 3)


def edge_column(dim):
    if dim == 1:
        return np.array([[EDGE[k % 9]] for k in range(54)], np.uint64)
    rows = []
    for k, v in enumerate(EDGE):
        for pos in range(3):
            lone = [0, 0, 0]
            lone[pos] = v
            full = [EDGE[(k + 1) % 9], EDGE[(k + 2) % 9], EDGE[(k + 4) % 9]]
            full[pos] = v
            rows += [lone, full]
    return np.array(rows, np.uint64)


@pytest.mark.parametrize("dim_num,dim_den", DIMS)
def test_chosen_words_at_the_carry_edges(lib, oracle, dim_num, dim_den):
    den = edge_column(dim_den)
    n = den.shape[0]
    assert n == 54 and (den < P).all()
    both(lib, oracle, rand_field(np.random.default_rng(dim_num + 2 * dim_den), (n, dim_num)), den, dim_num, dim_den)
    both(lib, oracle, edge_column(dim_num)[::-1].copy(), den, dim_num, dim_den)
    for v in EDGE:                                       # each as the sum's one numerator
        scan(lib, oracle, "gsum", np.array([[v, P - v, v][:dim_num]], np.uint64), den, dim_num, dim_den)


@pytest.mark.parametrize("dim", [3, 1])
def test_chosen_columns(lib, oracle, dim):
    n = C_ + 1
    num, den = columns(51 + dim, n, dim, dim)
    one = [1, 0, 0][:dim]
    # den == num on the same device buffer
    z = scan(lib, oracle, "gprod", den, den, dim, dim, alias=True)
    assert (z == np.array(one, np.uint64)).all()
    # the numerators a rotation of the denominators: the last denominator closes the product, z[n-1] num[n-1] / den[n-1] = 1
    rot = np.roll(den, 1, axis=0).copy()
    z = scan(lib, oracle, "gprod", rot, den, dim, dim)
    last = href.mul3(href.e3(z[n - 1], dim), href.mul3(href.e3(rot[n - 1], dim), href.inv3(href.e3(den[n - 1], dim))))
    assert last == (1, 0, 0) and z[n - 1].tolist() != one
    # a zero numerator is ordinary arithmetic
    nz = num.copy()
    nz[C_ - 3] = 0
    zz, sz = both(lib, oracle, nz, den, dim, dim)
    assert zz[C_ - 3].any() and not zz[C_ - 2:].any()
    nz[0] = 0
    _, sz = both(lib, oracle, nz, den, dim, dim)
    assert not sz.any()


def test_small_calls_after_a_large_one(lib, oracle):
    """the scratch only grows: after a call of T + 1 blocks the totals of the large call lie directly behind the one total of n = 5 and the
    two of n = C + 1"""
    big = T_ * C_ + 1
    assert pil2gl.hint_plan(big)["blocks"] == T_ + 1 and pil2gl.hint_plan(5)["blocks"] == 1 and pil2gl.hint_plan(C_ + 1)["blocks"] == 2
    bn, bd = columns(61, big, 3, 3)
    small = {n: columns(62 + n, n, 3, 3) for n in (5, C_ + 1)}
    for large, first, second in (("gprod", "gsum", "gprod"), ("gsum", "gprod", "gsum")):
        scan(lib, oracle, large, bn if large == "gprod" else bn[:1], bd, 3, 3)
        for op, n in ((first, 5), (second, C_ + 1), (second, 5), (first, C_ + 1)):
            num, den = small[n]
            scan(lib, oracle, op, num if op == "gprod" else num[:1], den, 3, 3)


# ---- h1h2 ----
def distinct(seed, n, dim):
    t = rand_field(np.random.default_rng(seed), (n, dim))
    assert len(set(keys_of(t, dim))) == n
    return t


@pytest.mark.parametrize("dim", [1, 3])
@pytest.mark.parametrize("n", [1, 2, I_, C_ - 1, C_, C_ + 1, 2 * C_ + 1])
def test_h1h2_edges(lib, oracle, n, dim):
    t = distinct(n * 2 + dim, n, dim)
    rng = np.random.default_rng(n)
    for f in (t[rng.permutation(n)], np.repeat(t[n // 3:n // 3 + 1], n, axis=0), np.repeat(t[n - 1:], n, axis=0)):
        lookup(lib, oracle, f.copy(), t, dim)


CANDIDATES = 4096


def candidate(i, dim):
    """the candidate rule of the searches: key = i in word 0"""
    return (i,) if dim == 1 else (i, 5, 9)


def by_home(dim, capacity):
    homes = {}
    for i in range(CANDIDATES):
        homes.setdefault(pil2gl.h1h2_home(np.array(candidate(i, dim), np.uint64), dim, capacity), []).append(candidate(i, dim))
    return homes


@pytest.mark.parametrize("dim", [1, 3])
@pytest.mark.parametrize("chain", ["one home", "wraps"])
def test_h1h2_forced_probe_chains(lib, oracle, chain, dim):
    """three values on one home slot, with a fourth whose home is the next slot; three values on the last two slots, whose chain wraps to
    slot 0, the home of a fourth.  t repeats them: the last index wins"""
    n = 8
    cap = 1 << pil2gl.hint_plan(n)["h1h2CapBits"]
    assert cap == 16
    homes = by_home(dim, cap)
    assert all(len(homes.get(h, ())) >= 3 for h in range(cap)), "the search: three candidates on every home slot"
    if chain == "one home":
        a, b, c = homes[6][:3]
        d = homes[7][0]
    else:
        a, (b, c) = homes[cap - 2][0], homes[cap - 1][:2]
        d = homes[0][0]
    t = np.array([a, b, c, d, a, b, c, a], np.uint64)
    f = np.array([a] * 4 + [b] * 2 + [c] + [d], np.uint64)
    lookup(lib, oracle, f, t, dim)
    lookup(lib, oracle, f[::-1].copy(), t[::-1].copy(), dim)


def test_h1h2_keys_that_differ_in_one_word(lib, oracle):
    """four dim-3 keys on ONE home slot of a 16-slot table: the base, one that differs from it in the high half of word 0 only, one in the
    low half of word 1 only, one in word 2 only.  A comparison of fewer than all three words merges two of them"""
    n = 8
    cap = 1 << pil2gl.hint_plan(n)["h1h2CapBits"]
    base = (0x0123456789ABCDEF, 0x0FEDCBA987654321, 0x00F0E1D2C3B4A596)
    home = lambda k: pil2gl.h1h2_home(np.array(k, np.uint64), 3, cap)      # noqa: E731
    variants = [lambda i: (base[0] ^ (i << 32), base[1], base[2]), lambda i: (base[0], base[1] ^ i, base[2]), lambda i: (base[0], base[1], base[2] ^ (i << 32 | i))]
    found = [next((v(i) for i in range(1, CANDIDATES) if home(v(i)) == home(base)), None) for v in variants]
    assert None not in found, "the search: a variant of every word on the base's home slot"
    k0, (k1, k2, k3) = base, found
    assert (k1[0] ^ k0[0]) >> 32 and not (k1[0] ^ k0[0]) & 0xFFFFFFFF and k1[1:] == k0[1:]
    assert not (k2[1] ^ k0[1]) >> 32 and (k2[1] ^ k0[1]) & 0xFFFFFFFF and (k2[0], k2[2]) == (k0[0], k0[2])
    assert k3[:2] == k0[:2] and k3[2] != k0[2] and max(max(k) for k in found) < P
    t = np.array([k0, k1, k2, k3, k3, k2, k1, k0], np.uint64)
    f = np.array([k0] + [k1] * 2 + [k2] * 5, np.uint64)
    lookup(lib, oracle, f, t, 3)
    lookup(lib, oracle, np.array([k3] * 4 + [k2] * 3 + [k0], np.uint64), t[::-1].copy(), 3)


@pytest.mark.parametrize("dim", [1, 3])
def test_h1h2_missing_values(lib, oracle, dim):
    """t holds even words 0 only, the missing value an odd one: rows 300, 64 and 129 of f -> the refusal names row 64; a good call on the
    same buffers follows.  Then a missing value whose home chain other keys occupy"""
    n = C_ + 1
    rng = np.random.default_rng(90 + dim)
    t = distinct(91 + dim, n, dim)
    t[:, 0] &= np.uint64(~1 & (2 ** 64 - 1))
    assert len(set(keys_of(t, dim))) == n
    good = t[rng.integers(0, n, n)]
    bad = good.copy()
    gone = t[17].copy()
    gone[0] |= np.uint64(1)
    assert int(gone[0]) < P
    for r in (300, 64, 129):
        bad[r] = gone
    bufs = lookup(lib, oracle, bad, t, dim, missing=64)
    lookup(lib, oracle, good, t, dim, bufs=bufs)
    bad[64] = good[64]
    lookup(lib, oracle, bad, t, dim, bufs=bufs, missing=129)
    lookup(lib, oracle, good[::-1].copy(), t, dim, bufs=bufs)
    # n = 8: three keys of t on the missing key's home slot
    cap = 1 << pil2gl.hint_plan(8)["h1h2CapBits"]
    homes = by_home(dim, cap)
    assert len(homes.get(3, ())) >= 4 and all(len(homes.get(h, ())) >= 1 for h in (4, 5, 9, 10, 11))
    a, b, c, m = homes[3][:4]
    t8 = np.array([a, b, c] + [homes[h][0] for h in (4, 5, 9, 10, 11)], np.uint64)
    f8 = np.array([a] * 8, np.uint64)
    f8[5] = m
    bufs = lookup(lib, oracle, f8, t8, dim, missing=5)
    f8[5] = c
    lookup(lib, oracle, f8, t8, dim, bufs=bufs)


@pytest.mark.parametrize("dim", [1, 3])
def test_h1h2_duplicates_over_a_block_boundary_of_the_start_scan(lib, oracle, dim):
    """n = 2 C + 1, every value of t twice but one: adjacent copies (those of X end at row C - 1), copies on opposite sides of row C (Y at
    rows 0 and C, W at rows 1 and 2 C); a quarter of f on X, a quarter on Y: heavy counts on both sides of the boundary"""
    n = 2 * C_ + 1
    v = distinct(97 + dim, C_ + 1, dim)
    y, w, x, single, pairs = v[0], v[1], v[2], v[3], v[4:]
    assert len(pairs) == C_ - 3
    lo, hi = pairs[:(C_ - 4) // 2], pairs[(C_ - 4) // 2:]
    t = np.concatenate([[y, w], np.repeat(lo, 2, axis=0), [x, x], [y, single], np.repeat(hi, 2, axis=0), [w]])
    assert t.shape == (n, dim) and len(hi) == (C_ - 2) // 2
    kt = keys_of(t, dim)
    last = {k: i for i, k in enumerate(kt)}
    assert last[kt[C_ - 1]] == C_ - 1 and kt[C_ - 2] == kt[C_ - 1] and last[kt[0]] == C_ and kt[1] == kt[2 * C_]
    rng = np.random.default_rng(5)
    f = t[rng.integers(0, n, n)]
    f[:n // 4] = x
    f[n // 4:2 * (n // 4)] = y
    f = f[rng.permutation(n)]
    lookup(lib, oracle, f, t, dim)
