"""The BN254 Fr plookup hint on the device (pil2gl.bn128.h1h2 over csrc/bn_h1h2.hip) against the Python checker (tests/bn128_h1h2_ref.py: the
reference's calculateH1H2 transcribed, a dict and a stable sort) and against the reference-recorded cases of tests/golden/hints.json.
Every comparison is exact equality of words.  Outputs are pre-filled with a sentinel, which the words between strided elements must
keep; inputs must be unchanged.  Threshold shapes are asked of the planner hook (h1h2_plan), never typed in; apart from one case of 2^16
rows everything is at most 2^14 rows."""
import numpy as np
import pytest

import bn128_chosen
import bn128_h1h2_ref as ref
import bn128_hints_ref as href
from bn128_hints_ref import R
from conftest import golden, H

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SENTINEL = np.uint64(0xA5A5A5A5A5A5A5A5)


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


def strided(words, stride):
    """(n, 4) words as a column of stride `stride`: flat words up to the last element, the sentinel between the elements"""
    n = words.shape[0]
    m = np.full((n, stride, 4), SENTINEL, np.uint64)
    m[:, 0] = words
    return m.reshape(-1)[:((n - 1) * stride + 1) * 4].copy()


def column_of(flat, n, stride):
    idx = (np.arange(n)[:, None] * 4 * stride + np.arange(4)[None, :]).reshape(-1)
    return flat[idx].reshape(n, 4), idx


def differs(got, want, what):
    bad = np.argwhere((got != want).any(axis=1))
    assert bad.size == 0, "%s: %d rows, differs first at row %d" % (what, got.shape[0], bad[0][0])


def distinct(n, seed):
    """n distinct canonical elements, as the integers their words spell"""
    vals = list(dict.fromkeys(href.rand_elems(n + 8, seed)))[:n]
    assert len(vals) == n
    return vals


def drawn(t, seed, n=None):
    rng = np.random.default_rng(seed)
    return [t[i] for i in rng.integers(0, len(t), n or len(t))]


def run(bn, f, t, strides=(1, 1, 1, 1), on_device=True, want=None, what=""):
    """f, t: integers below 2^256, the words as they are.  Calls h1h2 with sentinel-filled outputs of the given strides, compares both
    outputs in whole with the checker's (or `want`), the words between a strided output's elements with the sentinel, and the inputs
    with what they were.  -> (h1 words, h2 words)"""
    n, (sf, st, s1, s2) = len(t), strides
    wf, wt = strided(href.words(f), sf), strided(href.words(t), st)
    to = dev if on_device else (lambda a: a.copy())
    back = host if on_device else (lambda a: a)
    df, dt = to(wf), to(wt)
    o1, o2 = (to(np.full(((n - 1) * s + 1) * 4, SENTINEL, np.uint64)) for s in (s1, s2))
    r1, r2 = bn.h1h2(df, dt, n=n, f_stride=sf, t_stride=st, h1=o1, h1_stride=s1, h2=o2, h2_stride=s2)
    assert r1 is o1 and r2 is o2
    exp = want or ref.h1h2(f, t)
    cols = []
    for name, o, s, e in (("h1", o1, s1, exp[0]), ("h2", o2, s2, exp[1])):
        g = back(o)
        col, idx = column_of(g, n, s)
        differs(col, href.words(e), "%s %s n = %d strides %s" % (what, name, n, strides))
        rest = np.ones(g.shape[0], bool)
        rest[idx] = False
        assert (g[rest] == SENTINEL).all(), "%s: words between the elements were written" % name
        cols.append(col)
    assert np.array_equal(back(df), wf) and np.array_equal(back(dt), wt), "an input was written"
    return cols


# ---- 1. sizes ------------------------------------------------------------------------------------------------------------------------------
def test_sizes(bn):
    """tables of 2 to 16 slots (n = 1..5: probe sequences wrap round the end), one and several workgroups, the scan chunk and the expand
    step's rows per workgroup and one more of each"""
    p = bn.h1h2_plan(1000)
    chunk, rows = p["scanChunk"], p["expandRows"]
    assert [bn.h1h2_plan(n)["capacity"] for n in (1, 2, 3, 4, 5)] == [2, 4, 8, 8, 16]
    assert bn.h1h2_plan(chunk)["scanBlocks"] == 1 and bn.h1h2_plan(chunk + 1)["scanBlocks"] == 2
    assert bn.h1h2_plan(rows)["expandBlocks"] == 1 and bn.h1h2_plan(rows + 1)["expandBlocks"] == 2
    for n in sorted({1, 2, 3, 4, 5, 64, 65, 257, 1000, rows, rows + 1, chunk, chunk + 1}):
        for seed in range(3 if n <= 5 else 1):                      # several tiny tables: different slots collide
            t = distinct(n, 100 * n + seed)
            run(bn, drawn(t, n + seed), t, what="sizes")


def test_two_to_the_sixteen(bn):
    n = 1 << 16
    t = distinct(n, 16)
    run(bn, drawn(t, 17), t)


# ---- 2. reference-pinned -------------------------------------------------------------------------------------------------------------------
def test_reference_recorded_cases_as_fr_elements(bn):
    """the dim-1 cases of tests/golden/hints.json (what the reference's calculateH1H2 returned) as Fr elements in Montgomery form"""
    cases = [c for c in golden("hints.json")["h1h2"] if c["dim"] == 1]
    assert len(cases) >= 3
    for c in cases:
        f, t, h1, h2 = (href.ints(href.mont_words(H(c[k]))) for k in ("f", "t", "h1", "h2"))
        assert max(H(c["t"])) < R
        run(bn, f, t, want=(h1, h2), what="golden n = %d" % c["n"])


# ---- 3. duplicates in t --------------------------------------------------------------------------------------------------------------------
def test_worked_case_counts_go_to_the_last_occurrence(bn):
    a, b = distinct(2, 3)
    t, f = [a, b, a], [a, a, b]
    want = ([a, b, a], [b, a, a])
    assert ref.h1h2(f, t) == want and ref.by_counts(f, t, first_occurrence=True) != want
    run(bn, f, t, want=want)


def test_duplicates_in_t(bn):
    chunk = bn.h1h2_plan(1000)["scanChunk"]
    half = distinct(500, 31)
    twice = half + half[::-1]                                     # every value twice
    run(bn, drawn(half, 32, 1000), twice, what="every value twice")
    assert ref.h1h2(drawn(half, 32, 1000), twice) != ref.by_counts(drawn(half, 32, 1000), twice, first_occurrence=True)
    pairs = [v for v in distinct(150, 33) for _ in range(2)]      # ... and next to each other
    run(bn, drawn(pairs, 34), pairs, what="adjacent pairs")
    one = distinct(1, 35) * 300                                   # all equal: n maxima on one slot, n additions on one counter
    run(bn, one, one, what="all equal")
    n = chunk + 100                                               # first and last occurrence on the two sides of a scan-chunk boundary
    t = distinct(n, 36)
    t[chunk + 5] = t[chunk - 3]
    f = drawn(t, 37)
    f[10:40] = [t[chunk - 3]] * 30
    want = ref.h1h2(f, t)
    assert want != ref.by_counts(f, t, first_occurrence=True)
    run(bn, f, t, want=want, what="straddling a chunk")


# ---- 4. skew -------------------------------------------------------------------------------------------------------------------------------
def test_skew(bn):
    n = 1000
    t = distinct(n, 41)
    run(bn, [t[0]] * n, t, what="all f = t[0]")
    run(bn, [t[n - 1]] * n, t, what="all f = t[n - 1]")
    run(bn, drawn(t[::2], 42, n), t, what="half of t never referenced")


# ---- 5. chosen words -----------------------------------------------------------------------------------------------------------------------
def test_chosen_words(bn):
    """pairs of keys that differ in exactly one 32-bit limb, for each limb, and in one bit next to bit 255 (elements are compared as their
    bytes: the top bits are not validated away); 0 and r - 1; the limb patterns of tests/bn128_chosen.py.  Both keys of a pair are in t
    and f refers to both, so a compare that skips a limb merges two groups"""
    base = distinct(1, 51)[0] & ~(0xF << 252)
    keys = [base] + [base ^ (1 << (32 * limb + 7)) for limb in range(8)]
    keys += [base ^ (1 << bit) for bit in (252, 253, 254, 255)]
    keys += [0, R - 1, 1, 1 << 32, 1 << 224, (1 << 224) | 1]
    keys += [w for _, w in bn128_chosen.PATTERNS] + href.limb_pattern_elems(40, 5)
    keys = list(dict.fromkeys(keys))
    assert len(keys) > 40
    t = keys + distinct(len(keys), 52)
    f = [k for k in keys for _ in range(2)]                        # every chosen key twice
    h1, h2 = run(bn, f, t, what="chosen")
    merged = href.ints(np.stack([h1, h2], axis=1).reshape(-1, 4))
    assert all(merged.count(k) == 3 for k in keys)
    t2 = keys[::-1] + keys                                        # and duplicated in t: the counts at the second copy
    run(bn, f, t2, what="chosen, duplicated")


ONE_BIT_APART = tuple(32 * limb + 7 for limb in range(8)) + (252, 253, 254)


@pytest.mark.parametrize("bit", ONE_BIT_APART)
def test_keys_one_bit_apart_that_meet_in_the_table(bn, bit):
    """A hash that mixes every limb sends two keys that differ in one bit to unrelated slots, and the compare sees the pair only where
    the second key's probes pass the first one's slot.  So the pair is alone in a table of 4 slots (n = 2), where that happens one time
    in four, 40 times over with other bases: all 40 missing the compare has probability (3/4)^40, about 1e-5, and with fixed seeds the
    run is the same every time.  A compare that skips the limb then makes one group of two: x, y, y, y instead of x, x, y, y.
    Bit 255 has no case here: flipped alone it always changes the low bit of this hash's slot, so the pair cannot meet in 4 slots and 40
    runs would show nothing.  The top limb is met through bits 231 and 252 to 254; a pair one apart in bit 255 is among the keys of
    test_chosen_words, where the outputs must keep the two values apart."""
    for seed in range(40):
        x = distinct(1, 1000 * bit + seed)[0] & ~(0xF << 252)
        y = x ^ (1 << bit)
        run(bn, [y, x], [x, y], want=([x, y], [x, y]), what="bit %d base %d" % (bit, seed))


# ---- 6. strides ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("on_device", (True, False))
def test_strided_columns_and_two_columns_of_one_section(bn, on_device):
    n, w = 1300, 5
    t = distinct(n, 61)
    f = drawn(t, 62)
    want = ref.h1h2(f, t)
    run(bn, f, t, strides=(3, 1, 5, 2), on_device=on_device, want=want)
    # h1 and h2 as columns 1 and 3 of one section 5 wide
    sec = np.full((n, w, 4), SENTINEL, np.uint64)
    to, back = (dev, host) if on_device else ((lambda a: a.copy()), (lambda a: a))
    wf, wt = strided(href.words(f), 3), href.words(t).reshape(-1)
    df, dt, ds = to(wf), to(wt), to(sec.reshape(-1))
    bn.h1h2(df, dt, n=n, f_stride=3, h1=ds[4:], h1_stride=w, h2=ds[12:], h2_stride=w)
    got = back(ds).reshape(n, w, 4)
    differs(got[:, 1], href.words(want[0]), "column 1")
    differs(got[:, 3], href.words(want[1]), "column 3")
    assert (got[:, (0, 2, 4)] == SENTINEL).all()
    assert np.array_equal(back(df), wf) and np.array_equal(back(dt), wt)
    from pil2gl import Pil2glError
    with pytest.raises(Pil2glError, match="overlaps"):
        bn.h1h2(df, dt, n=n, f_stride=3, h1=ds[4:], h1_stride=w, h2=ds[4:], h2_stride=w)


def test_h2_below_h1_in_one_section_on_the_host(bn):
    n, w = 300, 3
    t = distinct(n, 63)
    f = drawn(t, 64)
    want = ref.h1h2(f, t)
    wf, wt = href.words(f).reshape(-1), href.words(t).reshape(-1)
    s = np.full(n * w * 4, SENTINEL, np.uint64)
    bn.h1h2(wf.copy(), wt.copy(), n=n, h1=s[8:], h1_stride=w, h2=s, h2_stride=w)      # h2 column 0, h1 column 2, host pointers
    got = s.reshape(n, w, 4)
    differs(got[:, 2], href.words(want[0]), "h1, column 2")
    differs(got[:, 0], href.words(want[1]), "h2, column 0")
    assert (got[:, 1] == SENTINEL).all()


# ---- 7. missing ----------------------------------------------------------------------------------------------------------------------------
def test_missing_value(bn):
    from pil2gl import Pil2glError
    n = 700
    t = distinct(n + 2, 71)
    absent, other, t = t[n], t[n + 1], t[:n]
    good = drawn(t, 72)
    for places, lowest in (((0,), 0), ((n - 1,), n - 1), ((400, 123), 123)):
        f = list(good)
        for k, j in enumerate(places):
            f[j] = (absent, other)[k]
        for on_device in (True, False):
            to, back = (dev, host) if on_device else ((lambda a: a.copy()), (lambda a: a))
            o1, o2 = (to(np.full(n * 4, SENTINEL, np.uint64)) for _ in range(2))
            with pytest.raises(Pil2glError, match=r"Number not included: w:%d$" % lowest) as e:
                bn.h1h2(to(href.words(f).reshape(-1)), to(href.words(t).reshape(-1)), n=n, h1=o1, h2=o2)
            assert e.value.missing_row == lowest
            assert (back(o1) == SENTINEL).all() and (back(o2) == SENTINEL).all(), "an output was written before the check"
        run(bn, good, t, what="right after a refusal")              # the missing cell is reset


# ---- 8. reuse ------------------------------------------------------------------------------------------------------------------------------
def test_reuse_of_the_working_buffer(bn):
    n = 1 << 14
    t = distinct(n, 81)
    f = drawn(t, 82)
    first = run(bn, f, t)
    small = distinct(5, 83)
    run(bn, drawn(small, 84), small)                              # a smaller call after a larger one
    t2 = distinct(n, 85)
    run(bn, drawn(t2, 86), t2)                                    # other data: nothing of the first call may be read
    again = run(bn, f, t)
    assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1])     # equal bytes


def test_no_rows(bn):
    d = dev(href.words([7]).reshape(-1))
    bn.h1h2(d, d, n=0, h1=d, h2=d)
    assert href.ints(host(d)) == [7]
