"""The recursion witness expansion on the device (pil2gl.wtns over csrc/wtns_exec.hip) against the checker tests/wtns_exec_ref.py, a plain
transcription of the reference's two loops (compressor_exec.js:17-29, main_final_exec.js:55-67) over Python integers.  Every comparison is
exact equality of words.  The reference tree ships no .exec or .wtns and its setups need pilcom / circom_runtime, which are not
available, so no reference-written fixture exists: the tables here are made to reach every path of the kernels instead -- widths and
row counts around the workgroup and wave sizes, more than 2^16 cells and additions, operands that are additions, chosen field values.
Nothing here provokes a fault: the guard tests use tables that stay inside their allocations."""
import numpy as np
import pytest

import wtns_exec_ref as ref
from wtns_exec_ref import P, R

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

RINV = pow(1 << 256, -1, R)


@pytest.fixture(scope="module")
def wt():
    import pil2gl
    from pil2gl import wtns
    pil2gl.init(0)
    return wtns


def dev(words):
    return torch.from_numpy(np.ascontiguousarray(words, np.uint64).view(np.int64)).cuda()


def host(t):
    return t.cpu().numpy().view(np.uint64)


def s_map_for(rng, n_w, n_rows, n_cols):
    """zeros, index 0 (which means zero), 1 and nW - 1, a row of all zeros and a row naming one signal in every column"""
    m = [rng.choice((0, 0, 1, n_w - 1, rng.randrange(n_w), rng.randrange(n_w), rng.randrange(n_w))) for _ in range(n_rows * n_cols)]
    for k, v in enumerate((0, 1, n_w - 1)):
        if k < len(m):
            m[-1 - k] = v
    if n_rows >= 4:
        m[n_cols:2 * n_cols] = [0] * n_cols
        m[2 * n_cols:3 * n_cols] = [n_w - 2] * n_cols
    return m


# ---- Goldilocks ----
GL_EDGE = [P - 1, P, P + 1, (1 << 64) - 1, 0, 1]


def gl_case(seed, n_extra_adds=40):
    """witness with the edge words, then additions: (p-1)(p-1) + (p-1)(p-1); both operands one signal; a coefficient 0; coefficient words
    p, p + 1, 2^64 - 1; an addition of two additions; then a random DAG"""
    rng = ref.rng(seed)
    w = GL_EDGE + [rng.randrange(1 << 64) for _ in range(26)]
    n = len(w)
    adds = [(0, 0, P - 1, P - 1), (7, 7, 3, 5), (8, 9, 0, 11), (10, 3, P, P + 1), (2, 11, (1 << 64) - 1, 2), (n + 0, n + 1, 7, 9), (n + 5, n + 5, P - 1, 1)]
    adds += [(a + 0, b + 0, ca, cb) for a, b, ca, cb in _shift(ref.random_dag(rng, n, n_extra_adds, 1 << 64), n, len(adds))]
    return w, adds


def _shift(adds, n, by):
    """operands that name additions move up by the additions put in front"""
    return [(a + by if a >= n else a, b + by if b >= n else b, ca, cb) for a, b, ca, cb in adds]


def gl_exec(w, adds, s_map, n_rows, n_cols):
    return {"field": "gl", "nWitness": len(w), "nAdds": len(adds), "nSMap": n_rows, "nCols": n_cols,
            "adds": np.array([x for r in adds for x in r], np.uint64), "sMap": np.array(s_map, np.uint64)}


def gl_resident(wt, ex, w, dst_cols=None, **kw):
    prep = wt.prepare(ex)
    w_dev = dev(np.concatenate([np.array(w, np.uint64), np.full(ex["nAdds"], 0xA5A5A5A5A5A5A5A5, np.uint64)]))
    return wt.exec_dev(prep, w_dev, dst_cols=dst_cols, **kw), w_dev


@pytest.mark.parametrize("n_cols,n_rows", [(c, r) for c in (1, 5, 12, 18) for r in (1, 63, 64, 65, 257, 1024)] + [(1, 70001)])
def test_gl_trace_host_and_resident_forms(wt, n_cols, n_rows):
    w, adds = gl_case(n_cols * 1000 + n_rows)
    rng = ref.rng(n_rows)
    n_w = len(w) + len(adds)
    s_map = s_map_for(rng, n_w, n_rows, n_cols)
    ex = gl_exec(w, adds, s_map, n_rows, n_cols)
    full = ref.additions(w, adds, P)
    want = np.array(ref.gather(full, s_map, n_rows, n_cols, n_cols, P), np.uint64)
    got = wt.exec_gl(np.array(w, np.uint64), ex)
    assert (got == want).all(), "host form"
    out, w_dev = gl_resident(wt, ex, w)
    assert (host(out) == want).all(), "resident form"
    assert [int(x) for x in host(w_dev)[len(w):]] == full[len(w):], "derived signals, canonical"
    wide, _ = gl_resident(wt, ex, w, dst_cols=n_cols + 3)
    want_wide = np.array(ref.gather(full, s_map, n_rows, n_cols, n_cols + 3, P), np.uint64)
    assert (host(wide) == want_wide).all(), "widened"


def test_gl_chain_of_depth_300_and_a_level_of_70000(wt):
    w = [3, 5, P - 2]
    chain = [(0, 1, 2, 3)] + [(3 + i, i % 3, P - 1 - i, i + 1) for i in range(299)]
    ex = gl_exec(w, chain, [len(w) + 299, 1, 0, 3], 2, 2)
    assert wt.plan_info(ex["adds"], len(w), 4)["levels"] == 300
    assert wt.exec_gl(np.array(w, np.uint64), ex).tolist() == ref.trace(w, chain, ex["sMap"].tolist(), 2, 2, P)
    rng = ref.rng(7)
    w = [rng.randrange(1 << 64) for _ in range(500)]
    flat = [(rng.randrange(500), rng.randrange(500), rng.randrange(1 << 64), rng.randrange(1 << 64)) for _ in range(70000)]
    flat.append((500 + 69999, 500 + 65536, 1, 1))                       # a second level over the first one's far end
    n_w = 500 + len(flat)
    s_map = [500 + k for k in range(0, 70000, 7)] + [n_w - 1]
    n_rows = len(s_map)
    ex = gl_exec(w, flat, s_map, n_rows, 1)
    info = wt.plan_info(ex["adds"], 500, 4)
    assert info["widths"] == [70000, 1] and info["launches"] == 2
    out, _ = gl_resident(wt, ex, w)
    assert host(out).reshape(-1).tolist() == [r[0] for r in ref.trace(w, flat, s_map, n_rows, 1, P)]


def test_gl_guards_report_the_first_bad_cell_and_write_zero(wt):
    w, adds = gl_case(5)
    n_w = len(w) + len(adds)
    n_rows, n_cols = 65, 5
    s_map = s_map_for(ref.rng(3), n_w, n_rows, n_cols)
    ex = gl_exec(w, adds, s_map, n_rows, n_cols)
    prep = wt.prepare(ex)
    w_dev = dev(np.array(w + [0] * len(adds), np.uint64))
    wt.adds_dev(prep, w_dev)
    bad = list(s_map)
    bad[201], bad[77] = n_w, (1 << 32) - 1
    table = dev(np.array(bad + [0] * (len(bad) % 2), np.uint32).view(np.uint64))
    out, first = wt.gather_dev(prep, w_dev, check=True, s_map=table)
    assert first == 77
    clean = list(s_map)
    clean[201] = clean[77] = 0
    want = np.array(ref.gather(ref.additions(w, adds, P), clean, n_rows, n_cols, n_cols, P), np.uint64)
    assert (host(out) == want).all()
    out, first = wt.gather_dev(prep, w_dev, check=True)
    assert first is None


def test_an_operand_out_of_range_is_refused_by_the_plan(wt):
    import pil2gl
    w, adds = gl_case(6)
    for k, what in ((3, len(w) + 3), (9, len(w) + len(adds)), (0, 1 << 40)):
        broken = list(adds)
        broken[k] = (what, 1, 1, 1)
        with pytest.raises(pil2gl.Pil2glError, match="error -1: addition %d" % k):
            wt.prepare(gl_exec(w, broken, [0], 1, 1))


def test_gl_expanded_trace_feeds_interpolate_unchanged(wt):
    import pil2gl
    w, adds = gl_case(9)
    n_bits, n_cols = 6, 5
    s_map = s_map_for(ref.rng(9), len(w) + len(adds), 1 << n_bits, n_cols)
    ex = gl_exec(w, adds, s_map, 1 << n_bits, n_cols)
    trace, _ = gl_resident(wt, ex, w)
    built = dev(np.array(ref.trace(w, adds, s_map, 1 << n_bits, n_cols, P), np.uint64))
    a = torch.empty((1 << (n_bits + 1)) * n_cols, dtype=torch.int64, device="cuda")
    b = torch.empty_like(a)
    pil2gl.interpolate(trace.reshape(-1), n_cols, n_bits, a, n_bits + 1)
    pil2gl.interpolate(built.reshape(-1), n_cols, n_bits, b, n_bits + 1)
    assert torch.equal(a, b)


# ---- BN254 Fr ----
FR_EDGE = [R - 1, R, (1 << 256) - 1, 0, 1]


def fr_case(seed, n_extra_adds=30):
    """the same structure over Fr; a coefficient is given as the 256-bit pattern of its Montgomery word, whatever it is"""
    rng = ref.rng(seed)
    w = FR_EDGE + [rng.randrange(1 << 256) for _ in range(20)] + [(k + 1) | ((k + 1001) << 128) for k in range(6)]
    n = len(w)
    adds = [(0, 0, R - 1, R - 1), (7, 7, 3, 5), (8, 9, 0, 11), (10, 2, R, (1 << 256) - 1), (2, 11, 1, 2), (n + 0, n + 1, 7, 9), (n + 5, n + 5, R - 1, 1)]
    adds += _shift(ref.random_dag(rng, n, n_extra_adds, 1 << 256), n, len(adds))
    return w, adds


def fr_exec(w, adds, s_map, n_rows, n_cols):
    return {"field": "bn128", "nWitness": len(w), "nAdds": len(adds), "nSMap": n_rows, "nCols": n_cols,
            "addsIdx": np.array([x for a, b, _, _ in adds for x in (a, b)], np.uint64),
            "addsCoef": ref.fr_words([c for _, _, ca, cb in adds for c in (ca, cb)]), "sMap": np.array(s_map, np.uint64)}


def fr_values(adds):
    """the additions with the VALUES their coefficient words stand for"""
    return [(a, b, ca * RINV % R, cb * RINV % R) for a, b, ca, cb in adds]


@pytest.mark.parametrize("n_cols,n_rows", [(1, 1), (1, 63), (1, 64), (1, 65), (6, 63), (6, 64), (6, 65), (9, 257), (7, 1024), (1, 33000)])
def test_fr_trace_both_forms_and_both_representations(wt, n_cols, n_rows):
    w, adds = fr_case(n_cols * 1000 + n_rows)
    n_w = len(w) + len(adds)
    s_map = s_map_for(ref.rng(n_rows), n_w, n_rows, n_cols)
    ex = fr_exec(w, adds, s_map, n_rows, n_cols)
    full = ref.additions(w, fr_values(adds), R)
    rows = ref.gather(full, s_map, n_rows, n_cols, n_cols, R)
    normal = ref.fr_words([v for r in rows for v in r]).reshape(n_rows, n_cols, 4)
    mont = ref.fr_words([ref.to_mont(v) for r in rows for v in r]).reshape(n_rows, n_cols, 4)
    assert (wt.exec_bn128(ref.fr_words(w), ex) == mont).all(), "host form, Montgomery"
    assert (wt.exec_bn128(ref.fr_words(w), ex, montgomery=False) == normal).all(), "host form, normal"
    prep = wt.prepare(ex)
    w_dev = dev(np.concatenate([ref.fr_words(w), np.full((len(adds), 4), 0xA5A5A5A5A5A5A5A5, np.uint64)]))
    out = wt.exec_dev(prep, w_dev)
    assert (host(out) == mont).all(), "resident form, Montgomery"
    assert ref.fr_ints(host(w_dev)[len(w):]) == full[len(w):], "derived signals, normal form, canonical"
    wide = wt.gather_dev(prep, w_dev, dst_cols=n_cols + 3, montgomery=False)
    rows_w = ref.gather(full, s_map, n_rows, n_cols, n_cols + 3, R)
    assert (host(wide) == ref.fr_words([v for r in rows_w for v in r]).reshape(n_rows, n_cols + 3, 4)).all(), "widened, normal"


def test_fr_halves_of_neighbouring_elements_stay_in_place(wt):
    """elements whose low and high 16 bytes differ, read back in normal form at every other cell: a swap of halves between the two lanes of a
    cell, or between neighbouring cells, shows as a wrong word"""
    w = [0] + [(k + 1) | ((k + 7) << 64) | ((k + 1001) << 128) | ((k + 5) << 192) for k in range(300)]
    n_rows, n_cols = 75, 4
    s_map = [1 + (k * 7) % 300 if k % 2 == 0 else 0 for k in range(n_rows * n_cols)]
    ex = fr_exec(w, [], s_map, n_rows, n_cols)
    got = wt.exec_bn128(ref.fr_words(w), ex, montgomery=False)
    want = ref.fr_words([w[s] for s in s_map]).reshape(n_rows, n_cols, 4)
    assert (got == want).all()
    out = wt.exec_dev(wt.prepare(ex), dev(ref.fr_words(w)), montgomery=False)
    assert (host(out) == want).all()


def test_fr_chain_and_guards(wt):
    w = [3, 5, R - 2]
    chain = [(0, 1, 2, 3)] + [(3 + i, i % 3, R - 1 - i, i + 1) for i in range(299)]
    s_map = [len(w) + 299, 1, 0, 3, 2, 150]
    ex = fr_exec(w, chain, s_map, 3, 2)
    want = ref.fr_words([v for r in ref.trace(w, fr_values(chain), s_map, 3, 2, R) for v in r]).reshape(3, 2, 4)
    assert (wt.exec_bn128(ref.fr_words(w), ex, montgomery=False) == want).all()
    prep = wt.prepare(ex)
    w_dev = dev(np.concatenate([ref.fr_words(w), np.zeros((300, 4), np.uint64)]))
    wt.adds_dev(prep, w_dev)
    bad = list(s_map)
    bad[4], bad[1] = len(w) + 300, (1 << 32) - 1
    out, first = wt.gather_dev(prep, w_dev, montgomery=False, check=True, s_map=dev(np.array(bad, np.uint32).view(np.uint64)))
    assert first == 1
    want[0, 1] = 0
    want[2, 0] = 0
    assert (host(out) == want).all()


def test_fr_level_of_70000_additions_and_one_over_its_far_end(wt):
    """one level wider than 2^16 records, so that every workgroup of the launch and the grid-stride step run, with the coefficients read at
    4 k halves for every k; then a second-level addition whose operands are the last record and one past 2^16.  Resident form."""
    rng = ref.rng(17)
    w = [rng.randrange(1 << 256) for _ in range(500)]
    flat = [(rng.randrange(500), rng.randrange(500), rng.randrange(1 << 256), rng.randrange(1 << 256)) for _ in range(70000)]
    flat.append((500 + 69999, 500 + 65536, 1 << 255, 3))
    n_w = 500 + len(flat)
    s_map = [500 + k for k in range(0, 70000, 7)] + [n_w - 1]
    n_rows = len(s_map)
    ex = fr_exec(w, flat, s_map, n_rows, 1)
    info = wt.plan_info(ex["addsIdx"], 500)
    assert info["widths"] == [70000, 1] and info["launches"] == 2 and info["widestBlocks"] > 1
    prep = wt.prepare(ex)
    w_dev = dev(np.concatenate([ref.fr_words(w), np.full((len(flat), 4), 0xA5A5A5A5A5A5A5A5, np.uint64)]))
    out = wt.exec_dev(prep, w_dev, montgomery=False)
    full = ref.additions(w, fr_values(flat), R)
    assert ref.fr_ints(host(w_dev)[500:]) == full[500:], "every derived signal, normal form, canonical"
    assert ref.fr_ints(host(out).reshape(-1, 4)) == [full[s] % R for s in s_map]


@pytest.mark.parametrize("field", ["gl", "bn128"])
def test_checked_gathers_reset_their_cell_and_share_none_with_conn_pols(wt, field):
    """The bad cell of a checked gather is a scratch slot kept across calls, so every checked call must reset it on its own stream: the
    reduction is a minimum, and a stale 5 would come back from the call whose only bad cell is 70.  One prepare() of 2 rows x 65 columns:
    130 cells are more than a wave, and for Fr 260 lanes are more than a workgroup.  Between the gathers a checked conn_pols_dev over the
    same resident tables reports its own cell: its cell lies in its working buffer, not in the slot.  conn_pols takes at most 64 columns,
    so it reads prepare()'s tables as 65 rows x 2 columns -- the flat cells, and with them the reported index, are the same."""
    import conn_pols_ref as cref
    n_rows, n_cols = 2, 65
    q = P if field == "gl" else R
    w, adds = gl_case(31, 6) if field == "gl" else fr_case(31, 6)
    n_w = len(w) + len(adds)
    s_map = s_map_for(ref.rng(31), n_w, n_rows, n_cols)
    if field == "gl":
        prep = wt.prepare(gl_exec(w, adds, s_map, n_rows, n_cols))
        w_dev = dev(np.array(w + [0] * len(adds), np.uint64))
        full = ref.additions(w, adds, P)
        words = lambda rows: np.array(rows, np.uint64)                                             # noqa: E731
    else:
        prep = wt.prepare(fr_exec(w, adds, s_map, n_rows, n_cols))
        w_dev = dev(np.concatenate([ref.fr_words(w), np.zeros((len(adds), 4), np.uint64)]))
        full = ref.additions(w, fr_values(adds), R)
        words = lambda rows: ref.fr_words([v for r in rows for v in r]).reshape(n_rows, n_cols, 4)  # noqa: E731
    wt.adds_dev(prep, w_dev)

    def gather(bad_cells, first):
        table = list(s_map)
        for c, v in bad_cells:
            table[c] = v
        out, got = wt.gather_dev(prep, w_dev, montgomery=False, check=True, s_map=dev(np.array(table, np.uint32).view(np.uint64)))
        assert got == first
        zeroed = [0 if s >= n_w else s for s in table]
        assert (host(out) == words(ref.gather(full, zeroed, n_rows, n_cols, n_cols, q))).all()

    gather([(5, n_w), (99, (1 << 32) - 1)], 5)
    gather([], None)
    table = list(s_map)
    table[9] = n_w + 1
    as_rows = dict(prep, nRows=n_cols, nCols=n_rows)                                               # 65 x 2 over the same device tables
    root, ks = cref.root(q, 7), cref.get_ks(q, 1)
    out, got = wt.conn_pols_dev(as_rows, 128, *cref.consts(root, ks, q), check=True, s_map=dev(np.array(table, np.uint32).view(np.uint64)))
    assert got == 9
    table[9] = 0
    assert np.array_equal(host(out), cref.words(cref.conn_pols(table, n_cols, n_rows, 128, root, ks, q), q))
    gather([(70, (1 << 32) - 1)], 70)
    torch.cuda.synchronize()
    with torch.cuda.stream(torch.cuda.Stream()):
        gather([(70, n_w)], 70)
    torch.cuda.synchronize()


def test_fr_expanded_trace_feeds_ifft_unchanged(wt):
    from pil2gl import bn128
    w, adds = fr_case(11)
    n_bits, n_cols = 5, 3
    s_map = s_map_for(ref.rng(11), len(w) + len(adds), 1 << n_bits, n_cols)
    ex = fr_exec(w, adds, s_map, 1 << n_bits, n_cols)
    trace = wt.exec_dev(wt.prepare(ex), dev(np.concatenate([ref.fr_words(w), np.zeros((len(adds), 4), np.uint64)])))
    rows = ref.trace(w, fr_values(adds), s_map, 1 << n_bits, n_cols, R)
    built = dev(ref.fr_words([ref.to_mont(v) for r in rows for v in r]).reshape(1 << n_bits, n_cols, 4))
    assert torch.equal(bn128.ifft(trace, n_cols, n_bits), bn128.ifft(built, n_cols, n_bits))
