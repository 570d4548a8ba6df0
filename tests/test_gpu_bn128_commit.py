"""BN254 G1 stage commit on the device (pil2gl.bn128.g1_commit over csrc/bn_msm.hip) against the Python checker
(tests/bn128_g1_packed_ref.py over tests/bn128_g1_ref.py).  Every comparison is exact equality of the 64 output bytes of a polynomial.  The
bases have known discrete logs, so the expected point of a packed polynomial is one scalar multiplication on the host.  One pool of bases
and one flat array of scalars serve every test: a test reads the array as a matrix of the row stride it chooses."""
import ctypes as C
import random

import numpy as np
import pytest

import bn128_g1_ref as ref
import bn128_g1_packed_ref as pref
from bn128_g1_ref import G, R

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

N_BASES = 40000
N_ELEMS = 1 << 16


@pytest.fixture(scope="module")
def bn():
    import pil2gl
    from pil2gl import bn128
    pil2gl.init(0)
    return bn128


@pytest.fixture(scope="module")
def lib():
    import pil2gl
    return pil2gl.load()


def dev(words):
    return torch.from_numpy(np.ascontiguousarray(words).view(np.int64)).cuda()


def host(t):
    return t.cpu().numpy().view(np.uint64)


class Pool:
    """made once, left unchanged: bases with known logs, a flat array of random scalars in both forms, and their device copies"""

    def __init__(self):
        self.points, self.logs = ref.known_log_bases(N_BASES, seed=2254)
        self.words = ref.point_words(self.points)
        rng = random.Random(22540)
        self.matrix = [rng.randrange(R) for _ in range(N_ELEMS)]
        self.mont = ref.scalar_words(self.matrix, True)
        self.normal = ref.scalar_words(self.matrix, False)
        self.d_bases, self.d_mont, self.d_normal = dev(self.words), dev(self.mont), dev(self.normal)


@pytest.fixture(scope="module")
def pool():
    return Pool()


def same(got, want_points):
    got = np.asarray(got).reshape(-1, 8)
    assert got.shape[0] == len(want_points)
    for k, want in enumerate(want_points):
        assert np.array_equal(got[k], ref.point_words([want]).reshape(8)), "polynomial %d: got %s, expected %s" % (
            k, ref.point_of(got[k]) if got[k].any() else None, want)


def check(bn, pool, polys, row_stride, montgomery=True):
    """the batch through the device entry against the checker; -> the (K, 8) words"""
    got = host(bn.g1_commit(pool.d_bases, pool.d_mont if montgomery else pool.d_normal, polys, row_stride, montgomery=montgomery))
    same(got, [pref.expected(pool.matrix, p, row_stride, pool.logs) for p in polys])
    return got


def batch_plan(lib, counts):
    out, nbytes = (C.c_uint32 * 4)(), C.c_uint64()
    assert lib.pil2gl_debug_bn128_msm_batch_plan(len(counts), (C.c_uint64 * len(counts))(*counts), out, C.byref(nbytes)) == 0
    return tuple(out)


# ---- 1. packed = the checker = g1_msm of the interleaved vector ---------------------------------------------------------------------
@pytest.mark.parametrize("rows", (1, 2, 65, 500))
@pytest.mark.parametrize("m", (1, 2, 3, 7, 64))
def test_packed_equals_the_checker_and_the_interleaved_msm(bn, pool, m, rows):
    row_stride = m + 3
    slots = random.Random(100 * m + rows).sample(range(row_stride), m)               # m distinct columns in a shuffled order
    polys = [(0, rows, slots), (5 * row_stride + 1, rows, sorted(slots))]            # the second starts inside a row: its columns wrap into the next
    for montgomery, words in ((True, pool.mont), (False, pool.normal)):
        got = check(bn, pool, polys, row_stride, montgomery)
        for k, poly in enumerate(polys):
            vector = dev(words[[e for e in pref.elements(poly, row_stride)]])       # the packed polynomial as a second buffer
            n = vector.shape[0]
            assert np.array_equal(host(bn.g1_msm(pool.d_bases, vector, n=n, montgomery=montgomery)), got[k])


# ---- 2. empty slots, empty polynomials ----------------------------------------------------------------------------------------------
def test_empty_slots_first_middle_last_and_everywhere(bn, pool):
    polys = [(0, 40, [None, 1, 2, 3]), (0, 40, [0, None, None, 3]), (0, 40, [0, 1, 2, None]), (0, 40, [None] * 4), (8, 3, [None, 2, None])]
    got = check(bn, pool, polys, 4)
    assert not got[3].any()                                           # every slot empty: 64 zero bytes
    check(bn, pool, polys, 4, montgomery=False)


def test_rows_zero_among_polynomials_with_points(bn, pool):
    got = check(bn, pool, [(0, 0, [0, 1]), (0, 300, [2, 0, 1]), (7, 0, [None]), (3, 5, [1]), (0, 0, [2])], 3)
    assert not got[0].any() and not got[2].any() and not got[4].any() and got[1].any() and got[3].any()


def test_an_all_empty_batch_is_zero_bytes(bn, pool):
    out = torch.ones((3, 8), dtype=torch.int64, device="cuda")
    bn.g1_commit(pool.d_bases, pool.d_mont, [(0, 0, [0]), (0, 0, [None, 1]), (0, 0, [1])], 2, out=out)
    assert not host(out).any()
    assert not host(bn.g1_commit(pool.d_bases, pool.d_mont, [(0, 9, [None, None])], 2)).any()       # points, but no coefficient


# ---- 3. points ----------------------------------------------------------------------------------------------------------------------
def test_a_base_at_infinity_at_an_occupied_index(bn, pool):
    n, polys = 200, [(0, 50, [1, 0, 3, 2]), (0, 100, [2, None])]
    points = list(pool.points[:n])
    for i in (0, 5, 6, 199):                                          # slot 0 and others, first row and last; 5 is an empty slot of the second
        points[i] = None
    got = host(bn.g1_commit(dev(ref.point_words(points)), pool.d_mont, polys, 4))
    same(got, [pref.expected(pool.matrix, p, 4, pool.logs, points) for p in polys])


def test_one_point_and_one_scalar_repeated_across_a_packed_polynomial(bn, pool):
    """one bucket per window holds everything; its second addition is P + P, inside a batch"""
    p, k, s = pool.points[5], pool.logs[5], pool.matrix[5]
    bases = dev(ref.point_words([p] * 192))
    scalars = dev(ref.scalar_words([s] * 256))
    got = host(bn.g1_commit(bases, scalars, [(0, 64, [0, 1, 3]), (0, 32, [2, None]), (1, 7, [0])], 4))
    same(got, [ref.mul(192 * s * k % R, G), ref.mul(32 * s * k % R, G), ref.mul(7 * s * k % R, G)])


# ---- 4. batches ---------------------------------------------------------------------------------------------------------------------
def test_very_unequal_sizes_share_blocks_and_one_window_width(bn, lib, pool):
    """n_k of 1, 255, 2, 257 and 40 000: each of the first three 256-lane blocks holds points of two polynomials, and the small ones run
    at the large one's window width"""
    polys = [(3, 1, [2]), (0, 85, [4, 0, 1]), (9, 1, [None, 3]), (1, 257, [0]), (0, 10000, [3, 1, 0, 2])]
    counts = [rows * len(slots) for _, rows, slots in polys]
    assert counts == [1, 255, 2, 257, 40000]
    assert batch_plan(lib, counts)[0] == ref.plan(40000)[0] > ref.plan(257)[0]
    check(bn, pool, polys, 5)
    check(bn, pool, polys[::-1], 5, montgomery=False)


def test_sixteen_commits_of_one_column_are_identical(bn, pool):
    got = check(bn, pool, [(0, 700, [2])] * 16, 3)
    assert got[0].any() and all(np.array_equal(got[0], row) for row in got)


def test_two_polynomials_share_a_column(bn, pool):
    got = check(bn, pool, [(0, 300, [1, 0]), (0, 300, [1]), (0, 150, [2, 1, None, 1])], 3)
    assert len({row.tobytes() for row in got}) == 3


def test_pieces_of_one_coefficient_vector(bn, pool):
    """rowStride = 1, m = 1 and different `first`: Q_0 .. Q_3 of computeQFflonk; then offsets into a wide matrix"""
    check(bn, pool, [(k * 1000, 1000 if k < 3 else 777, [0]) for k in range(4)], 1)
    check(bn, pool, [(1 + 40 * 50, 100, [0, 38]), (39, 900, [0]), (50 * 7 + 3, 2, [46, 0, 45])], 50)


# ---- 5. scalars ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("montgomery", (True, False))
def test_recoding_edge_scalars_in_chosen_slots_and_rows(bn, lib, pool, montgomery):
    """every edge scalar of the batch's window width in a cell of its own: all slots, first, middle and last rows"""
    row_stride, polys = 4, [(0, 150, [3, 0, 2]), (4, 60, [1, None, 2, 0])]
    c = batch_plan(lib, [450, 240])[0]
    edges = [s for s in ref.edge_scalars(c) if s < R]
    cells = sorted({e for p in polys for e in pref.elements(p, row_stride) if e is not None})
    assert len(edges) <= len(cells)
    matrix = list(pool.matrix[:cells[-1] + 1])
    spread = cells[:8] + cells[-8:] + cells[8:-8:max(1, (len(cells) - 16) // len(edges))]
    for cell, s in zip(spread, edges):
        matrix[cell] = s
    assert len(spread) >= len(edges)
    got = host(bn.g1_commit(pool.d_bases, dev(ref.scalar_words(matrix, montgomery)), polys, row_stride, montgomery=montgomery))
    same(got, [pref.expected(matrix, p, row_stride, pool.logs) for p in polys])


# ---- 6. plan boundaries (the checker places the cases, the library is asked) ------------------------------------------------------------
_HALF = N_ELEMS // 2                                                  # K = 2 with equal counts, up to 2^16 points in total
_PLANS = [pref.batch_plan([n, n]) for n in range(_HALF + 1)]
BOUNDARIES = [n for n in range(2, _HALF + 1) if (_PLANS[n][0], _PLANS[n][3]) != (_PLANS[n - 1][0], _PLANS[n - 1][3])]


def test_boundaries_are_the_batch_planners(lib):
    assert BOUNDARIES
    for n in BOUNDARIES:
        a, b = batch_plan(lib, [n - 1, n - 1]), batch_plan(lib, [n, n])
        assert (a[0], a[3]) != (b[0], b[3]), n
    assert any(batch_plan(lib, [n, n])[3] < batch_plan(lib, [n, n])[1] for n in BOUNDARIES)          # a multi-pass batch is among them
    assert any(batch_plan(lib, [n - 1] * 2)[0] != batch_plan(lib, [n] * 2)[0] for n in BOUNDARIES)
    assert any(batch_plan(lib, [n - 1] * 2)[3] != batch_plan(lib, [n] * 2)[3] for n in BOUNDARIES)


@pytest.mark.parametrize("n", sorted({m for b in BOUNDARIES for m in (b - 1, b)} | {_HALF}))
def test_both_sides_of_every_batch_plan_boundary(bn, lib, pool, n):
    if n == _HALF:
        assert batch_plan(lib, [n, n])[3] < batch_plan(lib, [n, n])[1]                # 2^16 points in total, several passes
    check(bn, pool, [(0, n, [1]), (0, n, [0])], 2)


# ---- 7. surface ---------------------------------------------------------------------------------------------------------------------
def test_host_pointer_form_equals_the_device_form(bn, pool):
    polys, row_stride = [(2, 60, [0, None, 3]), (0, 0, [1]), (0, 999, [4])], 5
    got = bn.g1_commit(pool.words.copy(), pool.mont.copy(), polys, row_stride)
    assert isinstance(got, np.ndarray) and got.shape == (3, 8)
    assert np.array_equal(got, check(bn, pool, polys, row_stride))
    top = 4 * 999 * 5                                                 # the host form stages only what the descriptors reach
    assert np.array_equal(bn.g1_commit(pool.words[:999].copy(), pool.mont.reshape(-1)[:top].copy(), polys, row_stride), got)
    with pytest.raises(Exception):
        bn.g1_commit(pool.words[:998].copy(), pool.mont, polys, row_stride)            # fewer bases than the largest polynomial
    with pytest.raises(Exception):
        bn.g1_commit(pool.d_bases, pool.d_mont.reshape(-1)[:top - 4].contiguous(), polys, row_stride)


def test_device_form_is_ordered_on_the_callers_stream(bn, pool):
    polys, n = [(0, 500, [0, 1, None, 3]), (0, 2000, [2])], 8000
    pinned = torch.from_numpy(pool.mont[:n].view(np.int64).copy()).pin_memory()
    d_scalars = torch.zeros_like(pinned, device="cuda")
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        d_scalars.copy_(pinned, non_blocking=True)                    # the commit must see these, not the zeros
        out = bn.g1_commit(pool.d_bases, d_scalars, polys, 4)
    stream.synchronize()
    same(host(out), [pref.expected(pool.matrix, p, 4, pool.logs) for p in polys])


def test_large_small_large_in_one_process(bn, pool):
    """stale scratch, stale histograms: the working buffer keeps the first batch's contents when the second, smaller one runs"""
    big = [(0, 4000, [0, 1, 2, 3]), (0, 8000, [2, None]), (0, 16000, [1])]
    small = [(3, 1, [0]), (0, 2, [1, None, 0])]
    first = check(bn, pool, big, 4)
    check(bn, pool, small, 4)
    assert np.array_equal(check(bn, pool, big, 4), first)


def test_single_msm_before_and_after_a_batch(bn, pool):
    n = 3000
    column = pool.d_mont.reshape(-1)[4 * 2:]
    alone = host(bn.g1_msm(pool.d_bases, column, n=n, stride=3))
    same(alone, [pref.expected(pool.matrix, (0, n, [2]), 3, pool.logs)])
    batch = check(bn, pool, [(0, n, [2]), (0, 1500, [0, 1])], 3)
    assert np.array_equal(batch[0], alone)
    assert np.array_equal(host(bn.g1_msm(pool.d_bases, column, n=n, stride=3)), alone)
