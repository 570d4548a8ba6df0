"""BN254 G1 multi-scalar multiplication on the device (pil2gl.bn128.g1_msm over csrc/bn_msm.hip) against the Python checker
(tests/bn128_g1_ref.py).  Every comparison is exact equality of the 64 output bytes.  The bases have known discrete logs, so the
expected point of any scalars is one scalar multiplication on the host; window widths come from the library's planner."""
import ctypes as C
import random

import numpy as np
import pytest

import bn128_g1_ref as ref
from bn128_g1_ref import G, R

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

N_MAX = 1 << 16


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


class Pool:
    """2^16 bases with known logs and as many random scalars, made once; every test takes prefixes and leaves them unchanged"""

    def __init__(self):
        self.points, self.logs = ref.known_log_bases(N_MAX, seed=254)
        self.words = ref.point_words(self.points)
        rng = random.Random(2540)
        self.scalars = [rng.randrange(R) for _ in range(N_MAX)]
        self.scalar_words = ref.scalar_words(self.scalars)


@pytest.fixture(scope="module")
def pool():
    return Pool()


def dev(words):
    return torch.from_numpy(np.ascontiguousarray(words).view(np.int64)).cuda()


def host(t):
    return t.cpu().numpy().view(np.uint64)


def expect(point):
    return ref.point_words([point]).reshape(8)


def plan(lib, n):
    out = (C.c_uint32 * 4)()
    nbytes = C.c_uint64()
    assert lib.pil2gl_debug_bn128_msm_plan(n, out, C.byref(nbytes)) == 0
    return tuple(out)


def run(bn, points, scalars, montgomery=True):
    """through the device entry, from Python values"""
    out = bn.g1_msm(dev(ref.point_words(points)), dev(ref.scalar_words(scalars, montgomery)), n=len(points), montgomery=montgomery)
    return host(out)


def same(got, want_point):
    assert np.array_equal(np.asarray(got).reshape(8), expect(want_point)), "got %s, expected %s" % (ref.point_of(got) if np.asarray(got).any() else None, want_point)


# ---- 1. small counts ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (0, 1, 2, 3, 63, 64, 65, 257, 1000))
def test_small_counts_match_the_checker(bn, pool, n):
    got = host(bn.g1_msm(dev(pool.words[:max(n, 1)]), dev(pool.scalar_words[:max(n, 1)]), n=n))
    same(got, ref.expected_from_logs(pool.scalars[:n], pool.logs[:n]))
    if n <= 65:
        same(got, ref.msm(pool.scalars[:n], pool.points[:n]))


# ---- 2. scalars ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (1, 65, 257))
def test_all_zero_all_one_all_minus_one(bn, pool, n):
    pts, logs = pool.points[:n], pool.logs[:n]
    same(run(bn, pts, [0] * n), None)
    total = ref.mul(sum(logs) % R, G)
    same(run(bn, pts, [1] * n), total)
    same(run(bn, pts, [R - 1] * n), ref.neg(total))


@pytest.mark.parametrize("n", (300, 5000))
def test_recoding_edge_scalars_among_random_ones(bn, lib, pool, n):
    """every edge scalar of the planned window width on a point of its own (spread over the list), random scalars on the others"""
    c = plan(lib, n)[0]
    edges = [s for s in ref.edge_scalars(c) if s < R]
    assert len(edges) <= n
    scalars = list(pool.scalars[:n])
    for k, s in enumerate(edges):
        scalars[(k * 7919) % n if n > len(edges) * 2 else k] = s
    same(run(bn, pool.points[:n], scalars), ref.expected_from_logs(scalars, pool.logs[:n]))
    same(run(bn, pool.points[:n], scalars, montgomery=False), ref.expected_from_logs(scalars, pool.logs[:n]))


def test_each_recoding_edge_scalar_alone_on_one_point(bn, lib, pool):
    n = 3
    c = plan(lib, n)[0]
    for s in [s for s in ref.edge_scalars(c) if s < R][::3] + [R - 1, 1 << 253]:
        scalars = [pool.scalars[0], s, pool.scalars[2]]
        same(run(bn, pool.points[:n], scalars), ref.expected_from_logs(scalars, pool.logs[:n]))


# ---- 3. points ----------------------------------------------------------------------------------------------------------------------
def test_points_at_infinity(bn, pool):
    n = 130
    same(run(bn, [None] * n, pool.scalars[:n]), None)
    pts = [None if i % 3 == 0 else p for i, p in enumerate(pool.points[:n])]
    want = ref.expected_from_logs([0 if p is None else s for s, p in zip(pool.scalars, pts)], pool.logs[:n])
    same(run(bn, pts, pool.scalars[:n]), want)


@pytest.mark.parametrize("n", (64, 4096))
def test_one_point_and_one_scalar_repeated(bn, pool, n):
    """one bucket per window holds everything; its second addition is P + P"""
    p, k, s = pool.points[5], pool.logs[5], pool.scalars[5]
    same(run(bn, [p] * n, [s] * n), ref.mul(n * s * k % R, G))


@pytest.mark.parametrize("n", (64, 65))
def test_point_and_its_negative_alternating(bn, pool, n):
    """a bucket passes through infinity again and again and goes on"""
    p, k, s = pool.points[9], pool.logs[9], pool.scalars[9]
    pts = [p if i % 2 == 0 else ref.neg(p) for i in range(n)]
    same(run(bn, pts, [s] * n), None if n % 2 == 0 else ref.mul(s * k % R, G))


def test_scalar_and_its_complement_cancel(bn, pool):
    p, s = pool.points[11], pool.scalars[11]
    same(run(bn, [p, p], [s, R - s]), None)
    same(run(bn, [p, p, pool.points[12]], [s, R - s, 7]), ref.mul(7 * pool.logs[12] % R, G))


# ---- 4. reduction edges (window width from the planner) -----------------------------------------------------------------------------
@pytest.mark.parametrize("n", (2, 600, 40000))
def test_reduction_edges(bn, lib, pool, n):
    c, n_w, nbw, _ = plan(lib, n)
    k = pool.logs[0]
    bases = pool.words[:n].copy()
    bases[1] = bases[0]                                              # the same point twice; the other points take no part: zero scalars
    d_bases = dev(bases)

    def check(s0, s1):
        scalars = np.zeros((n, 4), np.uint64)
        scalars[:2] = ref.scalar_words([s0, s1])
        same(host(bn.g1_msm(d_bases, dev(scalars), n=n)), ref.mul((s0 + s1) * k % R, G))

    for w in (0, 1, n_w - 2):
        for d in (1, 2, 7, 8, nbw - 1):                              # neighbouring buckets hold the same point: the running sum meets P + P
            check(d << (c * w), (d + 1) << (c * w))
    for w in (0, n_w // 2):
        check(nbw << (c * w), 0)                                     # only the highest bucket
        check(1 << (c * w), 0)                                       # only bucket 1
    top = 1 << (c * (n_w - 1))
    assert top < R
    check(top, 0)                                                    # only the top window
    check(top, top)


# ---- 5. plan boundaries -------------------------------------------------------------------------------------------------------------
_PLANS = [ref.plan(n) for n in range(N_MAX + 1)]                    # the checker's statement of the plan: it places the cases, the library is asked below
BOUNDARIES = [n for n in range(2, N_MAX + 1) if (_PLANS[n][0], _PLANS[n][3]) != (_PLANS[n - 1][0], _PLANS[n - 1][3])]


def test_boundaries_are_the_planners(lib):
    assert BOUNDARIES and max(BOUNDARIES) == N_MAX
    for n in BOUNDARIES:
        a, b = plan(lib, n - 1), plan(lib, n)
        assert (a[0], a[3]) != (b[0], b[3]), n
    assert any(plan(lib, n)[3] < plan(lib, n)[1] for n in BOUNDARIES)        # more than one pass is among them


@pytest.mark.parametrize("n", sorted({m for b in BOUNDARIES for m in (b - 1, b)}))
def test_both_sides_of_every_plan_boundary(bn, pool, n):
    got = host(bn.g1_msm(dev(pool.words[:n]), dev(pool.scalar_words[:n]), n=n))
    same(got, ref.expected_from_logs(pool.scalars[:n], pool.logs[:n]))


# ---- 6. surface ---------------------------------------------------------------------------------------------------------------------
def test_montgomery_and_normal_form_scalars_agree(bn, pool):
    n = 777
    want = ref.expected_from_logs(pool.scalars[:n], pool.logs[:n])
    same(run(bn, pool.points[:n], pool.scalars[:n], montgomery=True), want)
    same(run(bn, pool.points[:n], pool.scalars[:n], montgomery=False), want)


def test_a_strided_column_equals_the_contiguous_one(bn, pool):
    n = 500
    cols = [pool.scalars[j * n:(j + 1) * n] for j in range(3)]
    matrix = np.stack([ref.scalar_words(col) for col in cols], axis=1)          # (n, 3, 4): row-major coefficient matrix
    d_bases, d_matrix = dev(pool.words[:n]), dev(matrix)
    for j in range(3):
        strided = host(bn.g1_msm(d_bases, d_matrix.reshape(-1)[4 * j:], n=n, stride=3))
        packed = host(bn.g1_msm(d_bases, dev(matrix[:, j, :]), n=n))
        same(strided, ref.expected_from_logs(cols[j], pool.logs[:n]))
        assert np.array_equal(strided, packed)
        assert np.array_equal(bn.g1_msm(pool.words[:n].copy(), matrix.reshape(-1)[4 * j:].copy(), n=n, stride=3), strided)      # host pointers


def test_host_pointer_form_equals_the_device_form(bn, pool):
    for n in (1, 100, 3000):
        got = bn.g1_msm(pool.words[:n].copy(), pool.scalar_words[:n].copy())
        assert isinstance(got, np.ndarray)
        same(got, ref.expected_from_logs(pool.scalars[:n], pool.logs[:n]))
        assert np.array_equal(got, host(bn.g1_msm(dev(pool.words[:n]), dev(pool.scalar_words[:n]))))


def test_device_form_is_ordered_on_the_callers_stream(bn, pool):
    n = 2000
    pinned = torch.from_numpy(pool.scalar_words[:n].view(np.int64).copy()).pin_memory()
    d_bases = dev(pool.words[:n])
    d_scalars = torch.zeros_like(pinned, device="cuda")
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        d_scalars.copy_(pinned, non_blocking=True)                   # the MSM must see these, not the zeros
        out = bn.g1_msm(d_bases, d_scalars, n=n)
    stream.synchronize()
    same(host(out), ref.expected_from_logs(pool.scalars[:n], pool.logs[:n]))


def test_large_small_large_in_one_process(bn, pool):
    """stale scratch, stale histograms: the working buffer keeps the first call's contents when the second, smaller one runs"""
    big, small = 1 << 14, 5
    d_bases, d_scalars = dev(pool.words[:big]), dev(pool.scalar_words[:big])
    want_big = ref.expected_from_logs(pool.scalars[:big], pool.logs[:big])
    same(host(bn.g1_msm(d_bases, d_scalars, n=big)), want_big)
    same(host(bn.g1_msm(d_bases, d_scalars, n=small)), ref.expected_from_logs(pool.scalars[:small], pool.logs[:small]))
    same(host(bn.g1_msm(d_bases, d_scalars, n=big)), want_big)
