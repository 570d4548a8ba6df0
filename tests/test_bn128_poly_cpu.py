"""BN254 Fr polynomial division / evaluation without a device: the Python checker against its multiply-back identity and against the
reference's low-to-high divZh recurrence, the ABI surface (symbols, argument checks before any device call, ENODEV), and the planner
through the library's host-only entry."""
import ctypes as C
import random

import numpy as np
import pytest

import bn128_poly_ref as ref
from bn128_poly_ref import R

EINVAL, ENODEV = -1, -2
MAX_N = 1 << 28
SEG_MIN, LANES = 32, 1 << 17                          # bn_poly_plan.h: the shortest segment, the lanes segments are cut for
SCRATCH_BOUND = 16 * 1024 + 9 * 1024 * 1024           # include/pil2gl.h: the multipliers and, below 9 MiB, the segment values
SYMBOLS = ("pil2gl_bn128_poly_div_xk_sub", "pil2gl_bn128_poly_div_xk_sub_dev", "pil2gl_bn128_poly_eval", "pil2gl_bn128_poly_eval_dev",
           "pil2gl_debug_bn128_poly_plan")


# ---- the checker against itself ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (1, 2, 3, 7, 64, 65, 200))
def test_quotient_times_divisor_plus_remainder_is_the_dividend(n):
    rng = random.Random(n)
    c = ref.rand_elems(n, n)
    for k in sorted({1, 2, 3, 5, 64, max(n - 1, 1), n, n + 1}):
        for beta in (0, 1, R - 1, 2, rng.randrange(R)):
            q, rem = ref.divmod_xk(c, k, beta)
            assert len(rem) == min(k, n) and len(q) == max(n - k, 0)
            assert ref.mul_back(q, rem, k, beta)[:n] == c, (n, k, beta)
            if k >= n:
                assert rem == c                                   # k >= n copies


def test_the_first_element_of_a_division_by_x_minus_z_is_the_value():
    c = ref.rand_elems(50, 1)
    for z in (0, 1, R - 1, 12345, ref.rand_elems(1, 2)[0]):
        want = sum(v * pow(z, i, R) for i, v in enumerate(c)) % R
        assert ref.evaluate(c, z) == want and ref.scan(c, 1, z)[0] == want
    assert ref.evaluate([], 5) == 0


@pytest.mark.parametrize("N,ext", ((1, 4), (4, 2), (16, 4), (8, 3)))
def test_divzh_from_the_top_equals_the_reference_recurrence_from_the_low_end(N, ext):
    n = N * ext
    q = ref.rand_elems(n - N, N)
    c = ref.mul_back(q, [0] * N, N, 1)                            # q * (x^N - 1)
    d = ref.scan(c, N, 1)
    assert d[:N] == [0] * N and d[N:] == q
    assert ref.divzh_low_to_high(c, N) == (q, True)
    c[3 % n] = (c[3 % n] + 1) % R                                 # no longer divisible: both ends say so
    assert any(ref.scan(c, N, 1)[:N]) and not ref.divzh_low_to_high(c, N)[1]


def test_word_helpers_round_trip():
    v = [0, 1, R - 1, ref.MONT] + ref.limb_pattern_elems(20, 3)
    assert all(x < R for x in v) and ref.ints(ref.words(v)) == v
    assert ref.words([1 | 2 << 64 | 3 << 128 | 4 << 192]).tolist() == [[1, 2, 3, 4]]
    assert ref.mont(1) == ref.MONT and ref.mont(ref.MONT_INV) == 1


# ---- the ABI surface ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    import pil2gl
    return pil2gl.load()


def test_every_new_symbol_is_exported(lib):
    for name in SYMBOLS:
        assert hasattr(lib, name)
    from pil2gl import bn128
    assert callable(bn128.poly_div) and callable(bn128.poly_eval) and callable(bn128.poly_plan)


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _div(lib, name, src, n, stride, k, beta, dst):
    args = [_p(src), n, stride, k, _p(beta), _p(dst)]
    return getattr(lib, name)(*(args + [None] if name.endswith("_dev") else args))


def _eval(lib, name, src, n, stride, pts, n_pts, out):
    args = [_p(src), n, stride, _p(pts), n_pts, _p(out)]
    return getattr(lib, name)(*(args + [None] if name.endswith("_dev") else args))


@pytest.mark.parametrize("name", SYMBOLS[:2])
def test_division_argument_errors_come_before_any_device_call(lib, name):
    c, b, d = np.ones(16, np.uint64), np.ones(4, np.uint64), np.full(16, 7, np.uint64)
    assert _div(lib, name, None, 4, 1, 1, b, d) == EINVAL
    assert _div(lib, name, c, 4, 1, 1, None, d) == EINVAL
    assert _div(lib, name, c, 4, 1, 1, b, None) == EINVAL
    assert _div(lib, name, c, MAX_N + 1, 1, 1, b, d) == EINVAL and b"2^28" in lib.pil2gl_last_error()
    assert _div(lib, name, c, 4, 0, 1, b, d) == EINVAL and b"stride" in lib.pil2gl_last_error()
    assert _div(lib, name, c, 4, 1 << 32, 1, b, d) == EINVAL and b"stride" in lib.pil2gl_last_error()
    assert _div(lib, name, c, 4, 1, 0, b, d) == EINVAL and b"k = 0" in lib.pil2gl_last_error()
    assert _div(lib, name, c, 4, 1, MAX_N + 1, b, d) == EINVAL
    assert _div(lib, name, None, 0, 1, 1, None, None) == EINVAL      # beta is always needed
    assert (d == 7).all() and (c == 1).all()                         # nothing was written


@pytest.mark.parametrize("name", SYMBOLS[2:4])
def test_evaluation_argument_errors_come_before_any_device_call(lib, name):
    c, z, o = np.ones(16, np.uint64), np.ones(4 * 65, np.uint64), np.full(4 * 65, 7, np.uint64)
    assert _eval(lib, name, None, 4, 1, z, 1, o) == EINVAL
    assert _eval(lib, name, c, 4, 1, None, 1, o) == EINVAL
    assert _eval(lib, name, c, 4, 1, z, 1, None) == EINVAL
    assert _eval(lib, name, c, MAX_N + 1, 1, z, 1, o) == EINVAL
    assert _eval(lib, name, c, 4, 0, z, 1, o) == EINVAL and _eval(lib, name, c, 4, 1 << 32, z, 1, o) == EINVAL
    assert _eval(lib, name, c, 4, 1, z, 0, o) == EINVAL and b"nPoints" in lib.pil2gl_last_error()
    assert _eval(lib, name, c, 4, 1, z, 65, o) == EINVAL and b"nPoints" in lib.pil2gl_last_error()
    assert (o == 7).all()


def test_host_forms_of_an_empty_polynomial_need_no_device(lib):
    b, o = np.ones(4, np.uint64), np.ones(8, np.uint64)
    assert _div(lib, SYMBOLS[0], None, 0, 1, 1, b, None) == 0
    assert _eval(lib, SYMBOLS[2], None, 0, 1, np.ones(8, np.uint64), 2, o) == 0 and not o.any()


def _have_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


def test_compute_entries_need_a_device(lib):
    """valid arguments reach the device layer: without a device every form says so; with one the host forms compute (the device
    forms take device pointers: tests/test_gpu_bn128_poly.py)"""
    c = ref.rand_elems(5, 9)
    w, b, d, o = ref.words(c), ref.words([ref.mont(3)]), np.zeros((5, 4), np.uint64), np.zeros((1, 4), np.uint64)
    if _have_gpu():
        assert _div(lib, SYMBOLS[0], w, 5, 1, 2, b, d) == 0 and ref.ints(d) == ref.scan(c, 2, 3)
        assert _eval(lib, SYMBOLS[2], w, 5, 1, b, 1, o) == 0 and ref.ints(o) == [ref.evaluate(c, 3)]
        return
    for name in SYMBOLS[:2]:
        assert _div(lib, name, w, 5, 1, 2, b, d) == ENODEV
    for name in SYMBOLS[2:4]:
        assert _eval(lib, name, w, 5, 1, b, 1, o) == ENODEV
    assert not d.any() and not o.any()


# ---- the planner ---------------------------------------------------------------------------------------------------------------------
def plan(lib, n, k):
    info = (C.c_uint32 * 5)()
    nbytes = C.c_uint64(1)
    rc = lib.pil2gl_debug_bn128_poly_plan(n, k, info, C.byref(nbytes))
    return rc, tuple(info), nbytes.value


def sizes():
    ns = {0, 1, 2, 3, 7, 31, 32, 33, 64, 65, 1000, 1023, 1024, 1025, MAX_N}
    for j in range(1, 29):
        ns |= {(1 << j) - 1, 1 << j, min((1 << j) + 1, MAX_N)}
    return sorted(ns)


def strides_of(n):
    return sorted(k for k in {1, 2, 3, 1 << 10, 1 << 20, n, n + 1} if 1 <= k <= MAX_N)


def test_plan_covers_the_vector_bounds_its_scratch_and_has_no_carries_without_segments(lib):
    for n in sizes():
        for k in strides_of(n):
            rc, (L, S, levels, threads, form), nbytes = plan(lib, n, k)
            assert rc == 0, (n, k)
            M = -(-n // k)
            assert L >= 1 and S >= 1 and L * S * k >= n, (n, k)
            assert (S - 1) * L < max(M, 1), (n, k)                   # no segment that is always empty
            assert nbytes <= SCRATCH_BOUND, (n, k)
            assert (S == 1) == (levels == 0) == (form == 0), (n, k)
            if form == 0:
                assert nbytes == 16 * 1024 and L == max(M, 1), (n, k)
            else:
                # at most ceil(M / SEG_MIN) < M / (SEG_MIN / 2) segments, so each is longer than SEG_MIN / 2; no more lanes than asked for
                assert 2 * L > SEG_MIN and S * k < LANES + k, (n, k)
            assert form == (0 if M <= SEG_MIN or k >= LANES else 1), (n, k)
            assert threads == 256


def test_plan_refuses_what_the_compute_entries_refuse(lib):
    assert plan(lib, MAX_N + 1, 1)[0] == EINVAL and plan(lib, 4, 0)[0] == EINVAL and plan(lib, 4, MAX_N + 1)[0] == EINVAL
    assert lib.pil2gl_debug_bn128_poly_plan(4, 1, None, None) == EINVAL


def test_every_carry_level_count_is_reached_by_a_small_shape(lib):
    """what keeps the GPU tests honest: they run shapes of n <= 2^22, so no count of carry levels may exist only above that"""
    ks = (1, 2, 3, 5, 64, 1 << 10, (1 << 16) - 1, 1 << 16, (1 << 16) + 1, (1 << 17) - 1, 1 << 17, 1 << 20)
    everywhere, small = set(), {}
    for n in sizes():
        for k in sorted(set(ks) | set(strides_of(n))):
            levels = plan(lib, n, k)[1][2]
            everywhere.add(levels)
            if n <= 1 << 22 and (levels not in small or n < small[levels][0]):
                small[levels] = (n, k)
    print("carry levels -> a smallest (n, k) among the sizes tried:", sorted(small.items()))
    assert everywhere == set(small) and max(everywhere) >= 3
