"""BN254 Fr transforms without a device: the Python checker against itself, the sweep planner, the argument checks of the new entries."""
import ctypes as C
import random

import numpy as np
import pytest

import bn128_fft_ref as ref
from bn128_fft_ref import R

ENTRIES = ("pil2gl_bn128_fft", "pil2gl_bn128_ifft", "pil2gl_bn128_interpolate",
           "pil2gl_bn128_fft_dev", "pil2gl_bn128_ifft_dev", "pil2gl_bn128_interpolate_dev")
EINVAL, ENODEV = -1, -2


def _rand(n, seed):
    rng = random.Random(seed)
    return [rng.randrange(R) for _ in range(n)]


# ---- the checker against itself ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_bits", range(7))
def test_ntt_is_the_definition(n_bits):
    x = _rand(1 << n_bits, n_bits)
    assert ref.ntt(x) == ref.dft_naive(x)


@pytest.mark.parametrize("n_bits", (0, 1, 4, 9))
def test_intt_inverts_ntt(n_bits):
    x = _rand(1 << n_bits, 100 + n_bits)
    assert ref.intt(ref.ntt(x)) == x
    assert ref.ntt(ref.intt(x)) == x


@pytest.mark.parametrize("n_bits", (1, 3, 6))
def test_ntt_of_the_second_unit_vector_is_the_roots(n_bits):
    n = 1 << n_bits
    g = ref.w(n_bits)
    assert ref.ntt([0, 1] + [0] * (n - 2)) == [pow(g, j, R) for j in range(n)]


def test_roots_of_unity():
    assert ref.w(28) == ref.W28 == 19103219067921713944291392827692070036145651957329286315305642004821462161904
    assert pow(ref.w(28), 1 << 28, R) == 1 and pow(ref.w(28), 1 << 27, R) == R - 1       # order exactly 2^28
    assert ref.w(1) == R - 1 and ref.w(0) == 1
    assert all(pow(ref.w(k + 1), 2, R) == ref.w(k) for k in range(28))
    assert pow(5, (R - 1) // 2, R) == R - 1 and all(pow(a, (R - 1) // 2, R) == 1 for a in (2, 3, 4))     # 5: the smallest non-residue


def test_interpolate_is_ntt_of_padded_coefficients():
    x = _rand(8, 7)
    coefs, ext = ref.interpolate(x, 5)
    assert coefs == ref.intt(x) and ext == ref.dft_naive(coefs + [0] * 24)
    assert ext[::4] == x                                                                   # no coset shift: the points themselves come back


def test_montgomery_words_round_trip():
    cols = [_rand(4, 1), _rand(4, 2)]
    wd = ref.matrix_words(cols)
    assert wd.shape == (4, 2, 4) and ref.matrix_cols(wd) == cols
    assert ref.ints_of(wd[1, 0])[0] == cols[0][1] * (1 << 256) % R


# ---- the closed form of a geometric column ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_bits", range(1, 11))
def test_geometric_closed_form_is_the_transform_on_every_row(n_bits):
    n = 1 << n_bits
    rng = random.Random(300 + n_bits)
    for c, a in ((rng.randrange(1, R), rng.randrange(2, R)), (R - 1, 2), (1, R - 2), (rng.randrange(1, R), 0)):
        assert pow(a, n, R) != 1
        x = [c * pow(a, j, R) % R for j in range(n)]
        assert ref.geometric_ntt_rows(c, a, n_bits, range(n)) == ref.ntt(x)
        assert ref.geometric_ntt_rows(c, a, n_bits, range(n), inverse=True) == ref.intt(x)
        assert ref.matrix_cols(ref.geometric_words(c, a, n_bits).reshape(n, 1, 4)) == [x]
    some = [n - 1, 0, n // 2, 0]                                       # any order, repeats allowed
    assert ref.geometric_ntt_rows(c, a, n_bits, some) == [ref.ntt(x)[k] for k in some]


@pytest.mark.parametrize("n_bits", range(1, 11))
def test_geometric_closed_form_refuses_a_zero_denominator(n_bits):
    g = ref.w(n_bits)
    for a in (1, g, pow(g, 3, R), pow(g, -1, R), R - 1, 1 + R):
        for inverse in (False, True):
            with pytest.raises(ValueError):
                ref.geometric_ntt_rows(5, a, n_bits, [0, 1], inverse=inverse)
    assert ref.geometric_ntt_rows(5, ref.w(n_bits + 1), n_bits, [0]) == [5 * (R - 2) * pow(ref.w(n_bits + 1) - 1, -1, R) % R]   # a^n = -1


def test_batch_inverse_and_packed_words():
    v = _rand(50, 9) + [1, R - 1]
    assert [a * b % R for a, b in zip(v, ref.batch_inverse(v))] == [1] * len(v)
    with pytest.raises(AssertionError):
        ref.batch_inverse([3, 0, 5])
    assert (ref.pack_words(v) == ref.words_of(v)).all()


# ---- chosen words into the twiddle products ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_bits", range(1, 8))
def test_dif_layers_are_the_transform(n_bits):
    import bn128_fft_dif as dif
    x = _rand(1 << n_bits, 500 + n_bits)
    out, met = dif.dif(x)
    assert out == ref.ntt(x) and {(t, j) for _, t, j in met} == dif.twiddles_of(n_bits)
    assert dif.dif(x, inverse=True)[0] == ref.intt(x)


@pytest.mark.parametrize("n_bits", (2, 3))
def test_chosen_words_meet_every_twiddle(n_bits):
    """the columns of twiddle_cases put each chosen word itself, as the difference a - b, in front of every twiddle of the size"""
    import bn128_fft_dif as dif
    from test_gpu_bn128_fft import chosen_pairs
    words = dif.chosen_words(chosen_pairs())
    ones = (0x30644e71 << 224) | ((1 << 224) - 1)
    assert {ones, R - 1, (1 << 255) % R, 1, 1 << 31, 1 << 32, 1 << 63, 1 << 64, 1 << 127, 1 << 128, 1 << 191, 1 << 192,
            1 << 223, 1 << 224, 1 << 253} <= set(words) and 0 not in words and len(set(words)) == len(words)
    for x in words:
        for inverse in (False, True):
            met = set()
            for col in dif.twiddle_cases(n_bits, x):
                assert len(col) == 1 << n_bits and all(0 <= v < R for v in col)
                out, m = dif.dif(col, inverse)
                assert out == (ref.intt if inverse else ref.ntt)(col)
                met |= m
            assert {(x, t, j) for t, j in dif.twiddles_of(n_bits)} <= met
            if n_bits == 2:
                assert (2 * x % R, 1, 1) in met and (0, 1, 0) in met


# ---- the library: planner, argument checks, no device ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    import pil2gl
    return pil2gl.load()


def _plan(lib, n_bits, room=8):
    layers = (C.c_uint32 * max(room, 1))()
    n = C.c_uint32(99)
    rc = lib.pil2gl_debug_bn128_fft_plan(n_bits, layers, room, C.byref(n))
    return rc, list(layers[:n.value]) if rc == 0 else n.value


def test_every_new_symbol_is_exported(lib):
    for name in ENTRIES + ("pil2gl_debug_bn128_fft_plan", "pil2gl_debug_bn128_fft_tile_bytes"):
        assert hasattr(lib, name)


@pytest.mark.parametrize("n_bits", range(29))
def test_plan_layers_sum_to_nbits_and_fit_lds(lib, n_bits):
    rc, layers = _plan(lib, n_bits)
    assert rc == 0 and sum(layers) == n_bits and all(k >= 1 for k in layers)
    limit = lib.pil2gl_debug_bn128_fft_tile_bytes()
    assert 32 <= limit <= 160 * 1024                                  # what a gfx950 workgroup can have
    assert all((32 << k) <= limit for k in layers)                   # a tile of 2^k rows x one column fits
    assert all(k <= 10 for k in layers)                              # the tile twiddle table holds the 512 powers of w[10]
    assert (n_bits == 0) == (layers == [])


def test_plan_refuses_what_fr_has_no_root_for(lib):
    assert _plan(lib, 29)[0] == EINVAL
    assert _plan(lib, 28, room=1) == (EINVAL, 3)                     # the count still comes back
    assert lib.pil2gl_debug_bn128_fft_plan(4, None, 4, None) == EINVAL


def _call(lib, name, src, n_pols, n_bits, dst, n_bits_ext=None, coefs=None):
    f = getattr(lib, name)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    args = [p(src), n_pols, n_bits]
    args += [p(coefs), p(dst), n_bits if n_bits_ext is None else n_bits_ext] if "interpolate" in name else [p(dst)]
    if name.endswith("_dev"):
        args.append(None)
    return f(*args)


@pytest.mark.parametrize("name", ENTRIES)
def test_argument_errors_come_before_any_device_call(lib, name):
    buf = np.zeros(64, np.uint64)
    assert _call(lib, name, buf, 1, 29, buf) == EINVAL               # no root of unity of order 2^29
    assert _call(lib, name, None, 1, 2, buf) == EINVAL
    assert _call(lib, name, buf, 1, 2, None) == EINVAL
    if "interpolate" in name:
        assert _call(lib, name, buf, 1, 3, buf, n_bits_ext=2) == EINVAL
        assert _call(lib, name, buf, 1, 3, buf, n_bits_ext=29) == EINVAL
    assert _call(lib, name, buf, 1, 29, buf) == EINVAL and b"2^29" in lib.pil2gl_last_error()


def _have_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


@pytest.mark.skipif(_have_gpu(), reason="only meaningful on a machine without a GPU")
@pytest.mark.parametrize("name", ENTRIES)
def test_compute_entries_need_a_device(lib, name):
    src, dst = np.zeros(2 * 4 * 4, np.uint64), np.zeros(2 * 8 * 4, np.uint64)
    assert _call(lib, name, src, 2, 2, dst, n_bits_ext=3, coefs=np.zeros(2 * 4 * 4, np.uint64)) == ENODEV


def test_python_mirror_has_the_three_transforms():
    from pil2gl import bn128
    assert all(callable(getattr(bn128, k)) for k in ("fft", "ifft", "interpolate"))
