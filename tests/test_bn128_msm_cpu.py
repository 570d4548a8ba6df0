"""BN254 G1 multi-scalar multiplication without a device: the Python checker against itself, the signed-digit recoding and the planner
through the library's host-only entries, the argument checks of the compute entries, and the host code (Fq constants, recoding,
planner) run once more in a stand-alone program built with the address and undefined-behaviour sanitizers."""
import ctypes as C
import json
import os
import random
import subprocess

import numpy as np
import pytest

import bn128_g1_ref as ref
from bn128_g1_ref import G, Q, R
from conftest import ROOT

EINVAL, ENODEV = -1, -2
CSRC = os.path.join(ROOT, "pil2-stark-js_amd", "csrc")
WIDTHS = range(4, 17)                                # the planner's range of c


# ---- the checker against itself ------------------------------------------------------------------------------------------------
def test_generator_and_group_order():
    assert ref.on_curve(G) and not ref.on_curve((1, 3))
    assert ref.mul(R, G) is None
    assert ref.mul(R - 1, G) == ref.neg(G) == (1, Q - 2)
    assert ref.add(G, ref.neg(G)) is None and ref.add(G, None) == G and ref.add(G, G) == ref.mul(2, G)
    assert ref.on_curve(ref.mul(123456789, G))


@pytest.mark.parametrize("n", (1, 2, 17))
def test_known_log_shortcut_equals_the_naive_msm(n):
    pts, logs = ref.known_log_bases(n, seed=n)
    assert all(ref.on_curve(p) and p == ref.mul(k, G) for p, k in zip(pts, logs))
    rng = random.Random(50 + n)
    s = [rng.randrange(R) for _ in range(n)]
    assert ref.expected_from_logs(s, logs) == ref.msm(s, pts)


def test_byte_formats_round_trip():
    pts = [ref.mul(5, G), None, G]
    w = ref.point_words(pts)
    assert w.shape == (3, 8) and not w[1].any() and [ref.point_of(r) for r in w] == pts
    assert int(w[2, 0]) | int(w[2, 1]) << 64 | int(w[2, 2]) << 128 | int(w[2, 3]) << 192 == (1 << 256) % Q      # x = 1 in Montgomery form
    assert ref.scalar_words([1], False).tolist() == [[1, 0, 0, 0]]


# ---- the library's host-only entries -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    import pil2gl
    return pil2gl.load()


def lib_plan(lib, n):
    out = (C.c_uint32 * 4)()
    nbytes = C.c_uint64(1)
    rc = lib.pil2gl_debug_bn128_msm_plan(n, out, C.byref(nbytes))
    return rc, tuple(out), nbytes.value


def lib_digits(lib, s, c, room=64):
    words = (C.c_uint64 * 4)(*[(s >> (64 * k)) & (2 ** 64 - 1) for k in range(4)])
    d = (C.c_int32 * max(room, 1))()
    n = C.c_uint32(999)
    rc = lib.pil2gl_debug_bn128_msm_digits(words, c, d, room, C.byref(n))
    return rc, (list(d[:n.value]) if rc == 0 else n.value)


def test_every_new_symbol_is_exported(lib):
    for name in ("pil2gl_bn128_g1_msm", "pil2gl_bn128_g1_msm_dev", "pil2gl_debug_bn128_msm_plan", "pil2gl_debug_bn128_msm_digits"):
        assert hasattr(lib, name)
    from pil2gl import bn128
    assert callable(bn128.g1_msm)


@pytest.mark.parametrize("c", WIDTHS)
def test_digits_are_in_range_and_recombine(lib, c):
    n_w, half = -(-255 // c), 1 << (c - 1)
    for s in ref.edge_scalars(c):
        rc, d = lib_digits(lib, s, c)
        assert rc == 0 and len(d) == n_w, hex(s)
        assert all(-(half - 1) <= x <= half for x in d), hex(s)
        assert sum(x << (c * w) for w, x in enumerate(d)) == s, hex(s)
        assert d == ref.digits(s, c), hex(s)
    rng = random.Random(c)
    for _ in range(50):
        s = rng.randrange(R)
        assert lib_digits(lib, s, c) == (0, ref.digits(s, c))


def test_digits_cover_the_planned_windows(lib):
    for k in range(29):
        rc, (c, n_w, nbw, g), _ = lib_plan(lib, 1 << k)
        assert rc == 0 and len(lib_digits(lib, R - 1, c)[1]) == n_w


def test_digits_refuse_bad_arguments(lib):
    assert lib_digits(lib, 1, 3)[0] == EINVAL and lib_digits(lib, 1, 17)[0] == EINVAL
    assert lib_digits(lib, 1 << 254, 8)[0] == EINVAL
    assert lib_digits(lib, 1, 8, room=4) == (EINVAL, 32)            # the count still comes back
    assert lib.pil2gl_debug_bn128_msm_digits(None, 8, None, 0, None) == EINVAL


def test_plan_is_monotone_covers_the_scalar_and_bounds_its_scratch(lib):
    last_c = 0
    for k in range(29):
        n = 1 << k
        rc, (c, n_w, nbw, g), nbytes = lib_plan(lib, n)
        assert rc == 0
        assert 4 <= c <= 16 and c >= last_c                         # monotone in n
        last_c = c
        assert n_w * c >= 255                                        # 254 bits and the recoding's carry
        assert (n_w - 1) * c < 255                                   # and no window that is always empty
        assert nbw == 1 << (c - 1) and 1 <= g <= n_w
        assert 0 < nbytes <= ref.scratch_bound(n)
        assert nbytes >= 4 * n * g + 128 * n_w * nbw                 # the point lists of a pass and every window's buckets fit
        assert (c, n_w, nbw, g) == ref.plan(n)
    for n in (3, 1000, 65535, 65537, (1 << 28) - 1):
        rc, p, nbytes = lib_plan(lib, n)
        assert rc == 0 and p == ref.plan(n) and nbytes <= ref.scratch_bound(n)


def test_plan_handles_zero_and_refuses_too_many(lib):
    rc, p, nbytes = lib_plan(lib, 0)
    assert rc == 0 and p == ref.plan(1) and nbytes == 0
    assert lib_plan(lib, (1 << 28) + 1)[0] == EINVAL
    assert lib.pil2gl_debug_bn128_msm_plan(4, None, None) == EINVAL


# ---- argument checks of the compute entries ----------------------------------------------------------------------------------------
def _msm(lib, name, bases, scalars, n, stride, out, mont=1):
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    args = [p(bases), p(scalars), n, stride, mont, p(out)]
    if name.endswith("_dev"):
        args.append(None)
    return getattr(lib, name)(*args)


def _have_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


@pytest.mark.parametrize("name", ("pil2gl_bn128_g1_msm", "pil2gl_bn128_g1_msm_dev"))
def test_argument_errors_come_before_any_device_call(lib, name):
    b, s, o = np.zeros(16, np.uint64), np.zeros(8, np.uint64), np.ones(8, np.uint64)
    assert _msm(lib, name, None, s, 2, 1, o) == EINVAL
    assert _msm(lib, name, b, None, 2, 1, o) == EINVAL
    assert _msm(lib, name, b, s, 2, 1, None) == EINVAL
    assert _msm(lib, name, b, s, 2, 0, o) == EINVAL and b"scalarStride" in lib.pil2gl_last_error()
    assert _msm(lib, name, b, s, (1 << 28) + 1, 1, o) == EINVAL and b"2^28" in lib.pil2gl_last_error()
    assert (o == 1).all()                                            # nothing was written


def test_host_form_of_an_empty_sum_needs_no_device(lib):
    o = np.ones(8, np.uint64)
    assert _msm(lib, "pil2gl_bn128_g1_msm", None, None, 0, 1, o) == 0 and not o.any()


def test_compute_entries_need_a_device(lib):
    """the calls the argument checks above reject, with valid arguments, reach the device layer: without a device both forms say so;
    with one the host form computes (the device form takes device pointers: tests/test_gpu_bn128_msm.py)"""
    b, s, o = ref.point_words([G, G]).reshape(-1), ref.scalar_words([1, 2]).reshape(-1), np.zeros(8, np.uint64)
    if _have_gpu():
        assert _msm(lib, "pil2gl_bn128_g1_msm", b, s, 2, 1, o) == 0 and ref.point_of(o) == ref.mul(3, G)
        return
    for name in ("pil2gl_bn128_g1_msm", "pil2gl_bn128_g1_msm_dev"):
        assert _msm(lib, name, b, s, 2, 1, o) == ENODEV
        assert _msm(lib, name, b, s, 1, 1, o) == ENODEV


# ---- the host code under the sanitizers, in a program of its own ----------------------------------------------------------------------
def test_host_code_under_the_sanitizers_matches_python(tmp_path):
    exe = str(tmp_path / "bn_msm_dump")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                           os.path.join(ROOT, "tests", "bn_msm_dump.cpp"), os.path.join(CSRC, "bn_params.cpp"), "-o", exe])
    cases = [(c, s) for c in WIDTHS for s in ref.edge_scalars(c)]
    (tmp_path / "scalars.txt").write_text("".join("%d %064x\n" % cs for cs in cases))
    sizes = [0, 1, 2, 3, 1000] + [1 << k for k in range(29)] + [(1 << k) + 1 for k in range(28)]
    run = subprocess.run([exe, str(tmp_path / "scalars.txt")] + [str(n) for n in sizes], capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", "sanitizer report or failure:\n" + run.stderr
    got = json.loads(run.stdout)
    mont = 1 << 256
    assert int(got["q"], 16) == Q
    assert int(got["R"], 16) == mont % Q and int(got["R2"], 16) == mont * mont % Q and int(got["R3"], 16) == 3 * mont % Q
    assert got["n0inv"] == (-pow(Q, -1, 1 << 32)) % (1 << 32)
    assert got["digits"] == [ref.digits(s, c) for c, s in cases]
    for n in sizes:
        c, n_w, nbw, g, nbytes = got["plans"][str(n)]
        assert (c, n_w, nbw, g) == ref.plan(n) and nbytes <= ref.scratch_bound(n), n
