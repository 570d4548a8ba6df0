"""BN254 Fr batch inverse, grand product and grand sum without a device: the Python checker against the defining identities, the ABI
surface (symbols, every refusal before any device call, ENODEV), the Python wrappers' own refusals, the planner through the library's
host-only hook, and the planner header under the sanitizers in a program of its own."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import bn128_hints_ref as ref
from bn128_hints_ref import R
from conftest import ROOT

CSRC = os.path.join(ROOT, "pil2-stark-js_amd", "csrc")
EINVAL, ENODEV = -1, -2
MAX_N = 1 << 28
SEG_MIN, TOP_MAX, LANES = 16, 64, 1 << 17               # bn_scan_plan.h
# include/pil2gl.h: the levels above the first stay below 9 MiB (2 * 32 bytes for each of at most 2^17 + 2^13 + 2^9 + 2^5 items); an
# inversion in place adds its level-0 prefixes, 32 n bytes
UPPER_BOUND = 9 * 1024 * 1024
FIRST_N_OF_LEVELS = {1: 1, 2: 65, 3: 1025, 4: 16385, 5: 262145}
OPS = {"batch_inverse": 0, "gprod": 1, "gsum": 2, "batch_inverse_in_place": 3}
SYMBOLS = ("pil2gl_bn128_batch_inverse", "pil2gl_bn128_batch_inverse_dev", "pil2gl_bn128_gprod", "pil2gl_bn128_gprod_dev",
           "pil2gl_bn128_gsum", "pil2gl_bn128_gsum_dev", "pil2gl_debug_bn128_scan_plan")


def columns(n, seed, zeros=()):
    num, den = ref.rand_elems(n, seed), ref.rand_elems(n, seed + 1000)
    den = [v or 1 for v in den]
    for i in zeros:
        den[i] = 0
    return num, den


# ---- the checker against the definitions ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,zeros", ((1, ()), (2, (0,)), (7, ()), (200, ()), (200, (0, 57, 58, 199)), (5, (0, 1, 2, 3, 4))))
def test_checker_identities(n, zeros):
    num, den = columns(n, n, zeros)
    inv = ref.batch_inverse(den)
    for i in range(n):
        assert (inv[i] * den[i] % R == 1) if den[i] else (inv[i] == 0)
    z = ref.gprod(num, den)
    assert z[0] == 1
    first = min(zeros) if zeros else n
    for i in range(n - 1):
        if i < first:
            assert z[i + 1] * den[i] % R == z[i] * num[i] % R
        else:
            assert z[i + 1] == 0                                  # from the row after the first zero denominator on
    c = num[0]
    s = ref.gsum(c, den)
    for i in range(n):
        assert (s[i] - (s[i - 1] if i else 0)) * den[i] % R == (c if den[i] else 0)
        if not den[i]:
            assert s[i] == (s[i - 1] if i else 0)


def test_checker_conversions():
    v = [0, 1, R - 1, (1 << 255) % R] + ref.rand_elems(5, 3)
    assert ref.plain(ref.mont_words(v)) == v and [ref.unmont(ref.mont(x)) for x in v] == v


# ---- the ABI surface -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    import pil2gl
    return pil2gl.load()


def test_every_new_symbol_is_exported(lib):
    for name in SYMBOLS:
        assert hasattr(lib, name)
    from pil2gl import bn128
    assert all(callable(getattr(bn128, f)) for f in ("batch_inverse", "gprod", "gsum", "scan_plan"))


def _p(a, byte_offset=0):
    return None if a is None else C.c_void_p(a.ctypes.data + byte_offset)


def _inv(lib, name, src, ss, n, dst, ds):
    args = [src, ss, n, dst, ds]
    return getattr(lib, name)(*(args + [None] if name.endswith("_dev") else args))


def _gprod(lib, name, num, ns, den, ds, n, out, os_):
    args = [num, ns, den, ds, n, out, os_]
    return getattr(lib, name)(*(args + [None] if name.endswith("_dev") else args))


def _gsum(lib, name, e, den, ds, n, out, os_):
    args = [e, den, ds, n, out, os_]
    return getattr(lib, name)(*(args + [None] if name.endswith("_dev") else args))


@pytest.mark.parametrize("dev", (False, True))
def test_every_refusal_comes_before_any_device_call(lib, dev):
    """all of them through the host-pointer entries AND the _dev entries (which check their arguments as host integers first); the size
    refusal through the planner hook as well"""
    sfx = "_dev" if dev else ""
    a, b, o = np.ones(4 * 64, np.uint64), np.ones(4 * 64, np.uint64), np.full(4 * 64, 7, np.uint64)
    e = np.ones(4, np.uint64)
    inv, gp, gs = "pil2gl_bn128_batch_inverse" + sfx, "pil2gl_bn128_gprod" + sfx, "pil2gl_bn128_gsum" + sfx
    # n > 2^28
    assert _inv(lib, inv, _p(a), 1, MAX_N + 1, _p(o), 1) == EINVAL and b"2^28" in lib.pil2gl_last_error()
    assert _gprod(lib, gp, _p(a), 1, _p(b), 1, MAX_N + 1, _p(o), 1) == EINVAL and _gsum(lib, gs, _p(e), _p(b), 1, MAX_N + 1, _p(o), 1) == EINVAL
    # stride 0 and 2^32, every column
    for bad in (0, 1 << 32):
        assert _inv(lib, inv, _p(a), bad, 4, _p(o), 1) == EINVAL and b"stride" in lib.pil2gl_last_error()
        assert _inv(lib, inv, _p(a), 1, 4, _p(o), bad) == EINVAL
        assert _gprod(lib, gp, _p(a), bad, _p(b), 1, 4, _p(o), 1) == EINVAL and _gprod(lib, gp, _p(a), 1, _p(b), bad, 4, _p(o), 1) == EINVAL
        assert _gprod(lib, gp, _p(a), 1, _p(b), 1, 4, _p(o), bad) == EINVAL
        assert _gsum(lib, gs, _p(e), _p(b), bad, 4, _p(o), 1) == EINVAL and _gsum(lib, gs, _p(e), _p(b), 1, 4, _p(o), bad) == EINVAL
    # null buffers with n > 0; gsum's numerator always
    assert _inv(lib, inv, None, 1, 4, _p(o), 1) == EINVAL and _inv(lib, inv, _p(a), 1, 4, None, 1) == EINVAL
    assert _gprod(lib, gp, None, 1, _p(b), 1, 4, _p(o), 1) == EINVAL and _gprod(lib, gp, _p(a), 1, None, 1, 4, _p(o), 1) == EINVAL
    assert _gprod(lib, gp, _p(a), 1, _p(b), 1, 4, None, 1) == EINVAL
    assert _gsum(lib, gs, None, _p(b), 1, 4, _p(o), 1) == EINVAL and _gsum(lib, gs, _p(e), None, 1, 4, _p(o), 1) == EINVAL
    assert _gsum(lib, gs, _p(e), _p(b), 1, 4, None, 1) == EINVAL and _gsum(lib, gs, None, None, 1, 0, None, 1) == EINVAL
    # overlapping distinct columns: shifted rows of one column, another stride over the same bytes, a hint writing over its input
    assert _inv(lib, inv, _p(a), 1, 8, _p(a, 32), 1) == EINVAL and b"overlaps" in lib.pil2gl_last_error()
    assert _inv(lib, inv, _p(a), 2, 8, _p(a), 1) == EINVAL
    assert _inv(lib, inv, _p(a), 3, 8, _p(a, 32 * 6), 3) == EINVAL          # the same column two rows on
    assert _inv(lib, inv, _p(a), 3, 8, _p(a, 8), 3) == EINVAL               # not element-aligned
    assert _gprod(lib, gp, _p(a), 1, _p(b), 1, 8, _p(a), 1) == EINVAL and _gprod(lib, gp, _p(a), 1, _p(b), 1, 8, _p(b), 1) == EINVAL
    assert _gsum(lib, gs, _p(e), _p(b), 1, 8, _p(b), 1) == EINVAL          # only batch_inverse runs in place
    # n = 0 is OK, touches nothing, needs no device
    assert _inv(lib, inv, None, 1, 0, None, 1) == 0 and _gprod(lib, gp, None, 1, None, 1, 0, None, 1) == 0
    assert _gsum(lib, gs, _p(e), None, 1, 0, None, 1) == 0
    assert (o == 7).all() and (a == 1).all() and (b == 1).all()


def _have_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


def test_what_is_allowed_reaches_the_device_layer(lib):
    """in place on the same column, two interleaved columns of one section, disjoint buffers: past the host checks; without a device
    every entry then says so, with one the host forms compute"""
    n, w = 6, 3
    num, den = columns(n, 5, zeros=(2,))
    sec = ref.mont_words(ref.rand_elems(n * w, 9)).reshape(n, w, 4)
    sec[:, 0] = ref.mont_words(num)
    sec[:, 1] = ref.mont_words(den)
    flat = sec.reshape(-1)
    out = np.zeros((n, 4), np.uint64)
    e = ref.mont_words([num[0]])
    want_rc = 0 if _have_gpu() else ENODEV
    for sfx in ("",) if _have_gpu() else ("", "_dev"):
        before = flat.copy()
        assert _gprod(lib, "pil2gl_bn128_gprod" + sfx, _p(flat), w, _p(flat, 32), w, n, _p(out), 1) == want_rc
        if want_rc == 0:
            assert np.array_equal(out, ref.mont_words(ref.gprod(num, den)))
        assert _gsum(lib, "pil2gl_bn128_gsum" + sfx, _p(e), _p(flat, 32), w, n, _p(out), 1) == want_rc
        if want_rc == 0:
            assert np.array_equal(out, ref.mont_words(ref.gsum(num[0], den)))
        # column 1 inverted into column 2 of the same section (interleaved), then in place
        assert _inv(lib, "pil2gl_bn128_batch_inverse" + sfx, _p(flat, 32), w, n, _p(flat, 64), w) == want_rc
        assert _inv(lib, "pil2gl_bn128_batch_inverse" + sfx, _p(flat, 32), w, n, _p(flat, 32), w) == want_rc
        if want_rc == 0:
            inv = ref.mont_words(ref.batch_inverse(den))
            assert np.array_equal(sec[:, 2], inv) and np.array_equal(sec[:, 1], inv) and np.array_equal(sec[:, 0], ref.mont_words(num))
        else:
            assert np.array_equal(flat, before)


def test_python_wrappers_refuse_mixed_and_short_buffers():
    from pil2gl import bn128, Pil2glError
    a, short = np.ones((8, 4), np.uint64), np.ones((3, 4), np.uint64)
    e = np.ones(4, np.uint64)

    for call in (lambda: bn128.batch_inverse(a, n=8, out=short), lambda: bn128.batch_inverse(short, n=8),
                 lambda: bn128.batch_inverse(a, n=8, stride=2), lambda: bn128.batch_inverse(a, stride=0),
                 lambda: bn128.batch_inverse(a, stride=2, out_stride=2),               # a strided result needs out
                 lambda: bn128.gprod(short, a), lambda: bn128.gprod(a, a, out=short), lambda: bn128.gprod(a, a, n=8, den_stride=2),
                 lambda: bn128.gsum(e, a, out=short), lambda: bn128.gsum(np.ones(8, np.uint64), a), lambda: bn128.gsum(e, a, den_stride=0)):
        with pytest.raises(Pil2glError):
            call()
    torch = pytest.importorskip("torch")
    t = torch.zeros((8, 4), dtype=torch.int64)                    # a tensor is the device kind, wherever it lives: the mix is refused first
    for call in (lambda: bn128.batch_inverse(a, out=t), lambda: bn128.gprod(t, a), lambda: bn128.gprod(a, a, out=t),
                 lambda: bn128.gsum(e, a, out=t), lambda: bn128.gsum(t, a)):
        with pytest.raises(Pil2glError, match="mixing|host"):
            call()


# ---- the planner -------------------------------------------------------------------------------------------------------------------------
def plan(lib, n, op):
    info = (C.c_uint32 * 5)()
    nbytes = C.c_uint64(1)
    rc = lib.pil2gl_debug_bn128_scan_plan(n, op, info, C.byref(nbytes))
    return rc, tuple(info), nbytes.value


def sizes():
    ns = {0, 1, 2, 3, 15, 16, 17, 63, 64, 65, 1000, MAX_N}
    for j in range(1, 29):
        ns |= {(1 << j) - 1, 1 << j, min((1 << j) + 1, MAX_N)}
    return sorted(ns)


def test_plan_tiles_the_rows_and_bounds_its_scratch(lib):
    last = 0
    for n in sizes():
        for op in OPS.values():
            rc, (L, S, levels, threads, per_wg), nbytes = plan(lib, n, op)
            assert rc == 0, (n, op)
            assert L >= 1 and S >= 1 and L * S >= n and (S - 1) * L < max(n, 1), (n, op)
            assert S <= LANES and threads == 256 and per_wg == 256
            assert (S == 1) == (levels == 1) == (n <= TOP_MAX), (n, op)
            assert nbytes <= UPPER_BOUND + (32 * n if op == 3 else 0), (n, op)
            assert nbytes % 32 == 0 and (nbytes >= 32 * n if op == 3 else True)
            if n == 0:
                assert nbytes == 0
            if op != 3:
                assert plan(lib, n, 0)[1:] == plan(lib, n, op)[1:]      # one geometry for the three operators
        levels = plan(lib, n, 1)[1][2]
        assert levels >= last, n                                      # monotone in n
        last = levels


def test_plan_refusals(lib):
    assert plan(lib, MAX_N + 1, 0)[0] == EINVAL and b"2^28" in lib.pil2gl_last_error()
    assert plan(lib, 4, 4)[0] == EINVAL
    assert lib.pil2gl_debug_bn128_scan_plan(4, 0, None, None) == EINVAL


def test_every_level_count_is_first_met_by_a_small_shape(lib):
    """what keeps the GPU tests honest: every level count the plan yields up to 2^28 rows is met by some n <= 2^20, and the smallest n
    of each is the one the header names"""
    everywhere = {plan(lib, n, 1)[1][2] for n in sizes()}
    assert everywhere == set(FIRST_N_OF_LEVELS)
    for levels, n in FIRST_N_OF_LEVELS.items():
        assert n <= 1 << 20 and plan(lib, n, 1)[1][2] == levels
        if n > 1:
            assert plan(lib, n - 1, 1)[1][2] == levels - 1


# ---- the planner header under the sanitizers, in a program of its own ------------------------------------------------------------------
def test_planner_header_under_the_sanitizers(tmp_path, lib):
    exe = str(tmp_path / "bn_scan_dump")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                           os.path.join(ROOT, "tests", "bn_scan_dump.cpp"), "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", "sanitizer report or a broken invariant:\n" + run.stderr[-4000:]
    lines = run.stdout.splitlines()
    plans = [l for l in lines if not l.startswith("re")]
    assert len(plans) == (1 << 14) + 28 * 3 * 2 - 2                  # 2^28 + 1 is not walked
    seen = 0
    for line in plans:
        n, in_place, levels, L, S, nbytes = (int(v) for v in line.split(" | ")[0].split())
        if n in (1, 64, 65, 1024, 1025, 16385, 262145, MAX_N):
            assert plan(lib, n, 3 if in_place else 0) == (0, (L, S, levels, 256, 256), nbytes), line
            seen += 1
    assert seen >= 12
    verdicts = dict(l.split()[1:] for l in lines if l.startswith("relation"))
    assert verdicts == {"same": "1", "same-pointer-other-stride": "2", "interleaved": "0", "interleaved-later-row": "0", "shifted-rows": "2",
                        "misaligned": "2", "apart": "0", "touching": "2", "other-strides": "2", "empty": "0"}
    assert [l for l in lines if l.startswith("refusals")] == ["refusals 1 1 1 1 1"]


# ---- the staging decision of the host-pointer entries (bn_column.h) under the sanitizers, in a program of its own -------------------------
# n = 100 rows unless the case says otherwise; a range is "+<bytes from the section's start> words up down", a column "<range> +<word>"
STAGING = """\
stage apart words=800 | range +0 words=400 up=1 down=0 range +65536 words=400 up=0 down=1 | col 0 +0 col 1 +0
stage apart-strided-output words=2384 | range +0 words=1192 up=1 down=0 range +65536 words=1192 up=1 down=1 | col 0 +0 col 1 +0
stage same-stride-1 words=400 | range +0 words=400 up=1 down=1 | col 0 +0 col 0 +0
stage same-stride-3 words=1192 | range +0 words=1192 up=1 down=1 | col 0 +0 col 0 +0
stage outputs-at-0-and-1 words=1596 | range +65536 words=400 up=1 down=0 range +0 words=1196 up=1 down=1 | col 0 +0 col 1 +0 col 1 +4
stage outputs-at-2-and-0 words=1600 | range +65536 words=400 up=1 down=0 range +0 words=1200 up=1 down=1 | col 0 +0 col 1 +8 col 1 +0
stage output-among-inputs words=1196 | range +0 words=1196 up=1 down=1 | col 0 +0 col 0 +4
stage three-of-one-section words=780 | range +0 words=780 up=1 down=1 | col 0 +4 col 0 +8 col 0 +0
stage touching words=1592 | range +0 words=1192 up=1 down=0 range +9536 words=400 up=0 down=1 | col 0 +0 col 1 +0
stage empty-beside words=400 | range +0 words=400 up=0 down=1 | col - +0 col 0 +0
stage one-row words=8 | range +0 words=4 up=1 down=0 range +32 words=4 up=1 down=1 | col 0 +0 col 1 +0
stage one-row-in-place words=4 | range +0 words=4 up=1 down=1 | col 0 +0 col 0 +0
stage counts-acc-first words=1192 | range +0 words=1192 up=1 down=1 | col 0 +0 col 0 +4
stage counts-src-first words=1196 | range +0 words=1196 up=1 down=1 | col 0 +4 col 0 +0
stage inputs-of-one-section words=2784 | range +0 words=1192 up=1 down=0 range +32 words=1192 up=1 down=0 range +65536 words=400 up=0 down=1 | col 0 +0 col 1 +0 col 2 +0
"""


def test_staging_decision_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "bn_column_dump")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                           os.path.join(ROOT, "tests", "bn_column_dump.cpp"), "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", "sanitizer report or a broken invariant:\n" + run.stderr[-4000:]
    assert run.stdout == STAGING
