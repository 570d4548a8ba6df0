"""The connection polynomials without a device: the planner's refusals and its working-buffer formula, the ABI surface (declared, bound,
exported; every refusal before any device call, ENODEV otherwise), and the checker (tests/conn_pols_ref.py, sequential swaps) against the
reference-written fixture tests/golden/conn_pols.json (tools/gen_conn_golden.js)."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import conn_pols_ref as ref
from conn_pols_ref import P, R
from conftest import ROOT

import pil2gl  # noqa: E402  (a plain import: without the feature, or with a broken build, this file fails)
from pil2gl import _lib, wtns  # noqa: E402

EINVAL, ENODEV = -1, -2
NAMES = ("pil2gl_conn_plan", "pil2gl_conn_pols_dev", "pil2gl_bn128_conn_pols_dev", "pil2gl_conn_pols", "pil2gl_bn128_conn_pols")
GOLDEN = os.path.join(ROOT, "tests", "golden", "conn_pols.json")


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _have_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


def test_entries_are_declared_bound_and_exported(lib):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pil2gl.h")).read(), flags=re.S)
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, header), n + " is not declared in pil2gl.h"
        assert n in _lib.SIGNATURES, n + " is not bound in _lib.py"
        assert getattr(lib, n)
    for f in ("conn_plan", "conn_pols", "conn_pols_dev"):
        assert callable(getattr(wtns, f))


def r16(x):
    return (x + 15) & ~15


def scratch_formula(n_rows, n_cols, N, words, info):
    """include/pil2gl.h: 16 + 8 elemWords T + 4 r16(4 cells) + 1024 [3] + r16(4 [4])"""
    cells = n_rows * n_cols
    t = n_cols * (1 << info["loBits"]) + (1 << info["hiBits"])
    return 16 + 8 * words * t + 4 * r16(4 * cells) + 1024 * info["sortBlocks"] + r16(4 * info["scanChunks"])


def test_plan_passes_geometry_and_scratch_bound():
    for n_rows, n_cols, n_w, N, field in ((1, 1, 2, 1, "gl"), (63, 3, 200, 64, "gl"), (65, 12, 257, 128, "bn128"), (6000, 12, 70000, 8192, "gl"),
                                          (4096, 1, 1 << 16, 4096, "gl"), (4097, 1, (1 << 16) + 1, 8192, "bn128"), (1 << 24, 18, 5000000, 1 << 24, "bn128"),
                                          (1 << 24, 12, 1 << 24, 1 << 25, "gl"), ((1 << 32) // 64 - 1, 64, (1 << 32) - 1, 1 << 32, "gl")):
        words = 1 if field == "gl" else 4
        info = wtns.conn_plan(n_rows, n_cols, n_w, N, field)
        cells = n_rows * n_cols
        assert info["passes"] == -(-(n_w - 1).bit_length() // 8), (n_w, info)
        assert (info["threads"], info["tile"]) == (256, 4096)
        assert info["sortBlocks"] == -(-cells // 4096) and info["scanChunks"] == -(-256 * info["sortBlocks"] // 4096)
        n_bits = N.bit_length() - 1
        assert info["loBits"] + info["hiBits"] == n_bits and info["loBits"] == (n_bits + 1) // 2
        assert info["launches"] == 4 + 5 * info["passes"]
        assert info["scratchBytes"] == scratch_formula(n_rows, n_cols, N, words, info) and info["scratchBytes"] % 16 == 0
        t = n_cols * (1 << info["loBits"]) + (1 << info["hiBits"])
        assert info["scratchBytes"] < 16 * cells + cells // 4 + cells // 16384 + 8 * words * t + 2048
    assert wtns.conn_plan(1 << 24, 12, 1 << 24, 1 << 24)["passes"] == 3          # 24 bits of signal: three passes, not four
    assert wtns.conn_plan(10, 3, 1, 16)["passes"] == 0 and wtns.conn_plan(10, 3, 2, 16)["passes"] == 1
    empty = wtns.conn_plan(0, 5, 9, 8)
    assert empty["passes"] == 0 and empty["sortBlocks"] == 0 and empty["launches"] == 2
    assert wtns.conn_plan(0, 0, 9, 8)["scratchBytes"] == 0


def test_plan_refusals(lib):
    info = (C.c_uint32 * 8)()
    b = C.c_uint64(7)
    bad = [((1 << 32) // 4, 4, 9, 1 << 30, 1, b"2^32"),                       # nRows nCols = 2^32
           (5, 3, 1 << 32, 8, 1, b"nW"),
           (9, 3, 9, 8, 1, b"nRows"),                                           # nRows > N
           (5, 3, 9, 12, 1, b"power of two"), (0, 3, 9, 0, 1, b"power of two"), (5, 3, 9, 1 << 33, 1, b"power of two"),
           (5, 65, 9, 8, 1, b"columns"), (5, 3, 9, 8, 2, b"elemWords")]
    for n_rows, n_cols, n_w, N, words, msg in bad:
        assert lib.pil2gl_conn_plan(n_rows, n_cols, n_w, N, words, info, C.byref(b)) == EINVAL and b.value == 0, (n_rows, n_cols, n_w, N)
        assert msg in lib.pil2gl_last_error(), lib.pil2gl_last_error()
    assert lib.pil2gl_conn_plan((1 << 32) // 4 - 1, 4, (1 << 32) - 1, 1 << 30, 4, info, C.byref(b)) == 0 and info[0] == 4
    assert lib.pil2gl_conn_plan(5, 3, 9, 8, 1, None, None) == 0
    with pytest.raises(pil2gl.Pil2glError, match="-1"):
        wtns.conn_plan(9, 3, 9, 8)


def test_compute_entries_refuse_before_any_device_call(lib):
    buf = np.zeros(4096, np.uint64)
    a = buf.ctypes.data
    w = np.array([3, 0, 0, 0], np.uint64)
    ks = np.arange(1, 13, dtype=np.uint64)
    pw, pk = w.ctypes.data, ks.ctypes.data
    need = wtns.conn_plan(4, 3, 9, 8)["scratchBytes"]
    need4 = wtns.conn_plan(4, 3, 9, 8, "bn128")["scratchBytes"]
    s_map, dst, work = a, a + 1024, a + 8192
    bad = C.c_uint64(5)
    for fn, nb in ((lib.pil2gl_conn_pols_dev, need), (lib.pil2gl_bn128_conn_pols_dev, need4)):
        ok = [s_map, 4, 3, 9, 8, pw, pk, dst, 3, 0, work, nb, None, None]

        def call(**kw):
            args = list(ok)
            for k, v in kw.items():
                args[int(k[1:])] = v
            return fn(*args)
        assert call(a8=2) == EINVAL and b"dstStride" in lib.pil2gl_last_error()                 # dstStride < nCols
        assert call(a8=4, a9=2) == EINVAL and b"dstStride" in lib.pil2gl_last_error()           # dstStride < dstOffset + nCols
        assert call(a11=nb - 16) == EINVAL and b"scratch" in lib.pil2gl_last_error()
        assert call(a7=s_map + 32) == EINVAL and b"overlaps" in lib.pil2gl_last_error()         # dst inside sMap
        assert call(a7=work + 64) == EINVAL and b"overlaps" in lib.pil2gl_last_error()          # dst inside the scratch
        assert call(a10=s_map) == EINVAL and b"overlaps" in lib.pil2gl_last_error()             # the scratch over sMap
        assert call(a10=work + 8) == EINVAL and b"aligned" in lib.pil2gl_last_error()
        for k in (0, 5, 6, 7, 10):
            assert call(**{"a%d" % k: None}) == EINVAL, k
        assert call(a1=9) == EINVAL and call(a4=12) == EINVAL and call(a3=1 << 32) == EINVAL     # what the plan refuses
        assert call(a12=C.byref(bad), a8=2) == EINVAL and bad.value == (1 << 64) - 1
        assert call(a2=0, a8=0) == 0                                                             # no columns: nothing to do, no device
        if not _have_gpu():
            assert call() == ENODEV
    # the host forms
    sm64 = np.array([0, 1, 2, 1, 0, 8, 3, 3, 3, 0, 0, 1], np.uint64)
    sm32 = np.zeros((3, 8), np.uint32)
    sm32[:, :4] = sm64.reshape(4, 3).T
    out = np.zeros(8 * 3 * 4, np.uint64)
    p = lambda x: x.ctypes.data                                                                    # noqa: E731
    for fn in (lib.pil2gl_conn_pols, lib.pil2gl_bn128_conn_pols):
        assert fn(p(sm64), 2, 4, 3, 9, 8, pw, pk, p(out)) == EINVAL and b"layout" in lib.pil2gl_last_error()
        assert fn(p(sm64), 0, 4, 3, 8, 8, pw, pk, p(out)) == EINVAL and b"sMap cell 5 (row 1, column 2) = 8" in lib.pil2gl_last_error()
        assert fn(p(sm32), 1, 8, 3, 8, 8, pw, pk, p(out)) == EINVAL and b"sMap cell 5 (row 1, column 2) = 8" in lib.pil2gl_last_error()
        assert fn(None, 0, 4, 3, 9, 8, pw, pk, p(out)) == EINVAL
        assert fn(p(sm64), 0, 4, 3, 9, 8, None, pk, p(out)) == EINVAL
        assert fn(p(sm64), 0, 4, 3, 9, 8, pw, None, p(out)) == EINVAL
        assert fn(p(sm64), 0, 4, 3, 9, 8, pw, pk, None) == EINVAL
        assert fn(p(sm64), 0, 4, 3, 9, 8, pw, pk, p(sm64)) == EINVAL and b"overlaps" in lib.pil2gl_last_error()
        assert fn(p(sm64), 0, 9, 3, 9, 8, pw, pk, p(out)) == EINVAL                              # nRows > N
        assert fn(p(sm64), 0, 4, 0, 9, 8, pw, pk, p(out)) == 0                                   # no columns, no device
        if not _have_gpu():
            assert fn(p(sm64), 0, 4, 3, 9, 8, pw, pk, p(out)) == ENODEV
            assert fn(p(sm32), 1, 8, 3, 9, 8, pw, pk, p(out)) == ENODEV
    if not _have_gpu():
        with pytest.raises(pil2gl.Pil2glError, match="-2"):
            wtns.conn_pols(sm32, 3, 8, [3], [5, 6])
        with pytest.raises(pil2gl.Pil2glError, match="-2"):
            wtns.conn_pols(sm64, 3, 8, *ref.consts(3, [5, 6], R), field="bn128")
    with pytest.raises(pil2gl.Pil2glError, match="nCols - 1"):
        wtns.conn_pols(sm32, 3, 8, [3], [5, 6, 7])


# ---- the checker ----
def test_checker_constants():
    assert pow(ref.GL_W32, 1 << 31, P) == P - 1 and ref.GL_K == pow(7, 1 << 32, P)                # f3g.js:40 (a root of order 2^32), :26
    assert ref.FR_W28 == pow(5, (R - 1) >> 28, R) and pow(ref.FR_W28, 1 << 27, R) == R - 1
    for q in (P, R):
        assert pow(ref.root(q, 5), 32, q) == 1 and pow(ref.root(q, 5), 16, q) == q - 1


def test_checker_reproduces_the_reference_written_golden():
    if not os.path.exists(GOLDEN):
        pytest.skip("tests/golden/conn_pols.json is not shipped: node could not load the reference's polutils.js / f3g.js when the change was made")
    g = json.load(open(GOLDEN))
    assert int(g["k"]) == ref.GL_K and len(g["cases"]) == 2
    for c in g["cases"]:
        n_rows, n_cols, N = c["nRows"], c["nCols"], 1 << c["nBits"]
        ks = [int(x) for x in c["ks"]]
        assert int(c["w"]) == ref.root(P, c["nBits"]) and ks == ref.get_ks(P, n_cols - 1)
        flat = [c["sMap"][j][i] for i in range(n_rows) for j in range(n_cols)]
        S = ref.conn_pols(flat, n_rows, n_cols, N, int(c["w"]), ks, P)
        assert S == [[int(x) for x in col] for col in c["S"]], c["name"]
        assert sorted(v for col in S for v in col) == sorted(pow(int(c["w"]), i, P) * k % P for i in range(N) for k in [1] + ks), "a permutation of the identity"


def test_checker_small_case_by_hand():
    """one signal in cells 0, 2, 3 of a 2 x 2 table: swaps (0, 2) then (0, 3) leave S[0] = id(3), S[2] = id(0), S[3] = id(2)"""
    w, k = 4, 5
    ident = lambda c: pow(w, c // 2, P) * (k if c % 2 else 1) % P                                 # noqa: E731
    S = ref.conn_pols([7, 0, 7, 7], 2, 2, 4, w, [k], P)
    got = {c: S[c % 2][c // 2] for c in range(8)}
    assert got == {0: ident(3), 1: ident(1), 2: ident(0), 3: ident(2), 4: ident(4), 5: ident(5), 6: ident(6), 7: ident(7)}
