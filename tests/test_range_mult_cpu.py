"""The range-check multiplicities without a device: the checker (tests/range_mult_ref.py) on hand-computed cases, the planner through the
ABI and, in a program of its own, under the sanitizers (tests/range_mult_plan_dump.cpp) together with the aliasing rule of m as this unit
calls it, the refusals of the compute entries before any device call, ENODEV otherwise, and the exported surface."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

import range_mult_ref as rref
from conn_pols_ref import P, R, MONT
from conftest import ROOT

import pil2gl  # noqa: E402  (a plain import: without the feature, or with a broken build, this file fails)
from pil2gl import _lib, pilcheck  # noqa: E402

EINVAL, ENODEV = -1, -2
NONE = rref.NONE
CLEAN = (0, NONE, NONE, 0)
NAMES = ("pil2gl_range_mult_plan", "pil2gl_range_mult_dev", "pil2gl_bn128_range_mult_dev", "pil2gl_range_mult", "pil2gl_bn128_range_mult",
         "pil2gl_debug_range_mult_plan", "pil2gl_debug_range_mult_dev")
CSRC = os.path.join(ROOT, "pil2-stark-js_amd", "csrc")
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _have_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


def threshold():
    """the largest size that takes the LDS path, from the planner alone (the path is monotone in size)"""
    lo, hi = 0, 1 << 28                               # path(lo) == 0 or lo == 0; path(hi) == 1
    assert pilcheck.range_mult_plan(1 << 28, hi)["path"] == 1
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if pilcheck.range_mult_plan(1 << 28, mid)["path"] == 0 else (lo, mid)
    return lo


def test_entries_are_declared_bound_and_exported(lib):
    text = open(os.path.join(ROOT, "include", "pil2gl.h")).read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, header), n + " is not declared in pil2gl.h"
        assert n in _lib.SIGNATURES, n + " is not bound in _lib.py"
        assert getattr(lib, n)
    # the prototypes against the header: as many arguments, and lo signed
    for n in NAMES:
        decl = re.search(r"\bint %s\s*\(([^;]*)\);" % n, header).group(1)
        args = [a.strip() for a in decl.split(",")]
        res, argtypes = _lib.SIGNATURES[n]
        assert len(args) == len(argtypes) and res is C.c_int, n
        for a, ty in zip(args, argtypes):
            if a.startswith("int64_t"):
                assert ty is C.c_int64, (n, a)
            elif a.startswith("uint32_t") and "*" not in a:
                assert ty is C.c_uint32, (n, a)
            elif a.startswith("uint64_t") and "*" not in a:
                assert ty is C.c_uint64, (n, a)
            else:
                assert "*" in a and ty not in (C.c_int64, C.c_uint32, C.c_uint64), (n, a)
    assert "range_mult and bn128_range_mult" in text.split("#pragma once")[0], "listed among the blocking calls"
    assert "One range a call".upper() in text.upper()
    for f in ("range_mult_plan", "range_mult", "range_mult_dev"):
        assert callable(getattr(pilcheck, f))
    addon = open(os.path.join(ROOT, "pil2-stark-js_amd", "addon", "pil2gl_napi.cc")).read()
    for n in ("rangeMultPlan", "rangeMultDev", "rangeMult"):
        assert '"%s"' % n in addon, n + " is not exported by the addon"
    js = open(os.path.join(ROOT, "pil2-stark-js_amd", "js", "pil_checks.js")).read()
    assert re.search(r"module\.exports = \{[^}]*rangeMultiplicities, rangeMultiplicitiesDev, rangeMultPlan", js)


# ---- the checker against hand-computed cases ----
def test_checker_on_hand_computed_cases():
    f = [3, 4, 4, 7, 5, 6]
    assert rref.multiplicities([f], 3, 4, 6, P) == ([1, 2, 1, 1, 0, 0], (1, 0, 3, 5)), "7 = lo + size is out; counts at rows 0..3"
    assert rref.multiplicities([f], 3, 4, 6, P, row0=2) == ([0, 0, 1, 2, 1, 1], (1, 0, 3, 5)), "the table at rows 2..5"
    assert rref.multiplicities([f, f], 3, 5, 6, P, sel_fs=[None, [0, 1, P, 1, 1, 0]]) == ([1, 3, 2, 1, 2, 0], (0, NONE, NONE, 9)), "0 and p unselect"
    assert rref.multiplicities([[2, 3, 3, 3]], 3, 4, 4, P)[1] == (1, 0, 0, 3), "lo - 1"
    assert rref.multiplicities([[3, 3 + (1 << 32), 3, 3]], 3, 4, 4, P)[1] == (1, 0, 1, 3), "lo + 2^32: the difference is not truncated"
    # negative lo: p - 2, p - 1, 0, 1 are -2 .. 1
    assert rref.multiplicities([[P - 2, 1, 0, P - 1, P - 3]], -2, 4, 5, P) == ([1, 1, 1, 1, 0], (1, 0, 4, 4))
    assert rref.multiplicities([[P - 1]], 0, 1, 1, P)[1] == (1, 0, 0, 0) and rref.multiplicities([[P + 5, (1 << 64) - 1]], 5, 2, 2, P)[0] == [1, 0]
    assert rref.multiplicities([[(1 << 64) - 1]], (1 << 32) - 2, 1, 1, P) == ([1], (0, NONE, NONE, 1)), "2^64 - 1 = 2^32 - 2 mod p"
    # Fr: patterns are Montgomery words; the value decides
    mont = lambda v: v % R * MONT % R                                            # noqa: E731
    assert rref.value(mont(77), R) == 77 and rref.value(mont(77) + 3 * R, R) == 77
    assert rref.multiplicities([[mont(-2), mont(1), mont(2), mont(1) + R]], -2, 4, 4, R) == ([1, 0, 0, 2], (1, 0, 2, 3))
    assert rref.multiplicities([[5]], 5, 1, 1, R)[1] == (1, 0, 0, 0), "the pattern 5 is not the value 5 over Fr"
    assert rref.table_column(-1, 3, 5, P) == [P - 1, 0, 1, 1, 1] and rref.table_column(2, 2, 3, R) == [mont(2), mont(3), mont(3)]
    assert rref.element(5, P) == 5 and rref.element(5, R) == 5 * MONT % R and rref.element(0, R) == 0


# ---- the planner ----
def expected_plan(n, size, n_f, T, path=None):
    lds = size <= T if path is None else path == 0
    blocks = min(max(-(-n // 1024), 1), 512) if lds else min(max(-(-n // 256), 1), 2048)
    return {"path": 0 if lds else 1, "threads": 1024 if lds else 256, "blocks": blocks, "launches": 2 + n_f, "headerBytes": 64,
            "ldsCounters": size if lds else 0, "scratchBytes": (64 + 4 * size + 15) // 16 * 16 if n else 0}


def test_plan_values_across_the_threshold_and_size_one():
    T = threshold()
    assert 0 <= T <= 8192
    sizes = sorted({1, 2, 3, 256, max(T - 1, 1), max(T, 1), T + 1, 1 << 14, 1 << 28})
    for size in sizes:
        for n in (size, 1 << 28):
            for field in ("gl", "bn128"):
                for n_f in (1, 8):
                    assert pilcheck.range_mult_plan(n, size, n_f, field) == expected_plan(n, size, n_f, T), (n, size, field, n_f)
    assert pilcheck.range_mult_plan(5, 1)["scratchBytes"] == 80 and pilcheck.range_mult_plan(5, 5)["scratchBytes"] == 96
    assert pilcheck.range_mult_plan(0, 7, 3) == dict(expected_plan(0, 7, 3, T), scratchBytes=0)
    # the path forced, as the tests and the benchmark do
    for path in (0, 1):
        assert pilcheck.range_mult_plan(1 << 20, 300, 2, "gl", path) == expected_plan(1 << 20, 300, 2, T, path)
    assert pilcheck.range_mult_plan(1 << 20, 8192, 1, "bn128", 0)["ldsCounters"] == 8192
    assert pilcheck.range_mult_plan(1 << 20, 300, 1, "gl", 2) == pilcheck.range_mult_plan(1 << 20, 300)


def test_plan_refusals(lib):
    info = (C.c_uint32 * 6)()
    b = C.c_uint64(7)
    for n, size, n_f, words, msg in (((1 << 28) + 1, 3, 1, 1, b"n must"), (8, 0, 1, 1, b"size"), (1 << 28, (1 << 28) + 1, 1, 4, b"size"), (8, 9, 1, 1, b"size > n"),
                                     (8, 3, 0, 1, b"1 .. 8"), (8, 3, 9, 4, b"1 .. 8"), (8, 3, 1, 2, b"elemWords"), (1 << 63, 3, 1, 1, b"n must")):
        assert lib.pil2gl_range_mult_plan(n, size, n_f, words, info, C.byref(b)) == EINVAL and b.value == 0, (n, size, n_f, words)
        assert msg in lib.pil2gl_last_error(), lib.pil2gl_last_error()
    assert lib.pil2gl_range_mult_plan(64, 3, 2, 1, None, None) == 0
    assert lib.pil2gl_debug_range_mult_plan(1 << 20, 8193, 1, 1, 0, info, C.byref(b)) == EINVAL and b"8192" in lib.pil2gl_last_error()
    assert lib.pil2gl_debug_range_mult_plan(1 << 20, 8193, 1, 1, 3, info, C.byref(b)) == EINVAL and b"path" in lib.pil2gl_last_error()
    with pytest.raises(pil2gl.Pil2glError, match="-1"):
        pilcheck.range_mult_plan(8, 3, 9)


def test_planner_and_aliasing_rule_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "range_mult_plan_dump")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                           os.path.join(ROOT, "tests", "range_mult_plan_dump.cpp"), "-o", exe])
    T = threshold()
    big = 1 << 30                                     # 2^28 rows of 2^30 elements: n stride = 2^58, the largest that passes
    B = 1 << 40                                       # a byte address; never dereferenced
    plans = [(n, size, n_f, w, 2) for size in (1, 2, max(T, 1), T + 1, 1 << 28) for n in (size, 1 << 28) for n_f, w in ((1, 1), (8, 4))]
    plans += [(1 << 20, 300, 2, 1, 0), (1 << 20, 300, 2, 1, 1), (0, 9, 1, 1, 2)]
    refused = [((1 << 28) + 1, 3, 1, 1, 2), (8, 0, 1, 1, 2), (8, 9, 1, 1, 2), (8, 3, 0, 1, 2), (8, 3, 9, 1, 2), (8, 3, 1, 3, 2), ((1 << 64) - 1, (1 << 64) - 1, 8, 4, 2),
               (1 << 20, 8193, 1, 1, 0), (8, 3, 1, 1, 3)]
    rows = [((8, 3, 5), 1), ((8, 3, 6), 0), ((8, 8, 0), 1), ((8, 1, 7), 1), ((8, 1, 8), 0), ((1 << 28, 1 << 28, 0), 1), ((1 << 28, 1, (1 << 28) - 1), 1),
            ((8, 3, (1 << 64) - 2), 0), ((8, (1 << 64) - 1, 2), 0), ((1 << 28, 1 << 27, 1 << 27), 1), ((1 << 28, (1 << 27) + 1, 1 << 27), 0)]
    los = [0, 1, -1, -128, I64_MIN, I64_MIN + 1, I64_MAX, I64_MAX - (1 << 28) + 1, I64_MAX - 1 + 1, -(0x43e1f593f0000001), -(0x43e1f593f0000002), -(1 << 32)]
    alias = [  # (n, words, mBase, mStride, mCol, rBase, rStride, cols) -> (ok, columns)
        ((8, 1, B, 4, 3, B, 4, [0]), (1, 1)), ((8, 1, B, 4, 0, B, 4, [0]), (0, 1)), ((8, 4, B, 4, 1, B, 4, [3]), (1, 1)),
        ((8, 1, B, 4, 3, B, 5, [0]), (0, 1)), ((8, 1, B + 8, 4, 1, B, 4, [0]), (0, 1)),
        ((8, 1, B + 8 * 29, 4, 0, B, 4, [0]), (1, 1)), ((8, 1, B + 8 * 28, 4, 0, B, 4, [0]), (0, 1)),
        ((1, 1, B, 1, 0, B + 8, 1, [0]), (1, 1)), ((1, 1, B, 1, 0, B, 1, [0]), (0, 1)),                  # the narrowest stride
        ((8, 1, B, 4, 4, B, 4, [0]), (0, 0)), ((8, 1, B, 1 << 32, 0, B, 4, [0]), (0, 0)),              # a column and a stride that do not pass
        ((8, 1, B, (1 << 32) - 1, (1 << 32) - 2, B, (1 << 32) - 1, [(1 << 32) - 3]), (1, 1)),            # the widest stride
        ((1 << 28, 4, B, big, big - 1, B, big, [big - 2]), (1, 1)),                                     # the 2^58 limit: spans of 2^63 bytes, no overflow
        ((1 << 28, 4, B, big, big - 1, B, big, [big - 1]), (0, 1)),
        ((1 << 28, 4, B, big, 0, B + (1 << 62), big, [0]), (0, 1)),
        ((1 << 28, 1, B, big + 1, 0, B, big, [0]), (0, 0)),                                             # n stride above 2^58
    ]
    with open(tmp_path / "cmds.txt", "w") as f:
        f.write("".join("plan %d %d %d %d %d\n" % r for r in plans + refused))
        f.write("".join("rows %d %d %d\n" % r for r, _ in rows))
        f.write("".join("lo %d\n" % v for v in los))
        f.write("".join("alias %d %d %d %d %d %d %d %d %s\n" % (a[:7] + (len(a[7]), " ".join(map(str, a[7])))) for a, _ in alias))
    run = subprocess.run([exe, str(tmp_path / "cmds.txt")], capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", "sanitizer report:\n" + run.stderr[-4000:]
    out = [json.loads(line) for line in run.stdout.splitlines()]
    assert len(out) == len(plans) + len(refused) + len(rows) + len(los) + len(alias)
    for (n, size, n_f, w, path), got in zip(plans, out):
        want = expected_plan(n, size, n_f, T, None if path == 2 else path)
        assert got["ok"] == 1 and (got["offHeader"], got["offCounters"]) == (0, 64) and got["bytes"] == want["scratchBytes"], (n, size, got)
        assert {k: got[k] for k in ("path", "threads", "blocks", "launches", "ldsCounters")} == {k: want[k] for k in ("path", "threads", "blocks", "launches", "ldsCounters")}
        assert got["bytes"] % 16 == 0 and (n == 0 or got["bytes"] >= 64 + 4 * size)
    at = len(plans)
    assert all(g["ok"] == 0 and g["why"] for g in out[at:at + len(refused)])
    at += len(refused)
    assert [g["ok"] for g in out[at:at + len(rows)]] == [w for _, w in rows]
    at += len(rows)
    for v, got in zip(los, out[at:at + len(los)]):
        assert got["p"] == v % P and sum(x << (64 * i) for i, x in enumerate(got["r"])) == v % R, v
    at += len(los)
    assert [(g["ok"], g["columns"]) for g in out[at:]] == [w for _, w in alias]


# ---- the compute entries ----
def test_compute_entries_refuse_before_any_device_call(lib):
    buf = np.zeros(16384, np.uint64)
    base = buf.ctypes.data + (-buf.ctypes.data % 16)
    col0 = np.array([0], np.uint64)
    col2 = np.array([2], np.uint64)
    bad_col = np.array([5], np.uint64)
    rep = (C.c_uint64 * 4)()
    n, stride, n_f, size, row0 = 8, 5, 2, 3, 5
    for dev, host, field, words in ((lib.pil2gl_range_mult_dev, lib.pil2gl_range_mult, "gl", 1),
                                    (lib.pil2gl_bn128_range_mult_dev, lib.pil2gl_bn128_range_mult, "bn128", 4)):
        need = pilcheck.range_mult_plan(n, size, n_f, field)["scratchBytes"]
        span = n * stride * 8 * words
        f0, f1, sel, m, work = (base + i * span for i in range(5))
        assert work + need <= buf.ctypes.data + buf.nbytes

        def call(fn=dev, dev_form=True, **kw):
            """the good call with named changes: f0_*, f1_* fields of a side; lo, size, row0, m, m_stride, m_col, n, n_f, work, need, rep, F"""
            side = {"f0": dict(base=f0, stride=stride, hostCols=col0.ctypes.data, sel=None, selStride=0, selCol=0),
                    "f1": dict(base=f1, stride=stride, hostCols=col2.ctypes.data, sel=sel, selStride=stride, selCol=3)}
            top = dict(lo=-1, size=size, row0=row0, m=m, m_stride=stride, m_col=4, n=n, n_f=n_f, work=work, need=need, rep=rep, F=0)
            for key, v in kw.items():
                if key in top:
                    top[key] = v
                else:
                    s, field_name = key.split("_", 1)
                    side[s][field_name] = v
            F = (_lib.TupleSide * 2)(_lib.TupleSide(**side["f0"]), _lib.TupleSide(**side["f1"]))
            for i in range(4):
                rep[i] = 5
            args = [None if top["F"] is None else F, top["n_f"], top["lo"], top["size"], top["row0"], top["m"], top["m_stride"], top["m_col"], top["n"]]
            return fn(*(args + ([top["work"], top["need"], top["rep"], None] if dev_form else [top["rep"]])))
        err = lib.pil2gl_last_error
        assert call(n=(1 << 28) + 1) == EINVAL and b"2^28" in err()
        assert tuple(rep) == CLEAN, "a refused call leaves a clean report"
        assert call(size=0) == EINVAL and call(size=(1 << 28) + 1) == EINVAL and b"size" in err()
        assert call(size=9, row0=0) == EINVAL and b"size > n" in err()
        assert call(n_f=0) == EINVAL and call(n_f=9) == EINVAL and call(n_f=1 << 40) == EINVAL and b"1 .. 8" in err()
        assert call(row0=6) == EINVAL and b"row0 + size > n" in err() and tuple(rep) == CLEAN
        assert call(row0=(1 << 64) - 1) == EINVAL and call(row0=9, size=1) == EINVAL and b"row0 + size > n" in err()
        assert call(f0_hostCols=bad_col.ctypes.data) == EINVAL and b"f 0: a column >= stride" in err()
        assert call(f1_hostCols=bad_col.ctypes.data) == EINVAL and b"f 1: a column >= stride" in err()
        assert call(f0_stride=0) == EINVAL and call(f1_stride=1 << 32) == EINVAL and b"stride" in err()
        assert call(f0_stride=1 << 31, n=1 << 28) == EINVAL and b"2^58" in err()
        assert call(f1_selCol=stride) == EINVAL and b"selF 1" in err()
        assert call(m_col=5) == EINVAL and call(m_stride=1 << 32) == EINVAL and b"m: " in err()
        for key in ("f0_base", "f1_base", "f1_hostCols", "m", "work", "rep", "F"):
            assert call(**{key: None}) == EINVAL, key
        for key, v in (("f0_base", f0), ("f1_base", f1), ("f1_sel", sel), ("m", m), ("work", work)):
            assert call(**{key: v + 8}) == EINVAL and b"aligned" in err(), key
        assert call(need=need - 16) == EINVAL and b"scratch" in err()
        assert call(work=f0 + 16) == EINVAL and b"overlaps" in err()                             # the scratch inside f0
        assert call(work=sel - 16) == EINVAL and b"overlaps" in err()                            # ... reaching the selector's first element
        assert call(work=m + 16) == EINVAL and b"the scratch overlaps" in err()                   # ... and m's matrix
        # the aliasing rule, in both directions
        assert call(m=f0, m_col=0) == EINVAL and b"m overlaps" in err() and call(m=f1, m_col=2) == EINVAL and b"m overlaps" in err(), "the columns read"
        for where in (f0, f1):
            assert call(m=where + 16 * words, m_col=1) == EINVAL and b"m overlaps" in err(), "a foreign base"
            assert call(m=where, m_stride=stride + 1) == EINVAL and b"m overlaps" in err(), "another stride"
        assert call(m=sel, m_col=3) == EINVAL and b"m overlaps" in err(), "the selector's column is read too"
        assert tuple(rep) == CLEAN
        assert call(n=0) == 0 and tuple(rep) == CLEAN, "n = 0: clean, no device"
        assert call(n=0, f0_base=None, f1_base=None, m=None, work=None, row0=0) == 0
        hcall = lambda **kw: call(fn=host, dev_form=False, **kw)                 # noqa: E731
        assert hcall(n=(1 << 28) + 1) == EINVAL and hcall(size=0) == EINVAL and hcall(n_f=9) == EINVAL and hcall(row0=6) == EINVAL
        assert hcall(f0_hostCols=bad_col.ctypes.data) == EINVAL and hcall(m_col=stride) == EINVAL and hcall(f1_selCol=9) == EINVAL
        assert hcall(m=f0, m_col=0) == EINVAL and b"m overlaps" in err() and hcall(m=f1 + 8, m_col=4) == EINVAL and b"m overlaps" in err()
        for key in ("f0_base", "f1_base", "f0_hostCols", "m", "rep", "F"):
            assert hcall(**{key: None}) == EINVAL, key
        assert hcall(n=0) == 0 and tuple(rep) == CLEAN
        # the debug form refuses alike, and a path it cannot take
        dbg = lambda path, **kw: call(fn=lambda *a: lib.pil2gl_debug_range_mult_dev(*(a + (words, path))), **kw)      # noqa: E731
        assert dbg(4) == EINVAL and b"path" in err() and dbg(0, n=0) == 0 and dbg(1, row0=6) == EINVAL
        if not _have_gpu():
            assert call() == ENODEV and call(lo=I64_MIN) == ENODEV and call(lo=I64_MAX - size + 1) == ENODEV and call(row0=0) == ENODEV
            assert call(m=f0, m_col=3) == ENODEV and call(m=f1, m_col=0) == ENODEV, "a spare column of an f: nothing to refuse"
            assert call(f1_base=f0, m=f0, m_col=4) == ENODEV, "one matrix on both sides and m beside them"
            assert call(m=sel, m_col=2) == ENODEV, "a spare column of the selector's matrix"
            assert hcall() == ENODEV and hcall(m=f0, m_col=3) == ENODEV and hcall(m=m + 8) == ENODEV, "the host forms need no alignment"
            assert dbg(0) == ENODEV and dbg(1) == ENODEV
    a = np.zeros((8, 4), np.uint64)
    if not _have_gpu():
        with pytest.raises(pil2gl.Pil2glError, match="-2"):
            pilcheck.range_mult([(a, [0])], -3, 8, (a, 3), 8)
        fr = np.zeros((8, 4, 4), np.uint64)
        with pytest.raises(pil2gl.Pil2glError, match="-2"):
            pilcheck.range_mult([(fr, [0]), (fr, [1], (fr, 2))], 0, 2, (fr, 3), 8, field="bn128", row0=6)
    with pytest.raises(pil2gl.Pil2glError, match="m overlaps"):
        pilcheck.range_mult([(a, [2])], 0, 4, (a, 2), 8)
    with pytest.raises(pil2gl.Pil2glError, match="need more"):
        pilcheck.range_mult([(a, [0])], 0, 4, (a, 3), 9)
    with pytest.raises(pil2gl.Pil2glError, match="one column"):
        pilcheck.range_mult([(a, [0, 1])], 0, 4, (a, 3), 8)
    with pytest.raises(pil2gl.Pil2glError, match="in place"):
        pilcheck.range_mult([(a, [0])], 0, 4, (a.astype(np.int64), 3), 8)
    assert pilcheck.range_mult([(a, [0])], 0, 4, (a, 3), 0) == CLEAN
