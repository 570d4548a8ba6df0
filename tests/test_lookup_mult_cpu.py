"""The lookup multiplicities without a device: the checker (tests/lookup_mult_ref.py) on hand-written cases, the planner through the ABI
and, in a program of its own, under the sanitizers (tests/lookup_mult_plan_dump.cpp) together with the aliasing rule of m, the refusals of
the compute entries before any device call, ENODEV otherwise, and the exported surface."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

import lookup_mult_ref as mref
from conn_pols_ref import P, R, MONT
from conftest import ROOT

import pil2gl  # noqa: E402  (a plain import: without the feature, or with a broken build, this file fails)
from pil2gl import _lib, pilcheck  # noqa: E402

EINVAL, ENODEV = -1, -2
NONE = mref.NONE
CLEAN = (0, NONE, NONE, 0)
NAMES = ("pil2gl_lookup_mult_plan", "pil2gl_lookup_mult_dev", "pil2gl_bn128_lookup_mult_dev", "pil2gl_lookup_mult", "pil2gl_bn128_lookup_mult",
         "pil2gl_debug_lookup_mult_probe")
CSRC = os.path.join(ROOT, "pil2-stark-js_amd", "csrc")


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
    assert "pil2gl_tuple_side" in header and C.sizeof(_lib.TupleSide) == 48
    for f in ("lookup_mult_plan", "lookup_mult", "lookup_mult_dev", "lookup_mult_probe"):
        assert callable(getattr(pilcheck, f))
    assert pilcheck.lookup_mult_probe() >= 0
    addon = open(os.path.join(ROOT, "pil2-stark-js_amd", "addon", "pil2gl_napi.cc")).read()
    for n in ("lookupMultPlan", "lookupMultDev", "lookupMult", "lookupMultProbe"):
        assert '"%s"' % n in addon, n + " is not exported by the addon"
    js = open(os.path.join(ROOT, "pil2-stark-js_amd", "js", "pil_checks.js")).read()
    assert re.search(r"module\.exports = \{[^}]*lookupMultiplicities, lookupMultiplicitiesDev", js)


# ---- the checker against hand-written cases ----
def test_checker_first_selected_occurrence_and_missing_rows():
    t = [(1, 2), (3, 4), (3, 4), (5, 6)]
    f = [(3, 4), (1, 2), (3, 4), (3, 4)]
    assert mref.multiplicities([f], t, P) == ([1, 3, 0, 0], (0, NONE, NONE, 4))
    assert mref.multiplicities([f], t, P, sel_t=[1, 0, 1, 1]) == ([1, 0, 3, 0], (0, NONE, NONE, 4)), "the first SELECTED occurrence"
    assert mref.multiplicities([f, f], t, P, sel_fs=[None, [0, 1, 1, 0]]) == ([2, 4, 0, 0], (0, NONE, NONE, 6))
    # a tuple t holds at an unselected row only is absent; m still counts what matched
    assert mref.multiplicities([f], t, P, sel_t=[0, 1, 1, 1]) == ([0, 3, 0, 0], (1, 0, 1, 3))
    g = [(9, 9), (1, 2), (8, 8), (3, 4)]
    assert mref.multiplicities([f, g, g], t, P, sel_fs=[None, [0, 1, 1, 1], None]) == ([3, 5, 0, 0], (1, 1, 2, 8)), "side before row"
    assert mref.multiplicities([[(1, 2)]], [(2, 1)], P) == ([0], (1, 0, 0, 0)), "(a, b) is not (b, a)"
    assert mref.multiplicities([[(5, 7 + P)]], [(5 + P, 7)], P) == ([1], (0, NONE, NONE, 1)), "x and x + p are one value"
    assert mref.multiplicities([[(3 * R + 11,)]], [(11,)], R) == ([1], (0, NONE, NONE, 1))
    assert mref.multiplicities([[(1,)] * 3], [(1,)] * 3, P, sel_fs=[[0, P, 0]]) == ([0, 0, 0], (0, NONE, NONE, 0)), "0 and p select nothing"
    assert mref.element(5, P) == 5 and mref.element(5, R) == 5 * MONT % R and mref.element(0, R) == 0


# ---- the planner ----
SHAPES = (0, 1, 8, 9, 1 << 20, 1 << 28)


def expected_plan(n, n_f=1):
    cap = 16
    while cap < 2 * n:
        cap *= 2
    return {"capBits": cap.bit_length() - 1, "threads": 256, "blocks": min(max(-(-n // 256), 1), 2048), "launches": 3 + n_f, "headerBytes": 64,
            "slotBytes": 8, "scratchBytes": 64 + 8 * cap if n else 0}


def test_plan_capacity_geometry_and_scratch():
    assert [expected_plan(n)["capBits"] for n in SHAPES] == [4, 4, 4, 5, 21, 29], "n = 8 fills half of 16 slots, n = 9 needs 32"
    for n in SHAPES:
        for field in ("gl", "bn128"):
            for n_f in (1, 2, 8):
                assert pilcheck.lookup_mult_plan(n, 3, n_f, field) == expected_plan(n, n_f), (n, field, n_f)
    assert pilcheck.lookup_mult_plan(1 << 28, 16, 8, "bn128")["scratchBytes"] == 64 + (8 << 29)


def test_plan_refusals(lib):
    info = (C.c_uint32 * 6)()
    b = C.c_uint64(7)
    for n, k, n_f, words, msg in (((1 << 28) + 1, 3, 1, 1, b"2^28"), (8, 0, 1, 1, b"1 .. 16"), (8, 17, 1, 4, b"1 .. 16"), (8, 3, 0, 1, b"1 .. 8"),
                                  (8, 3, 9, 4, b"1 .. 8"), (8, 3, 1, 2, b"elemWords"), (1 << 63, 3, 1, 1, b"2^28")):
        assert lib.pil2gl_lookup_mult_plan(n, k, n_f, words, info, C.byref(b)) == EINVAL and b.value == 0, (n, k, n_f, words)
        assert msg in lib.pil2gl_last_error(), lib.pil2gl_last_error()
    assert lib.pil2gl_lookup_mult_plan(64, 3, 2, 1, None, None) == 0
    with pytest.raises(pil2gl.Pil2glError, match="-1"):
        pilcheck.lookup_mult_plan(8, 3, 9)


def test_planner_and_aliasing_rule_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "lookup_mult_plan_dump")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                           os.path.join(ROOT, "tests", "lookup_mult_plan_dump.cpp"), "-o", exe])
    refused = [((1 << 28) + 1, 3, 1, 1), (8, 0, 1, 1), (8, 17, 1, 1), (8, 3, 0, 1), (8, 3, 9, 1), (8, 3, 1, 3), ((1 << 64) - 1, 3, 8, 4)]
    B = 1 << 40                                       # a byte address; never dereferenced
    big = 1 << 30                                     # 2^28 rows of 2^30 elements: n stride = 2^58, the largest that passes
    alias = [  # (n, words, mBase, mStride, mCol, rBase, rStride, cols) -> (ok, columns)
        ((8, 1, B, 4, 3, B, 4, [0, 2]), (1, 1)),                                 # a spare column of the same matrix
        ((8, 1, B, 4, 2, B, 4, [0, 2]), (0, 1)),                                 # a column that is read
        ((8, 4, B, 4, 1, B, 4, [3]), (1, 1)),                                    # below the columns read, over Fr
        ((8, 1, B, 4, 3, B, 5, [0]), (0, 1)),                                    # the same base, another stride
        ((8, 1, B + 8, 4, 1, B, 4, [0]), (0, 1)),                                # the same stride, another base: an overlapping foreign span
        ((8, 1, B + 8 * 29, 4, 0, B, 4, [0]), (1, 1)),                           # r ends with element (7, 0) at word 28: word 29 on is free
        ((8, 1, B + 8 * 28, 4, 0, B, 4, [0]), (0, 1)),                           # ... word 28 is not
        ((8, 1, B, 4, 0, B + 8 * 29, 4, [3]), (1, 1)),                           # the other way round: m's span ends with ITS element (7, 0) at word 28
        ((8, 1, B, 4, 1, B + 8 * 29, 4, [3]), (0, 1)),                           # m's span reaches word 29
        ((8, 4, B, 4, 0, B + 32 * 29, 4, [0]), (1, 1)),                          # the same in 32-byte elements
        ((1, 1, B, 1, 0, B + 8, 1, [0]), (1, 1)), ((1, 1, B, 1, 0, B, 1, [0]), (0, 1)),      # one row, one column
        ((8, 1, B, 4, 4, B, 4, [0]), (0, 0)), ((8, 1, B, 1 << 32, 0, B, 4, [0]), (0, 0)), ((8, 1, B, 4, 0, B, 4, [4]), (0, 0)),      # columns and strides that do not pass
        ((8, 1, B, (1 << 32) - 1, (1 << 32) - 2, B, (1 << 32) - 1, [0, (1 << 32) - 3]), (1, 1)),      # the widest stride
        ((1 << 28, 4, B, big, big - 1, B, big, [0, big - 2]), (1, 1)),           # the 2^58 limit: spans of 2^63 bytes, no overflow
        ((1 << 28, 4, B, big, big - 1, B, big, [big - 1]), (0, 1)),
        ((1 << 28, 4, B, big, 0, B + (1 << 62), big, [0]), (0, 1)),              # a foreign base inside that span
        ((1 << 28, 1, B, big + 1, 0, B, big, [0]), (0, 0)),                      # n stride above 2^58
        ((0, 1, B, 4, 2, B, 4, [2]), (1, 1)),                                    # no rows: nothing meets
    ]
    with open(tmp_path / "cmds.txt", "w") as f:
        f.write("".join("plan %d 3 %d %d\n" % (n, nf, w) for n in SHAPES for nf, w in ((1, 1), (8, 4))))
        f.write("".join("plan %d %d %d %d\n" % r for r in refused))
        f.write("".join("alias %d %d %d %d %d %d %d %d %s\n" % (a[:7] + (len(a[7]), " ".join(map(str, a[7])))) for a, _ in alias))
    run = subprocess.run([exe, str(tmp_path / "cmds.txt")], capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", "sanitizer report:\n" + run.stderr[-4000:]
    out = [json.loads(line) for line in run.stdout.splitlines()]
    assert len(out) == 2 * len(SHAPES) + len(refused) + len(alias)
    for i, got in enumerate(out[:2 * len(SHAPES)]):
        n, n_f = SHAPES[i // 2], (1, 8)[i % 2]
        want = expected_plan(n, n_f)
        assert got["ok"] == 1 and got["capacity"] == 1 << want["capBits"] and got["capBits"] == want["capBits"] and got["blocks"] == want["blocks"]
        assert got["launches"] == want["launches"] and got["bytes"] == want["scratchBytes"] and (got["offHeader"], got["offSlots"]) == (0, 64)
        assert got["capacity"] >= max(2 * n, 16) and (got["capacity"] == 16 or got["capacity"] < 4 * n), "the smallest power of two"
    at = 2 * len(SHAPES)
    assert all(g["ok"] == 0 and g["why"] for g in out[at:at + len(refused)])
    at += len(refused)
    assert [(g["ok"], g["columns"]) for g in out[at:]] == [w for _, w in alias]


def test_shared_buffer_check_under_the_sanitizers(tmp_path):
    """csrc/mult_column_plan.h's check_buffers, the one copy that lookup_mult.hip and range_mult.hip call, over addresses that are never
    dereferenced: n = 8 rows of 4 words, t (column 1: a span of 240 bytes), one f with a selector, m and a scratch of 192 bytes"""
    exe = str(tmp_path / "lookup_mult_plan_dump")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                           os.path.join(ROOT, "tests", "lookup_mult_plan_dump.cpp"), "-o", exe])
    B = 1 << 40
    T, F, SEL, M, W, NEED = B, B + 0x1000, B + 0x2000, B + 0x3000, B + 0x4000, 192
    ALIGNED, SHORT, OVER = "t, every f, the selectors, m and the scratch must be 16-byte aligned", "the scratch holds 191 bytes, 192 needed", \
        "the scratch overlaps t, an f, a selector or m"

    def cmd(dev, n=8, work=W, have=NEED, need=NEED, m=M, m_col=3, t=T, f=F, sel=SEL, sel_col=2, t_col=1):
        sides = "%d 4 0 0 0 %d  %d 4 %d 4 %d 0" % (t, t_col, f, sel, sel_col)
        return "buffers %d %d 1 %d %d %d %d 4 %d 1 2 %s\n" % (dev, n, work if dev else 0, have if dev else 0, need, m, m_col, sides)
    cases = [(cmd(1), ""), (cmd(0), "")]
    cases += [(cmd(d, m=0), "null buffer") for d in (0, 1)] + [(cmd(d, f=0), "null buffer") for d in (0, 1)] + [(cmd(d, sel=0, sel_col=9), "") for d in (0, 1)]
    cases += [(cmd(1, work=0), "null buffer"), (cmd(0, work=0), "")]                     # a null scratch: the device form only
    for key, at in (("t", T), ("f", F), ("sel", SEL), ("m", M), ("work", W)):            # one misaligned pointer of each kind
        cases += [(cmd(1, **{key: at + 8}), ALIGNED)]
        cases += [(cmd(0, **{key: at + 8}), "")] if key != "work" else []
    cases += [(cmd(1, have=NEED - 1), SHORT), (cmd(1, have=NEED), ""), (cmd(1, have=NEED + 1), "")]
    cases += [(cmd(1, work=T + 224), OVER), (cmd(1, work=T + 240), "")]                  # t's last byte is 239
    cases += [(cmd(1, work=T + 224, t_col=0), OVER), (cmd(1, work=T + 240, t_col=0), "")]       # ... or 231, inside the scratch's first 16 bytes
    cases += [(cmd(1, work=M - NEED, need=NEED + 1, have=NEED + 1), OVER), (cmd(1, work=M - NEED), "")]      # the scratch's last byte on m's first
    cases += [(cmd(1, work=SEL + 16), OVER), (cmd(1, work=F - NEED + 16), OVER)]
    cases += [(cmd(d, m=T, m_col=1), "m overlaps") for d in (0, 1)] + [(cmd(d, m=T, m_col=0), "") for d in (0, 1)]
    cases += [(cmd(d, m=SEL, m_col=2), "m overlaps") for d in (0, 1)] + [(cmd(d, m=SEL, m_col=2, sel=0), "") for d in (0, 1)]      # an absent selector meets nothing
    cases += [(cmd(1, n=0, m=T, m_col=1, work=T), ""), (cmd(0, n=0, m=T, m_col=1), ""), (cmd(1, n=0, m=0), "null buffer")]      # no rows: nothing meets
    with open(tmp_path / "cmds.txt", "w") as f:
        f.write("".join(c for c, _ in cases))
    run = subprocess.run([exe, str(tmp_path / "cmds.txt")], capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", "sanitizer report:\n" + run.stderr[-4000:]
    out = [json.loads(line)["why"] for line in run.stdout.splitlines()]
    assert len(out) == len(cases)
    for (c, want), got in zip(cases, out):
        assert got == want if want in ("", ALIGNED, SHORT, OVER, "null buffer") else got.startswith(want), (c, got)


# ---- the compute entries ----
def test_compute_entries_refuse_before_any_device_call(lib):
    buf = np.zeros(16384, np.uint64)
    base = buf.ctypes.data + (-buf.ctypes.data % 16)
    cols = np.array([2, 0, 1] + [0] * 14, np.uint64)
    bad_cols = np.array([2, 5, 1], np.uint64)
    rep = (C.c_uint64 * 4)()
    n, k, stride, n_f = 8, 3, 5, 2
    for dev, host, field, words in ((lib.pil2gl_lookup_mult_dev, lib.pil2gl_lookup_mult, "gl", 1),
                                    (lib.pil2gl_bn128_lookup_mult_dev, lib.pil2gl_bn128_lookup_mult, "bn128", 4)):
        need = pilcheck.lookup_mult_plan(n, k, n_f, field)["scratchBytes"]
        span = n * stride * 8 * words
        t, f0, f1, sel, m, work = (base + i * span for i in range(6))
        assert work + need <= buf.ctypes.data + buf.nbytes

        def call(fn=dev, dev_form=True, **kw):
            """the good call with named changes: t_*, f0_*, f1_* fields of a side; m, m_stride, m_col, n, k, n_f, work, need, rep, F, T"""
            side = {"t": dict(base=t, stride=stride, hostCols=cols.ctypes.data, sel=sel, selStride=stride, selCol=4),
                    "f0": dict(base=f0, stride=stride, hostCols=cols.ctypes.data, sel=None, selStride=0, selCol=0),
                    "f1": dict(base=f1, stride=stride, hostCols=cols.ctypes.data, sel=sel, selStride=stride, selCol=3)}
            top = dict(m=m, m_stride=stride, m_col=4, n=n, k=k, n_f=n_f, work=work, need=need, rep=rep, F=0, T=0)
            for key, v in kw.items():
                if key in top:
                    top[key] = v
                else:
                    s, field_name = key.split("_", 1)
                    side[s][field_name] = v
            F = (_lib.TupleSide * 2)(_lib.TupleSide(**side["f0"]), _lib.TupleSide(**side["f1"]))
            T = _lib.TupleSide(**side["t"])
            for i in range(4):
                rep[i] = 5
            args = [None if top["F"] is None else F, top["n_f"], None if top["T"] is None else C.byref(T), top["m"], top["m_stride"], top["m_col"], top["n"], top["k"]]
            return fn(*(args + ([top["work"], top["need"], top["rep"], None] if dev_form else [top["rep"]])))
        err = lib.pil2gl_last_error
        assert call(n=(1 << 28) + 1) == EINVAL and b"2^28" in err()
        assert tuple(rep) == CLEAN, "a refused call leaves a clean report"
        assert call(k=0) == EINVAL and call(k=17) == EINVAL and b"1 .. 16" in err()
        assert call(n_f=0) == EINVAL and call(n_f=9) == EINVAL and b"1 .. 8" in err()
        assert call(t_hostCols=bad_cols.ctypes.data) == EINVAL and b"t: a column >= stride" in err()
        assert call(f1_hostCols=bad_cols.ctypes.data) == EINVAL and b"f 1: a column >= stride" in err()
        assert call(f0_stride=2) == EINVAL and call(t_stride=1 << 32) == EINVAL and b"stride" in err()
        assert call(f0_stride=1 << 31, n=1 << 28) == EINVAL and b"2^58" in err()
        assert call(t_selCol=5) == EINVAL and b"selT" in err()
        assert call(f1_selCol=stride) == EINVAL and b"selF 1" in err()
        assert call(m_col=5) == EINVAL and call(m_stride=1 << 32) == EINVAL and b"m: " in err()
        for key in ("t_base", "f0_base", "f1_hostCols", "t_hostCols", "m", "work", "rep", "F", "T"):
            assert call(**{key: None}) == EINVAL, key
        for key, v in (("t_base", t), ("f1_base", f1), ("t_sel", sel), ("m", m), ("work", work)):
            assert call(**{key: v + 8}) == EINVAL and b"aligned" in err(), key
        assert call(need=need - 16) == EINVAL and b"scratch" in err()
        assert call(work=f0 + 16) == EINVAL and b"overlaps" in err()                             # the scratch inside f0
        assert call(work=sel - 16) == EINVAL and b"overlaps" in err()                            # ... reaching the selectors' first element
        assert call(work=m - 16, need=32) == EINVAL and b"scratch" in err()
        assert call(work=m + 16) == EINVAL and b"the scratch overlaps" in err()                   # ... and m's matrix
        # the aliasing rule, in both directions
        for s in ("t", "f0", "f1"):
            where = dict(t=t, f0=f0, f1=f1)[s]
            assert call(m=where, m_col=0) == EINVAL and b"m overlaps" in err(), "column 0 of %s is read" % s
            assert call(m=where + 16 * words, m_col=1) == EINVAL and b"m overlaps" in err(), "a foreign base over " + s
            assert call(m=where, m_stride=stride + 1) == EINVAL and b"m overlaps" in err(), "another stride over " + s
        assert call(m=sel, m_col=4) == EINVAL and call(m=sel, m_col=3) == EINVAL and b"m overlaps" in err(), "the selectors' columns are read too"
        assert call(n=0) == 0 and tuple(rep) == CLEAN, "n = 0: clean, no device"
        assert call(n=0, t_base=None, f0_base=None, m=None, work=None) == 0
        hcall = lambda **kw: call(fn=host, dev_form=False, **kw)                 # noqa: E731
        assert hcall(n=(1 << 28) + 1) == EINVAL and hcall(k=17) == EINVAL and hcall(n_f=9) == EINVAL
        assert hcall(t_hostCols=bad_cols.ctypes.data) == EINVAL and hcall(m_col=stride) == EINVAL and hcall(f1_selCol=9) == EINVAL
        assert hcall(m=t, m_col=1) == EINVAL and b"m overlaps" in err() and hcall(m=f1 + 8, m_col=4) == EINVAL and b"m overlaps" in err()
        for key in ("t_base", "f1_base", "t_hostCols", "m", "rep", "F", "T"):
            assert hcall(**{key: None}) == EINVAL, key
        assert hcall(n=0) == 0 and tuple(rep) == CLEAN
        if not _have_gpu():
            assert call() == ENODEV
            for s in ("t", "f0", "f1"):
                where = dict(t=t, f0=f0, f1=f1)[s]
                assert call(m=where, m_col=3) == ENODEV and call(m=where, m_col=4) == ENODEV, "a spare column of %s: nothing to refuse" % s
            assert call(f0_base=t, f1_base=t, m=t, m_col=3) == ENODEV, "one matrix on every side and m beside them"
            assert call(m=sel, m_col=2) == ENODEV, "a spare column of the selectors' matrix"
            assert hcall() == ENODEV and hcall(m=t, m_col=3) == ENODEV and hcall(m=m + 8) == ENODEV, "the host forms need no alignment"
    a = np.zeros((8, 4), np.uint64)
    if not _have_gpu():
        with pytest.raises(pil2gl.Pil2glError, match="-2"):
            pilcheck.lookup_mult([(a, [0, 1])], (a, [1, 2]), (a, 3), 8)
        fr = np.zeros((8, 4, 4), np.uint64)
        with pytest.raises(pil2gl.Pil2glError, match="-2"):
            pilcheck.lookup_mult([(fr, [0]), (fr, [1], (fr, 2))], (fr, [1]), (fr, 3), 8, field="bn128")
    with pytest.raises(pil2gl.Pil2glError, match="m overlaps"):
        pilcheck.lookup_mult([(a, [0, 1])], (a, [1, 2]), (a, 2), 8)
    with pytest.raises(pil2gl.Pil2glError, match="need more"):
        pilcheck.lookup_mult([(a, [0, 1])], (a, [1, 2]), (a, 3), 9)
    with pytest.raises(pil2gl.Pil2glError, match="columns"):
        pilcheck.lookup_mult([(a, [0])], (a, [1, 2]), (a, 3), 8)
    with pytest.raises(pil2gl.Pil2glError, match="in place"):
        pilcheck.lookup_mult([(a, [0, 1])], (a, [1, 2]), (a.astype(np.int64), 3), 8)
    assert pilcheck.lookup_mult([(a, [0, 1])], (a, [1, 2]), (a, 3), 0) == CLEAN
