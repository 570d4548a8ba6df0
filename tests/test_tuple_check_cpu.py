"""The lookup and permutation checks without a device: the checker (tests/tuple_check_ref.py) on hand-written cases, the planner through
the ABI and, in a program of its own, under the sanitizers (tests/tuple_check_plan_dump.cpp), the home slot of a tuple, the refusals of
the compute entries before any device call, ENODEV otherwise, and the exported surface."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

import tuple_check_ref as tref
from conn_pols_ref import P, R
from conftest import ROOT

import pil2gl  # noqa: E402  (a plain import: without the feature, or with a broken build, this file fails)
from pil2gl import _lib, pilcheck  # noqa: E402

EINVAL, ENODEV = -1, -2
NONE = tref.NONE
NAMES = ("pil2gl_tuple_check_plan", "pil2gl_tuple_check_dev", "pil2gl_bn128_tuple_check_dev", "pil2gl_tuple_check", "pil2gl_bn128_tuple_check",
         "pil2gl_debug_tuple_home", "pil2gl_debug_tuple_check_probe")
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
    for f in ("tuple_check_plan", "lookup_check", "perm_check", "lookup_check_dev", "perm_check_dev", "tuple_home", "tuple_check_probe"):
        assert callable(getattr(pilcheck, f))
    assert pilcheck.tuple_check_probe() >= 0
    addon = open(os.path.join(ROOT, "pil2-stark-js_amd", "addon", "pil2gl_napi.cc")).read()
    for n in ("tupleCheckPlan", "tupleCheckDev", "tupleCheck", "tupleHome", "tupleCheckProbe"):
        assert '"%s"' % n in addon, n + " is not exported by the addon"
    index = open(os.path.join(ROOT, "pil2-stark-js_amd", "js", "index.js")).read()
    assert "pil_checks.js" in index


# ---- the checker against hand-written cases ----
L, M = tref.LOOKUP, tref.PERMUTATION
CLEAN = tref.CLEAN_REPORT


def test_checker_clean_and_each_kind():
    t = [(1, 2), (3, 4), (3, 4), (5, 6)]
    assert tref.check([(3, 4), (1, 2), (3, 4), (3, 4)], t, L, P) == CLEAN, "a lookup may use a row of t any number of times"
    assert tref.check([(3, 4), (5, 6), (1, 2), (3, 4)], t, M, P) == CLEAN
    assert tref.check([(3, 4), (7, 7), (1, 2), (7, 7)], t, L, P) == (1, 1, NONE, 2, 0)
    assert tref.check([(3, 4), (7, 7), (1, 2), (7, 7)], t, M, P) == (1, 1, NONE, 2, 0)
    # (1, 2) twice in f, once in t: the FIRST occurrence in f is named, not the second a decrementing walk would stop at
    assert tref.check([(1, 2), (3, 4), (3, 4), (1, 2)], t, M, P) == (2, 0, 0, 2, 1)
    assert tref.check([(1, 2), (3, 4), (3, 4), (1, 2)], t, L, P) == CLEAN
    # f one short: no row of f fails, so the first row of t whose tuple t has more often; its partner is the first f row with it
    assert tref.check([(5, 6), (3, 4), (1, 2)] + [(3, 4)], [(3, 4), (3, 4), (3, 4), (1, 2)], M, P, sel_t=[1, 1, 1, 1],
                      sel_f=[0, 1, 1, 1]) == (3, 0, 1, 2, 3)
    assert tref.check([(1, 2)], [(3, 4)], M, P, sel_f=[0]) == (3, 0, NONE, 0, 1)


def test_checker_f_goes_before_t_in_a_permutation():
    f = [(9, 9), (1, 1), (2, 2), (2, 2)]
    t = [(8, 8), (1, 1), (2, 2), (7, 7)]
    assert tref.check(f, t, M, P) == (1, 0, NONE, 1, 0), "row 0 of t fails too, and is smaller: f is reported first"
    assert tref.check(f[1:], t[1:], M, P) == (2, 1, 1, 2, 1), "kind 2 at f row 1, partner t row 1 (rows renumbered)"
    assert tref.check([(1, 1)], [(8, 8)], M, P, sel_f=[0]) == (3, 0, NONE, 0, 1), "kind 3 only when no row of f fails"


def test_checker_order_last_column_and_representatives():
    assert tref.check([(1, 2)], [(2, 1)], L, P) == (1, 0, NONE, 1, 0), "(a, b) is not (b, a)"
    assert tref.check([(1, 2, 3, 4)], [(1, 2, 3, 5)], L, P) == (1, 0, NONE, 1, 0), "the last column decides"
    assert tref.check([(5, 7 + P)], [(5 + P, 7)], M, P) == CLEAN, "x and x + p are one value over Goldilocks"
    pat = 3 * R + 11
    assert pat < 1 << 256
    assert tref.check([(pat,)], [(11,)], M, R) == CLEAN, "an Fr pattern >= r counts as its residue"
    assert tref.check([(pat,)], [(12,)], M, R) == (1, 0, NONE, 1, 0)


def test_checker_selector_words():
    f = [(1,), (2,), (3,), (4,)]
    sel = [0, P, 1, (1 << 64) - 1]                                               # 0 and p are zero; 1 and 2^64 - 1 (= 2^32 - 2 mod p) select
    assert tref.check(f, [(3,), (4,), (0,), (0,)], L, P, sel_f=sel) == CLEAN
    assert tref.check(f, [(3,), (0,), (0,), (0,)], L, P, sel_f=sel) == (1, 3, NONE, 1, 0)
    assert tref.check(f, f, M, P, sel_f=sel, sel_t=[1, 1, 0, 0]) == (1, 2, NONE, 1, 0)
    assert tref.check(f, f, M, P, sel_f=sel, sel_t=sel) == CLEAN
    assert tref.check([(1,)] * 4, [(1,)] * 4, L, P, sel_f=[0] * 4) == CLEAN, "nothing selected in f: nothing to look up"
    assert tref.check([(1,)] * 4, [(1,)] * 4, M, P, sel_f=[0] * 4) == (3, 0, NONE, 0, 4)


# ---- the planner ----
SHAPES = (0, 1, 2, 4, 5, 8, 16, 63, 64, 65, 1000, 1 << 12, (1 << 20) + 1, 1 << 22, 1 << 28)


def expected_plan(n):
    cap = 16
    while cap < 4 * n:
        cap *= 2
    blocks = min(max(-(-2 * n // 256), 1), 2048)
    return {"capBits": cap.bit_length() - 1, "threads": 256, "blocks": blocks, "launches": 3, "headerBytes": 64, "slotBytes": 16,
            "scratchBytes": 64 + 16 * cap if n else 0}


def test_plan_capacity_geometry_and_scratch():
    last = 0
    for n in SHAPES:
        for field in ("gl", "bn128"):
            for mode in (0, 1):
                info = pilcheck.tuple_check_plan(n, 3, field, mode)
                assert info == expected_plan(n), (n, field, mode)
        cap = 1 << info["capBits"]
        assert cap >= 16 and cap >= 2 * (2 * n), "at least twice the rows that can be inserted: both sides' n"
        assert cap & (cap - 1) == 0 and info["scratchBytes"] % 16 == 0
        assert info["scratchBytes"] >= last, "monotone in n"
        last = info["scratchBytes"]
    assert pilcheck.tuple_check_plan(8, 1)["capBits"] == 5, "n = 8: 32 slots (the collision test of the GPU file relies on it)"


def test_plan_refusals(lib):
    info = (C.c_uint32 * 6)()
    b = C.c_uint64(7)
    for n, k, words, mode, msg in (((1 << 28) + 1, 3, 1, 0, b"2^28"), (8, 0, 1, 0, b"1 .. 16"), (8, 17, 4, 1, b"1 .. 16"), (8, 3, 2, 0, b"elemWords"),
                                   (8, 3, 1, 2, b"mode"), (1 << 63, 3, 1, 0, b"2^28")):
        assert lib.pil2gl_tuple_check_plan(n, k, words, mode, info, C.byref(b)) == EINVAL and b.value == 0, (n, k, words, mode)
        assert msg in lib.pil2gl_last_error(), lib.pil2gl_last_error()
    assert lib.pil2gl_tuple_check_plan(1 << 28, 16, 4, 1, info, C.byref(b)) == 0 and info[0] == 30 and b.value == 64 + (16 << 30)
    assert lib.pil2gl_tuple_check_plan(64, 3, 1, 0, None, None) == 0
    with pytest.raises(pil2gl.Pil2glError, match="-1"):
        pilcheck.tuple_check_plan(8, 17)


def test_planner_header_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "tuple_check_plan_dump")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                           os.path.join(ROOT, "tests", "tuple_check_plan_dump.cpp"), "-o", exe])
    refused = [((1 << 28) + 1, 3, 1, 0), (8, 0, 1, 0), (8, 17, 1, 0), (8, 3, 3, 0), (8, 3, 1, 2), ((1 << 64) - 1, 3, 4, 1)]
    columns = [((8, 4, [3, 1]), 1), ((8, 4, [4, 1]), 0), ((8, 4, [0, 0, 3, 3]), 1), ((8, 1 << 32, [0]), 0), ((8, 1, [0] * 16), 1), ((8, 0, [0]), 0), ((8, 4, []), 0),
               ((1 << 28, 1 << 30, [(1 << 30) - 1]), 1), ((1 << 28, (1 << 30) + 1, [0]), 0), ((1 << 28, (1 << 32) - 1, [0]), 0), ((1 << 26, (1 << 32) - 1, [5]), 1)]
    spans = [((4, 8, 5, 4), (3 * 8 + 5 + 1) * 32), ((0, 8, 5, 1), 0), ((1, 1, 0, 1), 8), ((1 << 28, 1 << 30, (1 << 30) - 1, 4), 1 << 63)]      # the largest that passes
    homes = [(2, 1, 32, [5, 0]), (2, 1, 32, [0, 5]), (2, 1, 32, [5, 0]), (1, 4, 1 << 30, [1, 2, 3, 4]), (16, 4, 16, list(range(64)))]
    with open(tmp_path / "cmds.txt", "w") as f:
        f.write("".join("plan %d 3 %d %d\n" % (n, w, m) for n in SHAPES for w, m in ((1, 0), (4, 1))))
        f.write("".join("plan %d %d %d %d\n" % r for r in refused))
        f.write("".join("columns %d %d %d %s\n" % (n, s, len(c), " ".join(map(str, c))) for (n, s, c), _ in columns))
        f.write("".join("span %d %d %d %d\n" % s for s, _ in spans))
        f.write("".join("home %d %d %d %s\n" % (k, w, cap, " ".join(map(str, ws))) for k, w, cap, ws in homes))
    run = subprocess.run([exe, str(tmp_path / "cmds.txt")], capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", "sanitizer report:\n" + run.stderr[-4000:]
    out = [json.loads(l) for l in run.stdout.splitlines()]
    assert len(out) == 2 * len(SHAPES) + len(refused) + len(columns) + len(spans) + len(homes)
    for k, got in enumerate(out[:2 * len(SHAPES)]):
        n = SHAPES[k // 2]
        want = expected_plan(n)
        assert got["ok"] == 1 and got["rows"] == 2 * n and got["capacity"] == 1 << want["capBits"] and got["capBits"] == want["capBits"]
        assert got["blocks"] == want["blocks"] and got["bytes"] == want["scratchBytes"]
        parts = [got["offHeader"], got["offSlots"], got["offMinF"], got["offCounts"]]
        assert parts == sorted(parts) and all(p % 16 == 0 for p in parts) and parts[:2] == [0, 64], "every part on 16 bytes, header first"
        assert got["offMinF"] - got["offSlots"] == got["offCounts"] - got["offMinF"] == 4 * got["capacity"]
        assert n == 0 or got["bytes"] - got["offCounts"] == 8 * got["capacity"]
    at = 2 * len(SHAPES)
    assert all(g["ok"] == 0 and g["why"] for g in out[at:at + len(refused)])
    at += len(refused)
    assert [g["ok"] for g in out[at:at + len(columns)]] == [ok for _, ok in columns]
    at += len(columns)
    assert [g["bytes"] for g in out[at:at + len(spans)]] == [b for _, b in spans]
    got = [g["home"] for g in out[at + len(spans):]]
    assert got[0] == got[2] and all(h < cap for h, (_, _, cap, _) in zip(got, homes))
    for h, (k, w, cap, ws) in zip(got, homes):
        assert h == pilcheck.tuple_home(np.array(ws, np.uint64), k, "gl" if w == 1 else "bn128", cap), "the program and the library share the function"


# ---- the home slot ----
def test_tuple_home_is_below_capacity_deterministic_and_ordered(lib):
    for field, words in (("gl", 1), ("bn128", 4)):
        for cap in (16, 32, 1 << 20, 1 << 30):
            seen = set()
            for i in range(200):
                tup = np.arange(i, i + 3 * words, dtype=np.uint64)
                h = pilcheck.tuple_home(tup, 3, field, cap)
                assert 0 <= h < cap and h == pilcheck.tuple_home(tup.copy(), 3, field, cap)
                seen.add(h)
            assert len(seen) > (8 if cap == 16 else 24), "the slots spread"
        ab = [pilcheck.tuple_home(np.array(v, np.uint64).repeat(words), 2, field, 1 << 30) for v in ((1, 2), (2, 1))]
        assert ab[0] != ab[1], "(a, b) and (b, a) land apart in a table of 2^30 slots"
    one = np.array([7], np.uint64)
    assert lib.pil2gl_debug_tuple_home(one.ctypes.data, 1, 1, 48) == NONE and lib.pil2gl_debug_tuple_home(one.ctypes.data, 0, 1, 16) == NONE
    assert lib.pil2gl_debug_tuple_home(None, 1, 1, 16) == NONE and lib.pil2gl_debug_tuple_home(one.ctypes.data, 1, 2, 16) == NONE
    with pytest.raises(pil2gl.Pil2glError):
        pilcheck.tuple_home(one, 2, "gl", 16)


# ---- the compute entries ----
def test_compute_entries_refuse_before_any_device_call(lib):
    buf = np.zeros(16384, np.uint64)
    base = buf.ctypes.data + (-buf.ctypes.data % 16)
    cols = np.array([2, 0, 1] + [0] * 14, np.uint64)
    bad_cols = np.array([2, 4, 1], np.uint64)
    pc = cols.ctypes.data
    rep = (C.c_uint64 * 5)()
    n, k, stride = 8, 3, 4
    for dev, host, field, words in ((lib.pil2gl_tuple_check_dev, lib.pil2gl_tuple_check, "gl", 1),
                                    (lib.pil2gl_bn128_tuple_check_dev, lib.pil2gl_bn128_tuple_check, "bn128", 4)):
        need = pilcheck.tuple_check_plan(n, k, field)["scratchBytes"]
        span = n * stride * 8 * words
        f, t, sf, st, work = base, base + span, base + 2 * span, base + 3 * span, base + 4 * span
        assert work + need <= buf.ctypes.data + buf.nbytes
        ok = [f, stride, pc, t, stride, pc, sf, stride, 3, st, stride, 3, n, k, 1, work, need, rep, None]

        def call(fn=dev, upto=19, **kw):
            args = list(ok)
            for key, v in kw.items():
                args[int(key[1:])] = v
            for i in range(5):
                rep[i] = 5
            return fn(*args[:upto])
        assert call(a12=(1 << 28) + 1) == EINVAL and b"2^28" in lib.pil2gl_last_error()
        assert tuple(rep) == tref.CLEAN_REPORT, "a refused call leaves a clean report"
        assert call(a13=0) == EINVAL and call(a13=17) == EINVAL and b"1 .. 16" in lib.pil2gl_last_error()
        assert call(a14=2) == EINVAL and b"mode" in lib.pil2gl_last_error()
        assert call(a2=bad_cols.ctypes.data) == EINVAL and b"f: a column >= stride" in lib.pil2gl_last_error()
        assert call(a5=bad_cols.ctypes.data) == EINVAL and b"t: a column >= stride" in lib.pil2gl_last_error()
        assert call(a1=2) == EINVAL and call(a4=1 << 32) == EINVAL and b"stride" in lib.pil2gl_last_error()
        assert call(a8=4) == EINVAL and b"selF" in lib.pil2gl_last_error()
        assert call(a11=stride) == EINVAL and b"selT" in lib.pil2gl_last_error()
        for i in (0, 2, 3, 5, 15, 17):
            assert call(**{"a%d" % i: None}) == EINVAL, i
        for i in (0, 3, 6, 9, 15):
            assert call(**{"a%d" % i: ok[i] + 8}) == EINVAL and b"aligned" in lib.pil2gl_last_error(), i
        assert call(a16=need - 16) == EINVAL and b"scratch" in lib.pil2gl_last_error()
        assert call(a15=f + 16) == EINVAL and b"overlaps" in lib.pil2gl_last_error()                 # the scratch inside f
        assert call(a15=t - 16) == EINVAL and b"overlaps" in lib.pil2gl_last_error()
        assert call(a15=sf + span - 16) == EINVAL and b"overlaps" in lib.pil2gl_last_error()         # ... reaching selF's last element
        assert call(a15=st - need + 16 * words) == EINVAL and b"overlaps" in lib.pil2gl_last_error()      # ... and selT's first
        assert call(a12=0) == 0 and tuple(rep) == tref.CLEAN_REPORT, "n = 0: clean, no device"
        assert call(a12=0, a0=None, a3=None, a15=None) == 0
        if not _have_gpu():
            assert call() == ENODEV
            assert call(a3=f, a6=None, a9=f, a14=0) == ENODEV, "one matrix on both sides, a null selector: nothing to refuse"
        # the host forms: the same 15 arguments, then the report
        hok = ok[:15] + [rep]
        assert host(*[(1 << 28) + 1 if i == 12 else v for i, v in enumerate(hok)]) == EINVAL
        assert host(*[17 if i == 13 else v for i, v in enumerate(hok)]) == EINVAL
        assert host(*[3 if i == 14 else v for i, v in enumerate(hok)]) == EINVAL
        assert host(*[bad_cols.ctypes.data if i == 2 else v for i, v in enumerate(hok)]) == EINVAL
        assert host(*[9 if i == 11 else v for i, v in enumerate(hok)]) == EINVAL
        for i in (0, 2, 3, 5, 15):
            assert host(*[None if j == i else v for j, v in enumerate(hok)]) == EINVAL, i
        rep[0] = 5
        assert host(*[0 if i == 12 else v for i, v in enumerate(hok)]) == 0 and tuple(rep) == tref.CLEAN_REPORT
        if not _have_gpu():
            assert host(*hok) == ENODEV
    m = np.zeros((8, 4), np.uint64)
    if not _have_gpu():
        with pytest.raises(pil2gl.Pil2glError, match="-2"):
            pilcheck.lookup_check(m, [0, 1], m, [2, 3], 8)
        with pytest.raises(pil2gl.Pil2glError, match="-2"):
            pilcheck.perm_check(np.zeros((8, 4, 4), np.uint64), [0], m.reshape(2, 4, 4), [3], 2, field="bn128", sel_t=(m.reshape(2, 4, 4), 1))
    with pytest.raises(pil2gl.Pil2glError, match="need more"):
        pilcheck.lookup_check(m, [0, 1], m, [2, 3], 9)
    with pytest.raises(pil2gl.Pil2glError, match="columns"):
        pilcheck.lookup_check(m, [0, 1], m, [2], 8)
    with pytest.raises(pil2gl.Pil2glError, match="stride"):
        pilcheck.lookup_check(m.reshape(-1), [0], m, [2], 8)
    with pytest.raises(pil2gl.Pil2glError, match="-1"):
        pilcheck.perm_check(np.zeros((9, 4), np.uint64), [4], m, [2], 8)          # room for it, so the library is the one to refuse
    assert pilcheck.perm_check(m, [0], m, [2], 0) == tref.CLEAN_REPORT
