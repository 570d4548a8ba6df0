"""The multiplicity sessions without a device: the exported surface, the plans of both kinds through the ABI and, in a program of its own,
under the sanitizers (tests/mult_session_plan_dump.cpp), the refusals of open, add and write before any device call -- a side is checked
against ITS OWN row count --, ENODEV otherwise, and the checker (tests/mult_session_ref.py) against the one-shot checkers."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

import lookup_mult_ref as lref
import mult_session_ref as sref
import range_mult_ref as rref
from conn_pols_ref import P, R
from conftest import ROOT

import pil2gl  # noqa: E402,F401  (a plain import: with a broken build this file fails; without the feature every test but the checker's own does)
from pil2gl import _lib, pilcheck  # noqa: E402

EINVAL, ENODEV = -1, -2
NONE = sref.NONE
CLEAN = (0, NONE, NONE, 0)
CSRC = os.path.join(ROOT, "pil2-stark-js_amd", "csrc")
KINDS = ("lookup", "range")
NAMES = (["pil2gl_%s_session_plan" % kind for kind in KINDS] + ["pil2gl_range_session_open_dev", "pil2gl_debug_range_session_plan"]
         + ["pil2gl_%slookup_session_open_dev" % f for f in ("", "bn128_")]
         + ["pil2gl_%s%s_session_%s_dev" % (f, kind, e) for f in ("", "bn128_") for kind in KINDS for e in ("add", "write")]
         + ["pil2gl_debug_lookup_session_open_dev", "pil2gl_debug_range_session_open_dev", "pil2gl_debug_range_session_add_dev"])
VOID_NAMES = ("pil2gl_debug_mult_session_grids",)


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
    text = open(os.path.join(ROOT, "include", "pil2gl.h")).read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert len(NAMES) == 17
    for n in NAMES:
        decl = re.search(r"\bint %s\s*\(([^;]*)\);" % n, header)
        assert decl, n + " is not declared in pil2gl.h"
        assert n in _lib.SIGNATURES, n + " is not bound in _lib.py"
        assert getattr(lib, n)
        args = [a.strip() for a in decl.group(1).split(",")]
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
    for n in VOID_NAMES:
        assert re.search(r"\bvoid %s\s*\(" % n, header) and _lib.SIGNATURES[n][0] is None and getattr(lib, n)
    grids = (C.c_uint32 * 8)(*[7] * 8)
    lib.pil2gl_debug_mult_session_grids(grids)
    lib.pil2gl_debug_mult_session_grids(None)
    assert _have_gpu() or list(grids) == [0] * 8, "no add yet in a process without a device"
    top = text.split("#pragma once")[0]
    assert "lookup_session_plan, range_session_plan" in top and "the add of a lookup_session or range_session" in top
    for f in ("LookupSession", "RangeSession", "range_logup_cross", "lookup_session_plan", "range_session_plan"):
        assert callable(getattr(pilcheck, f))
    addon = open(os.path.join(ROOT, "pil2-stark-js_amd", "addon", "pil2gl_napi.cc")).read()
    for kind in KINDS:
        for n in ("Plan", "OpenDev", "AddDev", "WriteDev"):
            assert '"%sSession%s"' % (kind, n) in addon, kind + n + " is not exported by the addon"
    js = open(os.path.join(ROOT, "pil2-stark-js_amd", "js", "pil_checks.js")).read()
    assert re.search(r"module\.exports = \{[^}]*LookupSession, RangeSession, lookupSessionPlan, rangeSessionPlan", js)


# ---- the plans ----
def lookup_plan(n_t):
    cap_bits = max(4, (2 * n_t - 1).bit_length()) if n_t else 4
    return {"capBits": cap_bits, "threads": 256, "blocks": 2048, "headerBytes": 64, "slotBytes": 16, "openLaunches": 2, "addLaunches": 2, "writeLaunches": 1,
            "scratchBytes": 64 + 16 * (1 << cap_bits) if n_t else 0}


def range_plan(size, path=None):
    lds = size <= 8192 if path is None else path == 0
    return {"path": 0 if lds else 1, "threads": 1024 if lds else 256, "blocks": 512 if lds else 2048, "headerBytes": 64, "counterBytes": 8, "openLaunches": 1,
            "addLaunches": 2, "writeLaunches": 1, "scratchBytes": (64 + 8 * size + 15) // 16 * 16}


def test_plan_words_of_both_kinds_and_fields(lib):
    for field in ("gl", "bn128"):
        for n_t in (0, 1, 5, 8, 9, 64, 1000, 1 << 20, (1 << 28) - 1, 1 << 28):
            for k in (1, 16):
                assert pilcheck.lookup_session_plan(n_t, k, field) == lookup_plan(n_t), (n_t, k, field)
        for size in (1, 2, 3, 200, 8191, 8192, 8193, 1 << 16, 1 << 28):
            assert pilcheck.range_session_plan(size, field) == range_plan(size), (size, field)
        assert pilcheck.range_session_plan(8192, field)["path"] == 0 and pilcheck.range_session_plan(8193, field)["path"] == 1, "the threshold"
        for path in (0, 1):
            assert pilcheck.range_session_plan(300, field, path) == range_plan(300, path)
        assert pilcheck.range_session_plan(300, field, 2) == pilcheck.range_session_plan(300, field)
    assert pilcheck.lookup_session_plan(5, 3)["scratchBytes"] == 64 + 16 * 16 and pilcheck.range_session_plan(5)["scratchBytes"] == 112
    # the one-shot plans keep their layout: 8-byte slots, 4-byte counters
    assert pilcheck.lookup_mult_plan(5, 3)["slotBytes"] == 8 and pilcheck.range_mult_plan(5, 5)["scratchBytes"] == 96
    info = (C.c_uint32 * 6)()
    b = C.c_uint64(7)
    for args, msg in ((((1 << 28) + 1, 3, 1), b"nT must"), ((8, 0, 1), b"1 .. 16"), ((8, 17, 4), b"1 .. 16"), ((8, 3, 2), b"elemWords"), ((1 << 63, 3, 1), b"nT must")):
        assert lib.pil2gl_lookup_session_plan(*args, info, C.byref(b)) == EINVAL and b.value == 0 and msg in lib.pil2gl_last_error(), args
    for args, msg in (((0, 1), b"size"), (((1 << 28) + 1, 4), b"size"), ((8, 3), b"elemWords")):
        assert lib.pil2gl_range_session_plan(*args, info, C.byref(b)) == EINVAL and b.value == 0 and msg in lib.pil2gl_last_error(), args
    assert lib.pil2gl_debug_range_session_plan(8193, 1, 0, info, C.byref(b)) == EINVAL and b"8192" in lib.pil2gl_last_error()
    assert lib.pil2gl_debug_range_session_plan(8, 1, 3, info, C.byref(b)) == EINVAL and b"path" in lib.pil2gl_last_error()
    assert lib.pil2gl_lookup_session_plan(64, 3, 1, None, None) == 0 and lib.pil2gl_range_session_plan(64, 4, None, None) == 0


def test_planner_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "mult_session_plan_dump")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                           os.path.join(ROOT, "tests", "mult_session_plan_dump.cpp"), "-o", exe])
    B = 1 << 40                                       # a byte address; never dereferenced
    lookups = [(n_t, k, w) for n_t in (0, 1, 5, 8, 9, 1000, 1 << 28) for k, w in ((1, 1), (16, 4))]
    lookups_bad = [((1 << 28) + 1, 1, 1), (8, 0, 1), (8, 17, 1), (8, 1, 3), ((1 << 64) - 1, (1 << 64) - 1, 4)]
    ranges = [(size, w, path) for size in (1, 2, 8192, 8193, 1 << 28) for w in (1, 4) for path in (2,)] + [(300, 1, 0), (300, 1, 1)]
    ranges_bad = [(0, 1, 2), ((1 << 28) + 1, 1, 2), (8193, 1, 0), (8, 1, 3), (8, 2, 2), ((1 << 64) - 1, 4, 2)]
    grids = [((1, 1), 1), ((100, 1), 1), ((256, 1), 1), ((257, 1), 2), ((1 << 28, 1), 2048), ((1, 0), 1), ((100, 0), 1), ((1025, 0), 2), ((1 << 28, 0), 512),
             ((100, 2), 1)]
    big = 1 << 30
    sides = [  # (k, [(rows, stride, col, selStride, selCol, hasSel)..]) -> ok
        ((1, [(8, 4, 3, 0, 0, 0)]), 1), ((1, [(8, 4, 4, 0, 0, 0)]), 0), ((3, [(0, 0, 9, 0, 0, 0), (1, 1, 0, 0, 0, 0)]), 1),   # 0 rows: not looked at
        ((1, [(1 << 28, 4, 0, 0, 0, 0)]), 1), ((1, [((1 << 28) + 1, 4, 0, 0, 0, 0)]), 0), ((1, [((1 << 64) - 1, 1, 0, 0, 0, 0)]), 0),
        ((1, [(1 << 28, big, 0, 0, 0, 0)]), 1), ((1, [(1 << 28, big + 1, 0, 0, 0, 0)]), 0), ((1, [(5, big + 1, 0, 0, 0, 0)]), 1),  # 2^58 by ITS rows
        ((1, [(8, 4, 0, 4, 4, 1)]), 0), ((1, [(8, 4, 0, 4, 3, 1)]), 1), ((1, [(8, 1 << 32, 0, 0, 0, 0)]), 0),
        ((1, []), 0), ((1, [(1, 1, 0, 0, 0, 0)] * 8), 1), ((1, [(1, 1, 0, 0, 0, 0)] * 9), 0),
    ]
    spans = [  # (scratch, scratchBytes, planBytes, [(base, bytes)..]) -> ok
        ((B, 128, 128, []), 1), ((0, 128, 128, []), 0), ((B + 8, 128, 128, []), 0), ((B, 112, 128, []), 0),
        ((B, 128, 128, [(B + 128, 64)]), 1), ((B, 128, 128, [(B + 112, 64)]), 0), ((B, 128, 128, [(B - 64, 64)]), 1), ((B, 128, 128, [(B - 64, 65)]), 0),
        ((B, 128, 128, [(B + 256, 64), (0, 64)]), 0), ((B, 128, 128, [(B + 256, 64), (B + 264, 64)]), 0), ((B, 1 << 62, 1 << 62, [(B + (1 << 62), 1 << 62)]), 1),
    ]
    with open(tmp_path / "cmds.txt", "w") as f:
        f.write("".join("lookup %d %d %d\n" % r for r in lookups + lookups_bad))
        f.write("".join("range %d %d %d\n" % r for r in ranges + ranges_bad))
        f.write("".join("grid %d %d\n" % g for g, _ in grids))
        f.write("".join("sides %d %d %s\n" % (k, len(ss), " ".join(" ".join(map(str, s)) for s in ss)) for (k, ss), _ in sides))
        f.write("".join("spans %d %d %d %d %s\n" % (a[:3] + (len(a[3]), " ".join("%d %d" % s for s in a[3]))) for a, _ in spans))
    run = subprocess.run([exe, str(tmp_path / "cmds.txt")], capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", "sanitizer report:\n" + run.stderr[-4000:]
    out = [json.loads(line) for line in run.stdout.splitlines()]
    assert len(out) == len(lookups) + len(lookups_bad) + len(ranges) + len(ranges_bad) + len(grids) + len(sides) + len(spans)
    for (n_t, k, w), got in zip(lookups, out):
        want = lookup_plan(n_t)
        assert got["ok"] == 1 and got["capBits"] == want["capBits"] and got["capacity"] == 1 << want["capBits"] and got["bytes"] == want["scratchBytes"], (n_t, got)
        assert got["offSlots"] == 64 and got["blocks"] == min(max(-(-n_t // 256), 1), 2048)
    at = len(lookups)
    assert all(g["ok"] == 0 and g["why"] for g in out[at:at + len(lookups_bad)])
    at += len(lookups_bad)
    for (size, w, path), got in zip(ranges, out[at:]):
        want = range_plan(size, None if path == 2 else path)
        assert got["ok"] == 1 and (got["path"], got["threads"], got["bytes"]) == (want["path"], want["threads"], want["scratchBytes"]), (size, got)
        assert got["offCounters"] == 64 and got["ldsCounters"] == (size if want["path"] == 0 else 0) and got["bytes"] >= 64 + 8 * size
    at += len(ranges)
    assert all(g["ok"] == 0 and g["why"] for g in out[at:at + len(ranges_bad)])
    at += len(ranges_bad)
    assert [g["blocks"] for g in out[at:at + len(grids)]] == [w for _, w in grids], "a count launch's grid comes from its side's rows"
    at += len(grids)
    assert [g["ok"] for g in out[at:at + len(sides)]] == [w for _, w in sides]
    at += len(sides)
    assert [g["ok"] for g in out[at:]] == [w for _, w in spans]


# ---- the compute entries ----
def test_compute_entries_refuse_before_any_device_call(lib):
    buf = np.zeros(1 << 16, np.uint64)
    base = buf.ctypes.data + (-buf.ctypes.data % 16)
    cols01 = np.array([0, 1], np.uint64)
    col2 = np.array([2], np.uint64)
    bad_col = np.array([5, 0], np.uint64)
    rep = (C.c_uint64 * 4)()
    total = C.c_uint64()
    err = lib.pil2gl_last_error
    stride, n_t, size = 4, 8, 6
    for words, pre in ((1, "pil2gl_"), (4, "pil2gl_bn128_")):
        field = "gl" if words == 1 else "bn128"
        span = 64 * stride * 8 * words                # room for 64 rows a matrix
        t, f0, f1, sel, m, work = (base + i * span for i in range(6))
        assert work + (1 << 12) <= buf.ctypes.data + buf.nbytes
        for kind in KINDS:
            k = 2 if kind == "lookup" else 1
            need = (pilcheck.lookup_session_plan(n_t, k, field) if kind == "lookup" else pilcheck.range_session_plan(size, field))["scratchBytes"]
            cols = cols01 if kind == "lookup" else col2

            def call(entry, **kw):
                """the good call of `entry` (open, add, write) with named changes: t_*, f0_*, f1_* fields of a side; rows; n_t, k, lo, size, row0, n_m,
                n_f, m, m_stride, m_col, work, need, rep, total, F, T, R"""
                side = {"t": dict(base=t, stride=stride, hostCols=cols01.ctypes.data, sel=None, selStride=0, selCol=0),
                        "f0": dict(base=f0, stride=stride, hostCols=cols.ctypes.data, sel=None, selStride=0, selCol=0),
                        "f1": dict(base=f1, stride=stride, hostCols=cols.ctypes.data, sel=sel, selStride=stride, selCol=3)}
                top = dict(rows=[3, 40], n_t=n_t, k=k, lo=-1, size=size, row0=1, n_m=n_t, n_f=2, m=m, m_stride=stride, m_col=3, work=work, need=need, rep=rep,
                           total=C.byref(total), F=0, T=0, R=0)
                for key, v in kw.items():
                    if key in top:
                        top[key] = v
                    else:
                        s, name = key.split("_", 1)
                        side[s][name] = v
                F = None if top["F"] is None else (_lib.TupleSide * 2)(_lib.TupleSide(**side["f0"]), _lib.TupleSide(**side["f1"]))
                T = None if top["T"] is None else (_lib.TupleSide * 1)(_lib.TupleSide(**side["t"]))
                rows = np.array(top["rows"], np.uint64)
                Rw = None if top["R"] is None else C.c_void_p(rows.ctypes.data)
                for i in range(4):
                    rep[i] = 5
                scratch = [top["work"], top["need"]]
                if kind == "lookup":
                    head = [T, top["n_t"], top["k"]]
                    if entry == "open":
                        return getattr(lib, pre + "lookup_session_open_dev")(*head, *scratch, None)
                    if entry == "add":
                        return getattr(lib, pre + "lookup_session_add_dev")(*head, F, Rw, top["n_f"], *scratch, top["rep"], None)
                    return getattr(lib, pre + "lookup_session_write_dev")(*head, top["m"], top["m_stride"], top["m_col"], *scratch, top["total"], None)
                if entry == "open":
                    return lib.pil2gl_range_session_open_dev(top["size"], *scratch, None)
                if entry == "add":
                    return getattr(lib, pre + "range_session_add_dev")(top["lo"], top["size"], F, Rw, top["n_f"], *scratch, top["rep"], None)
                return getattr(lib, pre + "range_session_write_dev")(top["size"], top["row0"], top["m"], top["m_stride"], top["m_col"], top["n_m"], *scratch, top["total"], None)

            # what the plans refuse, in every entry
            for entry in ("open", "add", "write"):
                if kind == "lookup":
                    assert call(entry, n_t=(1 << 28) + 1) == EINVAL and b"2^28" in err(), entry
                    assert call(entry, k=0) == EINVAL and call(entry, k=17) == EINVAL and b"1 .. 16" in err(), entry
                    assert call(entry, T=None) == EINVAL, entry
                    assert call(entry, t_hostCols=bad_col.ctypes.data) == EINVAL and b"t: a column >= stride" in err(), entry
                    assert call(entry, t_base=None) == EINVAL and call(entry, t_base=t + 8) == EINVAL and b"aligned" in err(), entry
                    assert call(entry, work=t + 16) == EINVAL and b"scratch overlaps" in err(), "the scratch inside t"
                    assert call(entry, n_t=0) == 0, "nT = 0: OK, nothing done, no device"
                    assert call(entry, n_t=0, t_base=None, work=None, m=None) == 0
                else:
                    assert call(entry, size=0) == EINVAL and call(entry, size=(1 << 28) + 1) == EINVAL and b"size" in err(), entry
                assert call(entry, work=None) == EINVAL and call(entry, work=work + 8) == EINVAL and b"aligned" in err(), entry
                assert call(entry, need=need - 16) == EINVAL and b"scratch holds" in err(), entry
            # add
            assert call("add", n_f=0) == EINVAL and call("add", n_f=9) == EINVAL and call("add", n_f=1 << 40) == EINVAL and b"1 .. 8" in err()
            assert tuple(rep) == CLEAN, "a refused add leaves a clean report"
            assert call("add", rows=[3, (1 << 28) + 1]) == EINVAL and b"f 1: a side has at most 2^28 rows" in err()
            assert call("add", rep=None) == EINVAL and call("add", F=None) == EINVAL and call("add", R=None) == EINVAL
            assert call("add", f0_hostCols=bad_col.ctypes.data) == EINVAL and b"f 0: a column >= stride" in err()
            assert call("add", f1_selCol=stride) == EINVAL and b"selF 1" in err()
            # a side against ITS OWN rows: a stride whose span passes with nT = 8 rows (below, without a device) but not with the side's 2^28
            assert call("add", f0_stride=(1 << 31), rows=[1 << 28, 40]) == EINVAL and b"f 0: n stride above 2^58" in err()
            assert call("add", f1_stride=(1 << 31), f1_selStride=4, rows=[3, 1 << 28]) == EINVAL and b"f 1: n stride above 2^58" in err()
            # the scratch against the bytes ITS rows touch: f0's 3 rows end before `edge`, 40 rows do not
            edge = f0 + 3 * stride * 8 * words
            assert call("add", work=edge, rows=[40, 40], f1_base=t, f1_sel=None) == EINVAL and b"scratch overlaps" in err()
            assert call("add", work=sel - 16) == EINVAL and b"scratch overlaps" in err(), "reaching the selector's first element"
            for key, v in (("f0_base", f0), ("f1_base", f1), ("f1_sel", sel)):
                assert call("add", **{key: v + 8}) == EINVAL and b"aligned" in err(), key
                assert key == "f1_sel" or call("add", **{key: None}) == EINVAL, key
            assert tuple(rep) == CLEAN
            # write
            assert call("write", m=None) == EINVAL and call("write", m=m + 8) == EINVAL and b"aligned" in err()
            assert call("write", m_col=stride) == EINVAL and call("write", m_stride=1 << 32) == EINVAL and b"m: " in err()
            assert call("write", work=m + 16) == EINVAL and b"scratch overlaps" in err()
            if kind == "lookup":
                assert call("write", m=t, m_col=0) == EINVAL and b"m overlaps" in err(), "a column that is read"
                assert call("write", m=t + 16 * words, m_col=2) == EINVAL and b"m overlaps" in err(), "a foreign base"
                assert call("write", m=t, m_stride=stride + 1) == EINVAL and b"m overlaps" in err(), "another stride"
            else:
                assert call("write", row0=3) == EINVAL and b"row0 + size > n" in err() and call("write", n_m=0, row0=0) == EINVAL
                assert call("write", row0=(1 << 64) - 1) == EINVAL and call("write", n_m=(1 << 28) + 1) == EINVAL and b"nM" in err()
            if not _have_gpu():
                assert call("open") == ENODEV and call("add") == ENODEV and call("write") == ENODEV and call("write", total=None) == ENODEV
                assert call("add", rows=[0, 40], f0_base=None, f0_hostCols=None) == ENODEV, "a side of 0 rows: its pointers are not looked at"
                assert call("add", rows=[64, 1]) == ENODEV and call("add", f1_base=f0, f1_sel=f0) == ENODEV, "one matrix may serve several sides"
                assert call("add", f0_base=f0 + 5 * stride * 8 * words) == ENODEV, "a base advanced by whole rows"
                assert call("add", work=edge, f1_base=t, f1_sel=None) == ENODEV, "the scratch behind the 3 rows f0 has"
                assert call("add", f0_base=work + (1 << 12), f0_stride=1 << 31, rows=[n_t, 40]) == ENODEV, "8 rows of 2^31 elements pass (behind the scratch)"
                assert call("add", f1_sel=None) == ENODEV
                if kind == "lookup":
                    assert call("write", m=t, m_col=3) == ENODEV, "a spare column of t's matrix"
                else:
                    assert call("write", row0=2) == ENODEV and call("write", row0=0, n_m=size) == ENODEV
                    assert call("add", lo=-(1 << 63)) == ENODEV and call("add", lo=(1 << 63) - 1) == ENODEV
        # the debug forms refuse alike
        T = (_lib.TupleSide * 1)(_lib.TupleSide(base=t, stride=stride, hostCols=cols01.ctypes.data, sel=None, selStride=0, selCol=0))
        F = (_lib.TupleSide * 1)(_lib.TupleSide(base=f0, stride=stride, hostCols=col2.ctypes.data, sel=None, selStride=0, selCol=0))
        rows = np.array([3], np.uint64)
        rp = C.c_void_p(rows.ctypes.data)
        assert lib.pil2gl_debug_lookup_session_open_dev(T, n_t, 2, work, 1 << 12, None, 3, 7) == EINVAL and b"elemWords" in err()
        assert lib.pil2gl_debug_lookup_session_open_dev(T, n_t, 2, work, 16, None, words, 7) == EINVAL and b"scratch holds" in err()
        assert lib.pil2gl_debug_range_session_open_dev(0, work, 1 << 12, None, 7) == EINVAL
        assert lib.pil2gl_debug_range_session_add_dev(0, size, F, rp, 1, work, 1 << 12, rep, None, words, 3) == EINVAL and b"path" in err()
        assert lib.pil2gl_debug_range_session_add_dev(0, 8193, F, rp, 1, work, 1 << 20, rep, None, words, 0) == EINVAL and b"8192" in err()
        if not _have_gpu():
            assert lib.pil2gl_debug_lookup_session_open_dev(T, n_t, 2, work, 1 << 12, None, words, 7) == ENODEV
            assert lib.pil2gl_debug_range_session_open_dev(size, work, 1 << 12, None, (1 << 32) - 2) == ENODEV
            for path in (0, 1, 2):
                assert lib.pil2gl_debug_range_session_add_dev(0, size, F, rp, 1, work, 1 << 12, rep, None, words, path) == ENODEV


# ---- the checker ----
def test_checker_agrees_with_the_one_shot_checkers_on_equal_lengths():
    rng = np.random.default_rng(32)
    for q in (P, R):
        n = 40
        t = [[int(v) for v in row] for row in rng.integers(0, 4, (n, 2))]
        fs = [[[int(v) for v in row] for row in rng.integers(0, 5, (n, 2))] for _ in range(3)]
        sel_t = [int(v) for v in rng.integers(0, 2, n)]
        sel_fs = [None, [int(v) for v in rng.integers(0, 2, n)], [q] * 5 + [1] * (n - 5)]
        s = sref.LookupSession(t, q, sel_t)
        rep = s.add(fs, sel_fs)
        assert (s.m(), rep) == lref.multiplicities(fs, t, q, sel_fs, sel_t) and s.total == rep[3] == sum(s.m())
        lo, size, row0 = -3, 7, 2
        fr = [[rref.pattern(int(v), q) for v in rng.integers(-5, 6, n)] for _ in range(2)]
        r = sref.RangeSession(lo, size, q)
        rep = r.add(fr, [sel_fs[1], None])
        assert (r.m(n, row0), rep) == rref.multiplicities(fr, lo, size, n, q, [sel_fs[1], None], row0)
        # cut into adds and sides of other lengths: the same m, the reports each add's own
        r2 = sref.RangeSession(lo, size, q)
        reps = [r2.add([fr[0][:7], fr[0][7:]], [sel_fs[1][:7], sel_fs[1][7:]]), r2.add([fr[1]])]
        assert r2.m(n, row0) == r.m(n, row0) and sum(x[3] for x in reps) == r2.total == rep[3]
        assert sref.RangeSession(0, 2, q, seed=(1 << 32) - 2).m(3, 1) == [0, (1 << 32) - 2, (1 << 32) - 2]
    s = sref.RangeSession(5, 2, P)
    assert s.add([[5, 7, 6], [4]]) == (1, 0, 1, 2) and s.add([[6]]) == (0, NONE, NONE, 1) and s.m(2) == [1, 2] and s.total == 3
    assert sref.element(5, P) == 5 and sref.element((1 << 32) + 3, R) == rref.pattern((1 << 32) + 3, R)
