"""The connection check without a device: the checker (tests/conn_check_ref.py) on the reference-written S of tests/golden/conn_pols.json,
the planner through the ABI and, in a program of its own, under the sanitizers (tests/conn_check_plan_dump.cpp), the refusals of the
compute entries before any device call, ENODEV otherwise, and the exported surface."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

import conn_check_ref as cref
import conn_pols_ref as ref
from conn_pols_ref import P, R
from conftest import ROOT

import pil2gl  # noqa: E402  (a plain import: without the feature, or with a broken build, this file fails)
from pil2gl import _lib, wtns  # noqa: E402

EINVAL, ENODEV = -1, -2
NAMES = ("pil2gl_conn_check_plan", "pil2gl_conn_check_dev", "pil2gl_bn128_conn_check_dev", "pil2gl_conn_check", "pil2gl_bn128_conn_check",
         "pil2gl_debug_conn_check_probe")
GOLDEN = os.path.join(ROOT, "tests", "golden", "conn_pols.json")
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
    for f in ("conn_check_plan", "conn_check", "conn_check_dev"):
        assert callable(getattr(wtns, f))
    assert wtns.conn_check_probe() >= 0


# ---- the checker ----
def golden_cases():
    for c in json.load(open(GOLDEN))["cases"]:
        n_rows, n_cols, N = c["nRows"], c["nCols"], 1 << c["nBits"]
        flat = [c["sMap"][j][i] if i < n_rows else 0 for i in range(N) for j in range(n_cols)]
        S = [int(c["S"][j][i]) for i in range(N) for j in range(n_cols)]
        yield c["name"], flat, S, n_cols, N, int(c["w"]), [1] + [int(k) for k in c["ks"]]


def test_checker_accepts_the_reference_written_golden_with_any_trace_of_the_same_smap():
    seen = 0
    for name, flat, S, n_cols, N, w, ks1 in golden_cases():
        rng = ref.rng(len(flat))
        for _ in range(2):
            wit = [0] + [rng.randrange(P) for _ in range(max(flat))]
            a = [wit[s] for s in flat]
            assert cref.check(a, S, n_cols, N, w, ks1, P) == (cref.NONE, cref.NONE, cref.CLEAN), name
        # one altered cell of a group: the cell itself or the one that points at it, whichever comes first
        groups = {}
        for c, s in enumerate(flat):
            if s:
                groups.setdefault(s, []).append(c)
        big = max(groups.values(), key=len)
        if len(big) >= 3:
            x = big[1]
            a[x] = (a[x] + 1) % P
            cell, to, kind = cref.check(a, S, n_cols, N, w, ks1, P)
            assert (cell, to, kind) == (x, big[0], cref.VALUES_DIFFER), name      # S[big[1]] = id(big[0]); big[2] > big[1] fails later
            seen += 1
    assert seen, "no golden case has a group of three"


def test_checker_kinds_by_hand():
    """2 rows x 2 columns, w = 4 (order 2 in no field: the test only needs distinct ids), ks' = (1, 5): ids 1, 5, 4, 20"""
    w, ks1, q = 4, [1, 5], P
    ident = [1, 5, 4, 20]
    assert cref.check([7, 8, 9, 9], ident, 2, 2, w, ks1, q) == (cref.NONE, cref.NONE, 0)
    swapped = [1, 5, 20, 4]                                                      # cells 2 and 3 connected
    assert cref.check([7, 8, 9, 9], swapped, 2, 2, w, ks1, q) == (cref.NONE, cref.NONE, 0)
    assert cref.check([7, 8, 9, 3], swapped, 2, 2, w, ks1, q) == (2, 3, 2)
    assert cref.check([7, 8, 9, 9], [1, 6, 20, 4], 2, 2, w, ks1, q) == (1, cref.NONE, 1)
    assert cref.check([7, 8, 9 + P, 9], [1 + P, 5, 20, 4], 2, 2, w, ks1, q) == (cref.NONE, cref.NONE, 0)      # words past p count mod p
    assert cref.check([7, 8, 9, 9], ident, 2, 2, w, [1, 4], q) == (2, 1, 3)        # id(1, 0) = 4 = id(0, 1)


# ---- the planner ----
def r16(x):
    return (x + 15) & ~15


SHAPES = ((1, 1, "gl"), (2, 3, "gl"), (16, 1, "gl"), (64, 3, "bn128"), (1024, 12, "gl"), (64, 64, "gl"), (64, 6, "bn128"), (1 << 22, 12, "gl"),
          (1 << 20, 6, "bn128"), (1 << 24, 18, "bn128"), ((1 << 26) // 2, 63, "gl"), (1 << 32, 0, "gl"))


def expected_plan(N, n_cols, words):
    cells = N * n_cols
    cap = 16
    while cap < 2 * cells:
        cap *= 2
    n_bits = N.bit_length() - 1
    lo = (n_bits + 1) // 2
    hi = n_bits - lo
    blocks = lambda items: min(max(-(-items // 256), 1), 2048)                   # noqa: E731
    nbytes = 64 + 4 * cap + r16(8 * words << hi) + r16(8 * words * n_cols << lo) if n_cols else 0
    return {"capBits": cap.bit_length() - 1, "threads": 256, "loBits": lo, "hiBits": hi, "buildBlocks": blocks(cells),
            "checkBlocks": blocks(cells * (2 if words == 4 else 1)), "lanesPerCell": 2 if words == 4 else 1, "launches": 4, "scratchBytes": nbytes}


def test_plan_capacity_geometry_and_scratch():
    for N, n_cols, field in SHAPES:
        words = 1 if field == "gl" else 4
        info = wtns.conn_check_plan(N, n_cols, field)
        assert info == expected_plan(N, n_cols, words), (N, n_cols, field)
        assert info["scratchBytes"] % 16 == 0 and (1 << info["capBits"]) >= 2 * N * n_cols, "load factor at most 1 / 2"


def test_plan_refusals(lib):
    info = (C.c_uint32 * 8)()
    b = C.c_uint64(7)
    for N, n_cols, words, msg in ((1 << 30, 4, 1, b"2^32"), (48, 3, 1, b"power of two"), (0, 3, 1, b"power of two"), (1 << 33, 1, 1, b"power of two"),
                                  (64, 65, 1, b"columns"), (64, 3, 2, b"elemWords")):
        assert lib.pil2gl_conn_check_plan(N, n_cols, words, info, C.byref(b)) == EINVAL and b.value == 0, (N, n_cols, words)
        assert msg in lib.pil2gl_last_error(), lib.pil2gl_last_error()
    assert lib.pil2gl_conn_check_plan((1 << 30) - 0, 3, 4, info, C.byref(b)) == 0 and info[0] == 33       # 3 2^30 cells: 2^33 slots
    assert lib.pil2gl_conn_check_plan(64, 3, 1, None, None) == 0
    with pytest.raises(pil2gl.Pil2glError, match="-1"):
        wtns.conn_check_plan(48, 3)


def test_planner_header_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "conn_check_plan_dump")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                           os.path.join(ROOT, "tests", "conn_check_plan_dump.cpp"), "-o", exe])
    refused = [(1 << 30, 4, 1), (48, 3, 1), (0, 1, 1), (1 << 33, 1, 4), (64, 65, 1), (64, 3, 3), ((1 << 32), 1, 1)]
    columns = [((3, 0, 3), 1), ((2, 0, 3), 0), ((5, 2, 3), 1), ((4, 2, 3), 0), ((4, 5, 0), 0), ((1 << 32, 0, 1), 0), ((0, 0, 0), 1)]
    spans = [((4, 3, 3, 0, 1), 96), ((4, 3, 8, 2, 4), (3 * 8 + 2 + 3) * 32), ((0, 3, 3, 0, 1), 0), ((4, 0, 3, 0, 1), 0), ((1, 1, 1, 0, 4), 32)]
    with open(tmp_path / "cmds.txt", "w") as f:
        for N, n_cols, field in SHAPES:
            f.write("plan %d %d %d\n" % (N, n_cols, 1 if field == "gl" else 4))
        f.write("".join("plan %d %d %d\n" % r for r in refused) + "".join("columns %d %d %d\n" % c for c, _ in columns))
        f.write("".join("span %d %d %d %d %d\n" % s for s, _ in spans))
    run = subprocess.run([exe, str(tmp_path / "cmds.txt")], capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", "sanitizer report:\n" + run.stderr[-4000:]
    out = [json.loads(l) for l in run.stdout.splitlines()]
    assert len(out) == len(SHAPES) + len(refused) + len(columns) + len(spans)
    for (N, n_cols, field), got in zip(SHAPES, out):
        words = 1 if field == "gl" else 4
        want = expected_plan(N, n_cols, words)
        assert got["ok"] == 1 and got["cells"] == N * n_cols and got["capacity"] == 1 << want["capBits"], (N, n_cols, field)
        assert {k: got[k] for k in ("capBits", "loBits", "hiBits", "lanesPerCell", "buildBlocks", "checkBlocks")} == \
               {k: want[k] for k in ("capBits", "loBits", "hiBits", "lanesPerCell", "buildBlocks", "checkBlocks")}
        assert got["bytes"] == want["scratchBytes"]
        parts = [got["offHeader"], got["offTable"], got["offHi"], got["offLo"]]
        assert parts == sorted(parts) and all(p % 16 == 0 for p in parts) and parts[:2] == [0, 64], "every part on 16 bytes, header first"
        assert got["offHi"] - got["offTable"] == 4 * got["capacity"]
        if n_cols:
            assert got["offLo"] - got["offHi"] >= 8 * words << want["hiBits"] and got["bytes"] - got["offLo"] >= 8 * words * n_cols << want["loBits"]
            assert got["tableElems"] == (n_cols << want["loBits"]) + (1 << want["hiBits"])
    at = len(SHAPES)
    assert all(g["ok"] == 0 and g["why"] for g in out[at:at + len(refused)])
    at += len(refused)
    assert [g["ok"] for g in out[at:at + len(columns)]] == [ok for _, ok in columns]
    assert [g["bytes"] for g in out[at + len(columns):]] == [b for _, b in spans]


# ---- the compute entries ----
def test_compute_entries_refuse_before_any_device_call(lib):
    buf = np.zeros(8192, np.uint64)
    base = buf.ctypes.data + (-buf.ctypes.data % 16)
    w = np.array([3, 0, 0, 0], np.uint64)
    ks = np.arange(1, 4 * 65 + 1, dtype=np.uint64)
    pw, pk = w.ctypes.data, ks.ctypes.data
    rep = (C.c_uint64 * 3)(5, 5, 5)
    for fn, field, words in ((lib.pil2gl_conn_check_dev, "gl", 1), (lib.pil2gl_bn128_conn_check_dev, "bn128", 4)):
        need = wtns.conn_check_plan(8, 3, field)["scratchBytes"]
        a, S, work = base, base + 8 * 3 * 8 * words, base + 16384
        assert work + need <= buf.ctypes.data + buf.nbytes
        ok = [a, 3, 0, S, 3, 0, 8, 3, pw, pk, work, need, rep, None]

        def call(**kw):
            args = list(ok)
            for k, v in kw.items():
                args[int(k[1:])] = v
            rep[0] = rep[1] = rep[2] = 5
            return fn(*args)
        assert call(a1=2) == EINVAL and b"a: stride" in lib.pil2gl_last_error()                # aStride < nCols
        assert tuple(rep) == (cref.NONE, cref.NONE, 0), "a refused call leaves a clean report"
        assert call(a4=4, a5=2) == EINVAL and b"S: stride" in lib.pil2gl_last_error()          # sStride < sOffset + nCols
        assert call(a1=1 << 32) == EINVAL and b"stride" in lib.pil2gl_last_error()
        assert call(a11=need - 16) == EINVAL and b"scratch" in lib.pil2gl_last_error()         # short
        assert call(a10=work + 8) == EINVAL and b"aligned" in lib.pil2gl_last_error()
        assert call(a10=a + 16) == EINVAL and b"overlaps" in lib.pil2gl_last_error()           # the scratch inside a
        assert call(a10=S - 16) == EINVAL and b"overlaps" in lib.pil2gl_last_error()           # the scratch reaching into S
        assert call(a0=a + 4) == EINVAL and b"aligned" in lib.pil2gl_last_error()
        for k in (0, 3, 8, 9, 10, 12):
            assert call(**{"a%d" % k: None}) == EINVAL, k
        assert call(a7=65, a1=65, a4=65) == EINVAL and b"columns" in lib.pil2gl_last_error()
        assert call(a6=48) == EINVAL and b"power of two" in lib.pil2gl_last_error()
        assert call(a7=0, a1=0, a4=0) == 0 and tuple(rep) == (cref.NONE, cref.NONE, 0)         # no columns: clean, no device
        if not _have_gpu():
            assert call() == ENODEV
            assert call(a3=a, a1=8, a4=8, a5=4, a6=4) == ENODEV                                # a and S in one matrix: nothing to refuse
    host = np.zeros(8 * 3 * 4, np.uint64)
    p = host.ctypes.data
    for fn in (lib.pil2gl_conn_check, lib.pil2gl_bn128_conn_check):
        assert fn(p, p, 48, 3, pw, pk, rep) == EINVAL and b"power of two" in lib.pil2gl_last_error()
        assert fn(p, p, 8, 65, pw, pk, rep) == EINVAL
        for k in (0, 1, 4, 5, 6):
            args = [p, p, 8, 3, pw, pk, rep]
            args[k] = None
            assert fn(*args) == EINVAL, k
        rep[2] = 5
        assert fn(p, p, 8, 0, pw, pk, rep) == 0 and tuple(rep) == (cref.NONE, cref.NONE, 0)
        if not _have_gpu():
            assert fn(p, p, 8, 3, pw, pk, rep) == ENODEV
    if not _have_gpu():
        with pytest.raises(pil2gl.Pil2glError, match="-2"):
            wtns.conn_check(host[:24], host[:24], 3, 8, [3], [5, 6])
        with pytest.raises(pil2gl.Pil2glError, match="-2"):
            wtns.conn_check(host, host, 3, 8, *ref.consts(3, [5, 6], R), field="bn128")
    with pytest.raises(pil2gl.Pil2glError, match="nCols - 1"):
        wtns.conn_check(host[:24], host[:24], 3, 8, [3], [5, 6, 7])
    with pytest.raises(pil2gl.Pil2glError, match="words"):
        wtns.conn_check(host[:23], host[:24], 3, 8, [3], [5, 6])
