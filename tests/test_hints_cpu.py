"""The Goldilocks stage-2 hints without a device: the plan (csrc/hint_plan.h) through the ABI and, in a program of its own, under the
sanitizers (tests/hint_plan_dump.cpp), both against the restatement in tests/hints_ref.py; the key hash of h1h2 likewise; the restated
field arithmetic of hints_ref.py against the C oracle, so that the GPU tests' two references are known to agree before either is used."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

import hints_ref as href
from conftest import ROOT, P, rand_field

import pil2gl  # noqa: E402  (a plain import: without the feature, or with a broken build, this file fails)
from pil2gl import _lib  # noqa: E402

NONE = (1 << 64) - 1
CSRC = os.path.join(ROOT, "pil2-stark-js_amd", "csrc")
NAMES = ("pil2gl_debug_hint_plan", "pil2gl_debug_h1h2_home")


def first_n_with(per):
    """the smallest n whose second pass walks `per` totals a lane: one row into block (per - 1) THREADS + 1"""
    return (per - 1) * href.THREADS * href.CHUNK + 1


# the first n at which totals_per_lane becomes 1, 2 and 3 with their predecessors, the lane and block edges, 0, 1 and 2^30
SHAPES = (0, 1, 2, 7, 8, 9, 2047, 2048, 2049, 4096, 4097, 300001, first_n_with(2) - 1, first_n_with(2), first_n_with(3) - 1, first_n_with(3),
          1 << 28, 1 << 30, (1 << 30) + 1)
KEYS = [(1, [0]), (1, [1]), (1, [P - 1]), (1, [1 << 32]), (1, [(1 << 32) - 1]), (3, [0, 0, 0]), (3, [1, 0, 0]), (3, [0, 1, 0]), (3, [0, 0, 1]),
        (3, [P - 1, P - 1, P - 1]), (3, [1 << 63, 5, 1 << 32]), (3, [7, 5, 9]), (3, [7 + (1 << 40), 5, 9]), (3, [7, 5, 8])]


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_entries_are_declared_bound_and_exported(lib):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pil2gl.h")).read(), flags=re.S)
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, header), n + " is not declared in pil2gl.h"
        assert n in _lib.SIGNATURES, n + " is not bound in _lib.py"
        assert getattr(lib, n)
    assert callable(pil2gl.hint_plan) and callable(pil2gl.h1h2_home)


def test_plan_thresholds():
    assert first_n_with(2) == 256 * 2048 + 1 and first_n_with(3) == 512 * 2048 + 1
    for n in SHAPES:
        assert pil2gl.hint_plan(n) == href.plan(n), n
    assert [pil2gl.hint_plan(n)["totalsPerLane"] for n in (0, 1, first_n_with(2) - 1, first_n_with(2), first_n_with(3) - 1, first_n_with(3))] == [0, 1, 1, 2, 2, 3]
    assert [pil2gl.hint_plan(n)["blocks"] for n in (0, 1, 2048, 2049, 1 << 30)] == [0, 1, 1, 2, 1 << 19]
    assert [pil2gl.hint_plan(n)["h1h2CapBits"] for n in (0, 1, 2, 8, 9, 1 << 30, (1 << 30) + 1)] == [1, 1, 2, 4, 5, 31, 0], "n = 8 fills half of 16 slots"
    assert pil2gl.hint_plan(1 << 30)["totalsPerLane"] == 2048
    p = pil2gl.hint_plan(12345)
    assert p["chunk"] == p["threads"] * p["items"]


def test_plan_refusals(lib):
    info = (C.c_uint32 * 6)()
    assert lib.pil2gl_debug_hint_plan(2048 * ((1 << 31) - 1), info) == 0 and info[3] == (1 << 31) - 1 and info[5] == 0
    assert lib.pil2gl_debug_hint_plan(2048 * ((1 << 31) - 1) + 1, info) == -1 and b"grid too large" in lib.pil2gl_last_error()
    assert lib.pil2gl_debug_hint_plan(NONE, info) == -1
    assert lib.pil2gl_debug_hint_plan(64, None) == 0
    with pytest.raises(pil2gl.Pil2glError, match="-1"):
        pil2gl.hint_plan(1 << 63)


def test_h1h2_home_is_the_restated_hash(lib):
    rng = np.random.default_rng(5)
    for dim in (1, 3):
        keys = [rand_field(rng, dim) for _ in range(200)] + [np.array(w, np.uint64) for d, w in KEYS if d == dim]
        for cap in (2, 16, 1 << 20, 1 << 31):
            seen = set()
            for w in keys:
                h = pil2gl.h1h2_home(w, dim, cap)
                assert h == href.home(w, cap) and 0 <= h < cap
                seen.add(h)
            assert cap < 16 or len(seen) > 8, "the slots spread"
    one = np.array([7, 5, 9], np.uint64)
    assert pil2gl.h1h2_home(one, 3, 1 << 31) != pil2gl.h1h2_home(one[::-1].copy(), 3, 1 << 31), "(a, b, c) is not (c, b, a)"
    assert pil2gl.h1h2_home(one[:1], 1, 1 << 31) != pil2gl.h1h2_home(one, 3, 1 << 31)
    for dim, cap, words in ((1, 48, one.ctypes.data), (1, 0, one.ctypes.data), (2, 16, one.ctypes.data), (0, 16, one.ctypes.data), (3, 16, None)):
        assert lib.pil2gl_debug_h1h2_home(words, dim, cap) == NONE, (dim, cap)
    with pytest.raises(pil2gl.Pil2glError):
        pil2gl.h1h2_home(one, 1, 16)
    with pytest.raises(pil2gl.Pil2glError):
        pil2gl.h1h2_home(one, 3, 24)


def test_plan_and_hash_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "hint_plan_dump")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                           os.path.join(ROOT, "tests", "hint_plan_dump.cpp"), "-o", exe])
    caps = (2, 16, 1 << 31)
    with open(tmp_path / "cmds.txt", "w") as f:
        f.write("".join("plan %d\n" % n for n in SHAPES))
        f.write("".join("home %d %d %s\n" % (dim, cap, " ".join(map(str, w))) for dim, w in KEYS for cap in caps))
    run = subprocess.run([exe, str(tmp_path / "cmds.txt")], capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", "sanitizer report:\n" + run.stderr[-4000:]
    out = [json.loads(line) for line in run.stdout.splitlines()]
    assert len(out) == len(SHAPES) + len(KEYS) * len(caps)
    for n, got in zip(SHAPES, out):
        want = href.plan(n)
        assert (got["threads"], got["items"], got["chunk"], got["blocks"], got["totalsPerLane"], got["capBits"]) == tuple(want[k] for k in pil2gl.HINT_PLAN), n
        lib_plan = pil2gl.hint_plan(n)
        assert got["capBits"] == lib_plan.pop("h1h2CapBits") and all(got[k] == v for k, v in lib_plan.items()), "the program and the library share the header"
        if n <= 1 << 30:
            cap = got["capacity"]
            assert cap == 1 << want["h1h2CapBits"] and cap >= max(2 * n, 2) and (cap == 2 or cap < 4 * n), "the smallest power of two"
            # table[capacity] | cnt[n] | start[n] | totals[blocks] | missing[1]
            assert [got[k] for k in ("offTable", "offCnt", "offStart", "offTotals", "offMissing", "words")] == \
                [0, cap, cap + n, cap + 2 * n, cap + 2 * n + want["blocks"], cap + 2 * n + want["blocks"] + 1]
        else:
            assert got["capacity"] == 0 and got["words"] == 0
    at = len(SHAPES)
    for i, (dim, w) in enumerate(KEYS):
        for j, cap in enumerate(caps):
            got = out[at + i * len(caps) + j]
            assert got["hash"] == href.key_hash(w) and got["home"] == href.home(w, cap) == pil2gl.h1h2_home(np.array(w, np.uint64), dim, cap)
    bad = tmp_path / "bad.txt"
    bad.write_text("home 2 16 1 2\n")
    assert subprocess.run([exe, str(bad)], capture_output=True).returncode == 2


# ---- the restated arithmetic against the C oracle ----
EDGE = [1, 2, P - 1, P - 2, (1 << 32) - 1, 1 << 32, (1 << 32) + 1, P - (1 << 32), 1 << 63]


def test_restated_extension_field_agrees_with_the_oracle(oracle):
    rng = np.random.default_rng(11)
    elems = [tuple(int(x) for x in rand_field(rng, 3)) for _ in range(40)]
    elems += [(v, 0, 0) for v in EDGE] + [(0, v, 0) for v in EDGE] + [(0, 0, v) for v in EDGE] + [(EDGE[k], EDGE[(k + 1) % 9], EDGE[(k + 2) % 9]) for k in range(9)]
    for a, b in zip(elems, elems[1:] + elems[:1]):
        assert href.mul3(a, b) == tuple(int(x) for x in oracle.mul3(a, b))
        ai = href.inv3(a)
        assert ai == tuple(int(x) for x in oracle.inv3(a)) and href.mul3(a, ai) == (1, 0, 0)
    assert href.inv3((0, 0, 0)) == (0, 0, 0)
    assert href.mul3((0, 1, 0), (0, 0, 1)) == (1, 1, 0) and href.mul3((0, 0, 1), (0, 0, 1)) == (0, 1, 1), "x^3 = x + 1, x^4 = x^2 + x"


@pytest.mark.parametrize("dim_num,dim_den", [(1, 1), (1, 3), (3, 1), (3, 3)])
def test_restated_columns_agree_with_the_oracle(oracle, dim_num, dim_den):
    rng = np.random.default_rng(dim_num * 3 + dim_den)
    n = 37
    num, den = rand_field(rng, (n, dim_num)), rand_field(rng, (n, dim_den))
    den[5] = 0; den[36] = 0
    if dim_den == 3:
        den[9] = (0, 7, 0); den[10] = (0, 0, 7); den[11] = (7, 0, 0)
    assert href.gprod(num, dim_num, den, dim_den) == oracle.gprod(num, den, dim_num, dim_den).tolist()
    assert href.gsum(num[:1], dim_num, den, dim_den) == oracle.gsum(num[:1], den, dim_num, dim_den).tolist()


def test_restated_h1h2_agrees_with_the_oracle(oracle):
    t = [5, 7, 5, 9, 7, 11]
    f = [5, 5, 7, 11, 5, 7]
    assert href.h1h2(f, t) == oracle.h1h2(f, t) == ([5, 5, 5, 9, 7, 11], [7, 5, 5, 7, 7, 11])
    with pytest.raises(ValueError, match="w:1$"):
        href.h1h2([5, 6, 8], t[:3])
