"""The range-check grand sum without a device: the exported surface, the plan's numbers against logup_sum's, the layout of
pil2gl_range_term against the header and the addon, the checker (tests/range_sum_ref.py) against logup_sum_ref on materialised columns and
its own identity (s[i] - s[i-1]) prod D = N, the refusals of the compute entries before any device call, ENODEV otherwise, and the planner
with the aliasing rule in a program of its own under the sanitizers (tests/range_sum_plan_dump.cpp)."""
import ctypes as C
import json
import os
import random
import re
import shutil
import subprocess

import numpy as np
import pytest

import logup_sum_ref as lref
import range_sum_ref as rref
from hints_ref import P
from conftest import ROOT

import pil2gl  # noqa: E402  (a plain import: without the feature, or with a broken build, this file fails)
from pil2gl import _lib, pilcheck  # noqa: E402

EINVAL, ENODEV = -1, -2
NAMES = ("pil2gl_range_sum_plan", "pil2gl_range_sum_dev", "pil2gl_bn128_range_sum_dev", "pil2gl_range_sum", "pil2gl_bn128_range_sum")
CSRC = os.path.join(ROOT, "pil2-stark-js_amd", "csrc")
SHAPES = (0, 1, 8, 9, 2048, 2049, 2048 * 256 + 1, 64, 65, 1024, 1025, 16385, 262145, 1 << 28)
NODE = shutil.which("node")
LAYOUT = ("size", "m", "mStride", "mCol", "lo", "rangeSize", "row0", "coef", "busId")


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _have_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


def _layout():
    T = _lib.RangeTerm
    return dict(size=C.sizeof(T), m=T.m.offset, mStride=T.mStride.offset, mCol=T.mCol.offset, lo=T.lo.offset, rangeSize=T.size.offset, row0=T.row0.offset,
                coef=T.coef.offset, busId=T.busId.offset)


def test_entries_are_declared_bound_and_exported(lib):
    full = open(os.path.join(ROOT, "include", "pil2gl.h")).read()
    header = re.sub(r"/\*.*?\*/", "", full, flags=re.S)
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, header), n + " is not declared in pil2gl.h"
        assert n in _lib.SIGNATURES, n + " is not bound in _lib.py"
        assert getattr(lib, n)
    assert "pil2gl_range_term" in header
    for f in ("range_sum_plan", "range_sum", "range_sum_dev", "range_logup"):
        assert callable(getattr(pilcheck, f))
    listed = full[full.index("only ENQUEUE work on that stream"):full.index("dev_upload_async / dev_download_async")]
    assert "range_sum and bn128_range_sum" in listed, "the header's list of enqueue-only calls"
    assert "range_sum_plan" in full[full.index("Calls that need no device"):full.index("Calls are not thread-safe")]
    src = open(os.path.join(ROOT, "pil2-stark-js_amd", "js", "pil_checks.js")).read()
    assert re.search(r"module\.exports = \{[^}]*rangeSum, rangeSumDev, rangeSumPlan", src)
    for f in ("polutils.js", "polutils_bn128.js"):
        src = open(os.path.join(ROOT, "pil2-stark-js_amd", "js", f)).read()
        assert "calculateSRange" in src and "calculateSRangeDev" in src, f


def test_plan_values_are_logup_sums(lib):
    for n in SHAPES:
        for field in ("gl", "bn128"):
            want, nbytes = rref.plan(n, 0, 1, field)
            logup = pilcheck.logup_sum_plan(n, 1, field)
            for n_f, n_r in ((0, 1), (0, 8), (1, 8), (8, 1), (4, 5)):
                got = pilcheck.range_sum_plan(n, n_f, n_r, field)
                assert got == logup, "logup_sum_plan's values for the same n"
                assert (got["threads"], got["items"], got["blocks"], got["launches"], got["depth"], got["outWidth"]) == want, (n, field)
                assert got["workBytes"] == nbytes, "the working memory grows with neither nF nor nR"
    info = (C.c_uint32 * 6)()
    b = C.c_uint64(7)
    bad = (((1 << 28) + 1, 0, 1, 1, b"2^28"), (8, 0, 0, 1, b"1 .. 8"), (8, 0, 9, 1, b"1 .. 8"), (8, 9, 1, 4, b"at most 8"), (8, 2, 8, 1, b"at most 9"),
           (8, 8, 2, 4, b"at most 9"), (8, 0, 1, 3, b"elemWords"), (8, 0, 1, 0, b"elemWords"))
    for n, n_f, n_r, words, msg in bad:
        assert lib.pil2gl_range_sum_plan(n, n_f, n_r, words, info, C.byref(b)) == EINVAL and msg in lib.pil2gl_last_error(), (n, n_f, n_r, words)
        assert b.value == 0
    assert lib.pil2gl_range_sum_plan(8, 8, 1, 1, info, C.byref(b)) == 0 and lib.pil2gl_range_sum_plan(8, 1, 8, 4, info, C.byref(b)) == 0


def test_term_layout_matches_the_header(tmp_path):
    exe = str(tmp_path / "dump")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", CSRC, os.path.join(ROOT, "tests", "range_sum_plan_dump.cpp"), "-o", exe])
    (tmp_path / "c.txt").write_text("layout\n")
    got = json.loads(subprocess.run([exe, str(tmp_path / "c.txt")], capture_output=True, text=True, check=True).stdout)
    assert got == _layout()
    assert tuple(got[k] for k in LAYOUT) == (112, 0, 8, 16, 24, 32, 40, 48, 80)


@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_term_layout_matches_what_the_addon_states():
    """the ctypes struct against sizeof / offsetof as the ADDON was compiled (a fresh Node child; no device needed), and the addon's surface"""
    js = "const a = require(%r).addon; console.log(JSON.stringify([a.rangeTermLayout()].concat(['rangeSumPlan', 'rangeSumDev', 'rangeSum'].map((f) => typeof a[f])).concat([a.rangeSumPlan(2049, 0, 8, 1)])));"
    out = subprocess.run([NODE, "-e", js % os.path.join(ROOT, "pil2-stark-js_amd", "js", "native.js")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    got = json.loads(out.stdout)
    assert got[0] == _layout()
    assert got[1:4] == ["function"] * 3
    assert got[4] == pilcheck.range_sum_plan(2049, 0, 8, "gl")


def _rand_ext(rng, field):
    return tuple(rng.randrange(P) for _ in range(3)) if field == "gl" else rng.randrange(lref.FIELDS[field].q)


def _neg(field, a):
    q = lref.FIELDS[field].q
    return tuple((q - x) % q for x in a) if field == "gl" else (q - a) % q


def _rand_case(rng, field, n, n_f, windows):
    """n_f random f terms and one range per (lo, size, row0); m is None outside its window"""
    q = lref.FIELDS[field].q
    terms = []
    for u in range(n_f):
        k = (1, 3, 16)[u % 3]
        terms.append(([[rng.randrange(q) for _ in range(k)] for _ in range(n)], [rng.randrange(4) for _ in range(n)] if u % 2 else None, rng.choice((1, q - 1, 5)), rng.randrange(q)))
    ranges = []
    for lo, size, row0 in windows:
        m = [rng.choice((0, 1, 2, rng.randrange(q))) if row0 <= i < row0 + size else None for i in range(n)]
        ranges.append((m, lo, size, row0, rng.choice((q - 1, 1, 5)), rng.randrange(q)))
    return terms, ranges


@pytest.mark.parametrize("field", ["gl", "bn128"])
def test_reference_equals_logup_sum_ref_on_materialised_columns(field):
    """the statement's promise, over integers: a self-check of the CHECKER, which runs no library code"""
    rng = random.Random(31)
    n = 40
    for n_f, windows in ((0, [(0, n, 0)]), (0, [(-3, 8, 5)]), (2, [(-(1 << 63), 7, 33), ((1 << 63) - 9, 9, 0)]), (1, [(5, 1, 0), (5, 1, n - 1), (1 << 32, 20, 10), (7, 20, 15)]),
                         (8, [((1 << 32) - 2, 17, 3)]), (1, [(i, 3 + i, 2 * i) for i in range(8)])):
        terms, ranges = _rand_case(rng, field, n, n_f, windows)
        alpha, beta = _rand_ext(rng, field), _rand_ext(rng, field)
        want = lref.logup_sum(field, terms + rref.materialise(field, ranges, n), alpha, beta, n)
        assert rref.range_sum(field, terms, ranges, alpha, beta, n) == want
    # the field value of the range: lo signed, reduced mod the modulus
    q = lref.FIELDS[field].q
    t = rref.materialise(field, [([1] * 6, -2, 4, 1, 1, 0)], 6)[0]
    assert [r[0] for r in t[0]] == [q - 2, q - 2, q - 1, 0, 1, 1] and t[1] == [0, 1, 1, 1, 1, 0]


@pytest.mark.parametrize("field", ["gl", "bn128"])
def test_checker_identity(field):
    """(s[i] - s[i-1]) prod D = N with the products over the non-zero denominators, and a forced zero E adds nothing while the rows around
    it and the other terms of its row still count.  A self-check of the CHECKER only."""
    rng = random.Random(37)
    F = lref.FIELDS[field]
    n = 24
    terms, ranges = _rand_case(rng, field, n, 2, [(-3, 8, 4), (100, 10, 8)])
    alpha = _rand_ext(rng, field)
    hit = 9                                            # inside both windows
    beta = _neg(field, rref.range_denominator(F, ranges[0], F.ext(alpha), F.zero, hit))
    assert rref.range_denominator(F, ranges[0], F.ext(alpha), F.ext(beta), hit) == F.zero
    s = rref.range_sum(field, terms, ranges, alpha, beta, n)
    prev = F.zero
    for i in range(n):
        N, D, ratio = rref.row_fraction(F, terms, ranges, F.ext(alpha), F.ext(beta), i)
        step = F.add(s[i], _neg(field, prev))
        assert step == ratio and F.mul(step, D) == N and D != F.zero
        prev = s[i]
    assert rref.row_fraction(F, terms, ranges, F.ext(alpha), F.ext(beta), hit)[2] == rref.row_fraction(F, terms, ranges[1:], F.ext(alpha), F.ext(beta), hit)[2]
    assert rref.row_fraction(F, terms, ranges, F.ext(alpha), F.ext(beta), 3)[2] == rref.row_fraction(F, terms, [], F.ext(alpha), F.ext(beta), 3)[2], "outside every window"


def test_planner_and_aliasing_rule_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "range_sum_plan_dump")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                           os.path.join(ROOT, "tests", "range_sum_plan_dump.cpp"), "-o", exe])
    shapes = [(0, 1, 1), (0, 8, 4), (8, 1, 1), (1, 8, 4)]
    refused = [((1 << 28) + 1, 0, 1, 1), (8, 0, 0, 1), (8, 0, 9, 1), (8, 9, 1, 1), (8, 2, 8, 4), (8, 0, 1, 3), ((1 << 64) - 1, (1 << 64) - 1, 1, 4)]
    B = 1 << 40                                       # a byte address; never dereferenced
    big = 1 << 30                                     # 2^28 rows of 2^30 elements: n stride = 2^58, the largest that passes
    u64 = lambda v: v & ((1 << 64) - 1)               # noqa: E731
    calls = [  # (n, words, oBase, oStride, oCol, mBase, mStride, mCol, lo, size, row0) -> ok, a word of the message
        ((8, 1, B, 8, 1, B, 8, 0, 0, 8, 0), 1, ""),                              # out as three spare word columns of m's matrix
        ((8, 1, B, 8, 5, B, 8, 4, 0, 8, 0), 1, ""),
        ((8, 1, B, 8, 0, B, 8, 0, 0, 8, 0), 0, "out overlaps"),                  # out on the m column: its first word
        ((8, 1, B, 8, 2, B, 8, 3, 0, 8, 0), 0, "out overlaps"),                  # its second
        ((8, 1, B, 8, 2, B, 8, 4, 0, 8, 0), 0, "out overlaps"),                  # its third
        ((8, 1, B, 8, 2, B, 8, 4, 0, 1, 0), 0, "out overlaps"),                  # a window of one row: the column counts over all n rows
        ((8, 4, B, 4, 1, B, 4, 3, 0, 8, 0), 1, ""), ((8, 4, B, 4, 3, B, 4, 3, 0, 8, 0), 0, "out overlaps"),    # Fr: one element column
        ((8, 1, B, 8, 5, B, 9, 0, 0, 8, 0), 0, "out overlaps"),                  # the same base, another stride
        ((8, 1, B + 16, 8, 1, B, 8, 0, 0, 8, 0), 0, "out overlaps"),             # the same stride, another base
        ((8, 1, B + 8 * 57, 8, 0, B, 8, 0, 0, 8, 0), 0, "aligned"),              # an odd word: misaligned out
        ((8, 1, B + 8 * 58, 8, 0, B, 8, 0, 0, 8, 0), 1, ""),                     # m ends with element (7, 0) at word 56: behind it is free
        ((8, 1, B + 8 * 56, 8, 0, B, 8, 0, 0, 8, 0), 0, "out overlaps"),
        ((8, 1, B, 8, 0, B + 8, 8, 0, 0, 8, 0), 0, "aligned"),                   # a misaligned m
        ((8, 1, B, 8, 0, 0, 8, 0, 0, 8, 0), 0, "null"), ((8, 1, 0, 8, 0, B, 8, 3, 0, 8, 0), 0, "null"),
        ((8, 1, B, 8, 6, B + 4096, 8, 0, 0, 8, 0), 0, "out: a column >= stride"),
        ((8, 1, B, 8, 0, B + 4096, 8, 8, 0, 8, 0), 0, "m: a column >= stride"), ((8, 1, B, 8, 0, B + 4096, 1 << 32, 0, 0, 8, 0), 0, "stride >= 2^32"),
        ((8, 1, B, 8, 0, B + 4096, (1 << 32) - 1, (1 << 32) - 2, 0, 8, 0), 1, ""),    # the widest stride, its last column
        ((8, 1, B, (1 << 32) - 1, (1 << 32) - 4, B, (1 << 32) - 1, (1 << 32) - 5, 0, 8, 0), 1, ""),
        ((8, 1, B, (1 << 32) - 1, (1 << 32) - 4, B, (1 << 32) - 1, (1 << 32) - 2, 0, 8, 0), 0, "out overlaps"),
        ((1 << 28, 4, B, big, big - 1, B, big, big - 2, 0, 1 << 28, 0), 1, ""),  # the 2^58 limit: spans of 2^63 bytes, no overflow
        ((1 << 28, 4, B, big, big - 1, B, big, big - 1, 0, 1 << 28, 0), 0, "out overlaps"),
        ((1 << 28, 1, B, big, big - 3, B, big, big - 4, 0, 1 << 28, 0), 1, ""),
        ((1 << 28, 1, B, big, big - 3, B, big, big - 2, 0, 1 << 28, 0), 0, "out overlaps"),
        ((1 << 28, 4, B, big, 0, B + (1 << 62), big, 0, 0, 1, 0), 0, "out overlaps"),        # a foreign base inside that span
        ((1 << 28, 1, B, 8, 0, B + (1 << 40), big + 1, 0, 0, 1, 0), 0, "2^58"),
        ((8, 1, B, 8, 1, B, 8, 0, 0, 0, 0), 0, "size must be"), ((1 << 28, 1, B, 8, 1, B, 8, 0, 0, (1 << 28) + 1, 0), 0, "size must be"),
        ((8, 1, B, 8, 1, B, 8, 0, 0, 9, 0), 0, "row0 + size > n"), ((8, 1, B, 8, 1, B, 8, 0, 0, 8, 1), 0, "row0 + size > n"),
        ((8, 1, B, 8, 1, B, 8, 0, 0, 1, 8), 0, "row0 + size > n"), ((8, 1, B, 8, 1, B, 8, 0, 0, 2, (1 << 64) - 1), 0, "row0 + size > n"),
        ((8, 1, B, 8, 1, B, 8, 0, u64(-(1 << 63)), 1, 7), 1, ""), ((8, 1, B, 8, 1, B, 8, 0, (1 << 63) - 1, 8, 0), 1, ""),
        ((0, 1, 0, 8, 1, 0, 8, 0, 0, 9, 5), 1, ""),                              # no rows: no window check, no pointer is looked at
        ((0, 1, 0, 8, 1, 0, 8, 8, 0, 1, 0), 0, "m: a column >= stride"),
    ]
    c0 = [(lo, bus, [rng_ for rng_ in a], [x for x in b]) for lo, bus, a, b in
          ((0, 0, (1, 2, 3), (4, 5, 6)), (-3, 7, (P - 1, 0, 5), (P - 1, P - 1, 0)), (-(1 << 63), P - 1, (P - 1, P - 2, 1), (9, 8, 7)), ((1 << 63) - 1, 5, (3, P - 1, 2), (0, 0, 0)))]
    stage = [(1, 8, 3, 5, 2, (6 * 8 + 3 + 1)), (4, 4, 3, 1, 0, (0 * 4 + 3 + 1) * 4), (1, 1, 0, 1 << 28, 0, 1 << 28)]
    with open(tmp_path / "cmds.txt", "w") as f:
        f.write("".join("plan %d %d %d %d\n" % (n, nf, nr, w) for n in SHAPES for nf, nr, w in shapes))
        f.write("".join("plan %d %d %d %d\n" % r for r in refused))
        f.write("".join("call " + " ".join(map(str, c)) + "\n" for c, _, _ in calls))
        f.write("".join("c0 %d %d %s %s\n" % (u64(lo), bus, " ".join(map(str, a)), " ".join(map(str, b))) for lo, bus, a, b in c0))
        f.write("".join("words %d %d %d %d %d\n" % s[:5] for s in stage))
        f.write("layout\n")
    run = subprocess.run([exe, str(tmp_path / "cmds.txt")], capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", "sanitizer report:\n" + run.stderr[-4000:]
    out = [json.loads(line) for line in run.stdout.splitlines()]
    assert len(out) == len(shapes) * len(SHAPES) + len(refused) + len(calls) + len(c0) + len(stage) + 1
    for i, got in enumerate(out[:len(shapes) * len(SHAPES)]):
        nf, nr, w = shapes[i % len(shapes)]
        want, nbytes = rref.plan(SHAPES[i // len(shapes)], nf, nr, "gl" if w == 1 else "bn128")
        assert got["ok"] == 1 and (got["threads"], got["items"], got["blocks"], got["launches"], got["depth"], got["width"]) == want
        assert got["bytes"] == nbytes
    at = len(shapes) * len(SHAPES)
    assert all(g["ok"] == 0 and g["why"] for g in out[at:at + len(refused)])
    at += len(refused)
    for got, (c, ok, word) in zip(out[at:], calls):
        assert got["ok"] == ok and word in got["why"], (c, got)
    at += len(calls)
    for got, (lo, bus, a, b) in zip(out[at:], c0):
        assert got["c0"] == [(a[0] * (lo % P) + b[0] + bus) % P, (a[1] * (lo % P) + b[1]) % P, (a[2] * (lo % P) + b[2]) % P]
    at += len(c0)
    assert [g["words"] for g in out[at:-1]] == [s[5] for s in stage]
    assert out[-1] == _layout()


def test_compute_entries_refuse_before_any_device_call(lib):
    buf = np.zeros(16384, np.uint64)
    base = buf.ctypes.data + (-buf.ctypes.data % 16)
    cols = np.array([2, 0, 1] + [0] * 14, np.uint64)
    bad_cols = np.array([2, 8, 1], np.uint64)
    n, stride = 8, 8
    ch = np.array([3, 4, 5, 6], np.uint64)
    for dev, host, words in ((lib.pil2gl_range_sum_dev, lib.pil2gl_range_sum, 1), (lib.pil2gl_bn128_range_sum_dev, lib.pil2gl_bn128_range_sum, 4)):
        span = n * stride * 8 * words
        f0, num, mm, out = (base + i * span for i in range(4))
        assert out + span <= buf.ctypes.data + buf.nbytes
        top_ok = stride - (3 if words == 1 else 1)       # the highest column out may start at

        def call(fn=dev, dev_form=True, **kw):
            """the good call (one f term, two ranges on one m matrix) with named changes: f_* fields of the f term and its side, r_* fields of
            range 1; out, out_stride, out_col, n, n_f, n_r, alpha, beta, T, Rg"""
            side = dict(base=f0, stride=stride, hostCols=cols.ctypes.data, sel=num, selStride=stride, selCol=4)
            f = dict(k=3, coef=1, bus=7)
            r = dict(m=mm, mStride=stride, mCol=1, lo=-3, size=5, row0=2, coef=P - 1, bus=7)
            top = dict(out=out, out_stride=stride, out_col=top_ok, n=n, n_f=1, n_r=2, alpha=ch.ctypes.data, beta=ch.ctypes.data, T=0, Rg=0)
            for key, v in kw.items():
                if key in top:
                    top[key] = v
                elif key.startswith("r_"):
                    r[key[2:]] = v
                else:
                    (f if key[2:] in f else side)[key[2:]] = v
            T = (_lib.LogupTerm * 10)()
            for u in range(10):
                T[u].side = _lib.TupleSide(**side)
                T[u].k, T[u].coef[0], T[u].busId[0] = f["k"], f["coef"], f["bus"]
            Rg = (_lib.RangeTerm * 10)()
            for i in range(10):
                x = r if i == 1 else dict(m=mm, mStride=stride, mCol=0, lo=5, size=n, row0=0, coef=1, bus=9)
                Rg[i].m, Rg[i].mStride, Rg[i].mCol, Rg[i].lo, Rg[i].size, Rg[i].row0 = x["m"], x["mStride"], x["mCol"], x["lo"], x["size"], x["row0"]
                Rg[i].coef[0], Rg[i].busId[0] = x["coef"], x["bus"]
            args = [None if top["T"] is None else T, top["n_f"], None if top["Rg"] is None else Rg, top["n_r"], top["alpha"], top["beta"], top["out"], top["out_stride"],
                    top["out_col"], top["n"]]
            return fn(*(args + ([None] if dev_form else [])))
        err = lib.pil2gl_last_error
        # everything logup_sum refuses for the f terms and out
        assert call(n=(1 << 28) + 1) == EINVAL and b"2^28" in err()
        assert call(f_k=0) == EINVAL and call(f_k=17) == EINVAL and b"1 .. 16" in err()
        assert call(f_hostCols=bad_cols.ctypes.data) == EINVAL and b"term 0: a column >= stride" in err()
        assert call(f_stride=2) == EINVAL and call(f_stride=1 << 32) == EINVAL and b"stride" in err()
        assert call(f_selCol=stride) == EINVAL and b"selTerm 0" in err()
        assert call(out_col=top_ok + 1) == EINVAL and b"out: a column >= stride" in err()
        assert call(out_stride=1 << 32) == EINVAL and b"out: " in err()
        assert call(out_col=top_ok + 1, n_f=0) == EINVAL and b"out: a column >= stride" in err() and call(out_stride=1 << 32, n_f=0) == EINVAL, "out's checks with no f term"
        for key in ("f_base", "f_hostCols", "out", "alpha", "beta"):
            assert call(**{key: None}) == EINVAL, key
        for key in ("out", "alpha", "beta"):
            assert call(n_f=0, **{key: None}) == EINVAL, key + " with no f term"
        if words == 1:
            assert call(f_coef=P) == EINVAL and call(f_bus=(1 << 64) - 1) == EINVAL and b"canonical" in err()
        for key, v in (("f_base", f0), ("f_sel", num), ("out", out)):
            assert call(**{key: v + 8}) == EINVAL and b"aligned" in err(), key
        assert call(out=out + 8, n_f=0) == EINVAL and b"aligned" in err()
        assert call(out=f0, out_col=0) == EINVAL and b"out overlaps" in err(), "a column of the f term that is read"
        # the counts
        assert call(n_r=0) == EINVAL and call(n_r=9) == EINVAL and b"1 .. 8" in err()
        assert call(n_f=9) == EINVAL and b"at most 8" in err()
        assert call(n_f=2, n_r=8) == EINVAL and call(n_f=8, n_r=2) == EINVAL and b"at most 9" in err()
        # the ranges
        assert call(r_size=0) == EINVAL and call(r_size=(1 << 28) + 1, n=1 << 28, n_f=0) == EINVAL and b"range 1: size must be" in err()
        assert call(r_size=7) == EINVAL and call(r_row0=4) == EINVAL and call(r_row0=(1 << 64) - 1) == EINVAL and b"range 1" in err() and b"row0 + size > n" in err()
        assert call(r_mCol=stride) == EINVAL and b"range 1: m: a column >= stride" in err()
        assert call(r_mStride=1 << 32) == EINVAL and b"range 1: m: stride >= 2^32" in err()
        assert call(r_mStride=1 << 31, n=1 << 28, n_f=0) == EINVAL and b"2^58" in err()
        assert call(r_m=None) == EINVAL and b"null" in err()
        assert call(r_m=mm + 8) == EINVAL and b"aligned" in err()
        if words == 1:
            assert call(r_coef=P) == EINVAL and call(r_bus=(1 << 64) - 1) == EINVAL and b"range 1: coef and busId must be canonical" in err()
        assert call(Rg=None) == EINVAL and b"null ranges" in err()
        assert call(T=None) == EINVAL and b"null terms" in err(), "null hostTerms with nF > 0"
        # the aliasing rule: every m counts as a read column of its matrix
        assert call(out=mm, out_col=1) == EINVAL and b"out overlaps an m matrix" in err(), "out on an m column"
        assert call(out=mm, out_col=0) == EINVAL and b"out overlaps an m matrix" in err(), "range 0's column"
        if words == 1:
            assert call(out=mm, out_col=top_ok, r_mCol=stride - 1) == EINVAL and b"out overlaps an m matrix" in err(), "m under out's third word"
        assert call(out=mm + 16 * words, out_col=2) == EINVAL and b"out overlaps an m matrix" in err(), "a foreign base inside m's matrix"
        assert call(out=mm, out_stride=stride + 1) == EINVAL and b"out overlaps an m matrix" in err(), "another stride"
        assert call(n=0) == 0 and call(n=0, f_base=None, r_m=None, out=None) == 0 and call(n=0, n_f=0, T=None, out=None) == 0, "n = 0: no device"
        hcall = lambda **kw: call(fn=host, dev_form=False, **kw)                 # noqa: E731
        assert hcall(n=(1 << 28) + 1) == EINVAL and hcall(f_k=17) == EINVAL and hcall(n_r=9) == EINVAL and hcall(n_f=8) == EINVAL
        assert hcall(r_size=0) == EINVAL and hcall(r_row0=4) == EINVAL and hcall(r_mCol=stride) == EINVAL and hcall(out_col=stride) == EINVAL
        assert hcall(out=mm, out_col=1) == EINVAL and b"out overlaps an m matrix" in err()
        for key in ("f_base", "r_m", "out", "alpha", "beta", "T", "Rg"):
            assert hcall(**{key: None}) == EINVAL, key
        assert hcall(n=0) == 0
        if not _have_gpu():
            assert call() == ENODEV and call(n_f=0, T=None) == ENODEV and call(n_f=0, n_r=8) == ENODEV and call(n_f=8, n_r=1) == ENODEV and call(n_f=1, n_r=8) == ENODEV
            assert call(out=mm, out_col=2) == ENODEV, "spare columns of the m matrix: nothing to refuse"
            assert call(out=f0, out_col=3 if words == 1 else 4, f_sel=None) == ENODEV, "spare columns of the f term's matrix"
            assert call(r_lo=-(1 << 63)) == ENODEV and call(r_lo=(1 << 63) - 5) == ENODEV and call(r_row0=3) == ENODEV and call(r_size=1, r_row0=7) == ENODEV
            assert hcall() == ENODEV and hcall(out=out + 8, r_m=mm + 8) == ENODEV, "the host forms need no alignment"
            assert hcall(n_f=0, T=None) == ENODEV
    a = np.zeros((8, 8), np.uint64)
    with pytest.raises(pil2gl.Pil2glError, match="out overlaps an m matrix"):
        pilcheck.range_sum([], [((a, 1), 0, 8, 0, P - 1, 0)], [1, 0, 0], [2, 0, 0], (a, 1), 8)
    with pytest.raises(pil2gl.Pil2glError, match="need more"):
        pilcheck.range_sum([], [((a, 8), 0, 8, 0, P - 1, 0)], [1, 0, 0], [2, 0, 0], (a, 1), 8)
    with pytest.raises(pil2gl.Pil2glError, match="3 words"):
        pilcheck.range_sum([], [((a, 0), 0, 8, 0, P - 1, 0)], [1, 0], [2, 0, 0], (a, 1), 8)
    with pytest.raises(pil2gl.Pil2glError, match="range 0: coef is 1 words"):
        pilcheck.range_sum([], [((a, 0), 0, 8, 0, [1, 2], 0)], [1, 0, 0], [2, 0, 0], (a, 1), 8)
    if not _have_gpu():
        with pytest.raises(pil2gl.Pil2glError, match="-2"):
            pilcheck.range_sum([(a, [4], None, 1, 3)], [((a, 0), -3, 8, 0, P - 1, 3)], [1, 0, 0], [2, 0, 0], (a, 1), 8)
        frm = np.zeros((8, 4, 4), np.uint64)
        with pytest.raises(pil2gl.Pil2glError, match="-2"):
            pilcheck.range_sum([], [((frm, 0), -3, 8, 0, [1, 0, 0, 0], [0, 0, 0, 0])], [1, 0, 0, 0], [2, 0, 0, 0], (frm, 3), 8, field="bn128")
