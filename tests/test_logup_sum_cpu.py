"""The lookup grand sum without a device: the plan's numbers against their restatement (tests/logup_sum_ref.py) -- through the library
and, in a program of its own, under the sanitizers (tests/logup_sum_plan_dump.cpp) together with the aliasing rule of out and the layout of
pil2gl_logup_term -- the refusals of the compute entries before any device call, ENODEV otherwise, the checker's own identity
(s[i] - s[i-1]) prod D_u = N, and the exported surface."""
import ctypes as C
import json
import os
import random
import re
import subprocess

import numpy as np
import pytest

import logup_sum_ref as lref
import bn128_hints_ref as bref
from hints_ref import P, mul3
from conftest import ROOT

import pil2gl  # noqa: E402  (a plain import: without the feature, or with a broken build, this file fails)
from pil2gl import _lib, pilcheck, bn128  # noqa: E402

EINVAL, ENODEV = -1, -2
R = bref.R
NAMES = ("pil2gl_logup_sum_plan", "pil2gl_logup_sum_dev", "pil2gl_bn128_logup_sum_dev", "pil2gl_logup_sum", "pil2gl_bn128_logup_sum",
         "pil2gl_gsum_col_dev", "pil2gl_bn128_gsum_col", "pil2gl_bn128_gsum_col_dev")
CSRC = os.path.join(ROOT, "pil2-stark-js_amd", "csrc")
SHAPES = (0, 1, 8, 9, 2048, 2049, 2048 * 256 + 1, 64, 65, 1024, 1025, 16385, 262145, 1 << 28)


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
    assert "pil2gl_logup_term" in header
    for f in ("logup_sum_plan", "logup_sum", "logup_sum_dev"):
        assert callable(getattr(pilcheck, f))
    assert callable(pil2gl.calculateS_col) and callable(bn128.gsum_col)
    from pil2gl import stark
    assert callable(stark.GpuBackend.gsum_col)
    full = open(os.path.join(ROOT, "include", "pil2gl.h")).read()
    listed = full[full.index("only ENQUEUE work on that stream"):full.index("dev_upload_async / dev_download_async")]
    assert "logup_sum and bn128_logup_sum" in listed and "gsum_col" in listed, "the header's list of enqueue-only calls"


def test_plan_values(lib):
    for n in SHAPES:
        for field in ("gl", "bn128"):
            want, nbytes = lref.plan(n, 2, field)
            for n_terms in (1, 9):
                got = pilcheck.logup_sum_plan(n, n_terms, field)
                assert (got["threads"], got["items"], got["blocks"], got["launches"], got["depth"], got["outWidth"]) == want, (n, field)
                assert got["workBytes"] == nbytes, "the working memory grows with neither nTerms nor k"
    gl = pilcheck.logup_sum_plan(2048 * 256 + 1, 9, "gl")
    assert (gl["blocks"], gl["depth"], gl["launches"]) == (257, 2, 3), "257 block totals: a lane of the second pass walks two"
    assert gl["workBytes"] == 24 * (2048 * 256 + 1) + 24 * 257, "what gsum takes: 3 words a row, 3 a block"
    for n, levels in ((1, 1), (64, 1), (65, 2), (1025, 3), (16385, 4), (262145, 5)):
        fr = pilcheck.logup_sum_plan(n, 3, "bn128")
        scan = bn128.scan_plan(n, "gprod")
        assert fr["depth"] == levels == scan["levels"] and fr["launches"] == 4 * levels - 1
        assert fr["workBytes"] == scan["scratchBytes"] + 64 * n, "bnscan::plan's bytes plus 64 n"
    info = (C.c_uint32 * 6)()
    b = C.c_uint64(7)
    for n, n_terms, words, msg in (((1 << 28) + 1, 1, 1, b"2^28"), (8, 0, 1, b"1 .. 9"), (8, 10, 4, b"1 .. 9"), (8, 1, 3, b"elemWords"), (8, 1, 0, b"elemWords")):
        assert lib.pil2gl_logup_sum_plan(n, n_terms, words, info, C.byref(b)) == EINVAL and msg in lib.pil2gl_last_error()
        assert b.value == 0


NODE = __import__("shutil").which("node")


@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_term_layout_matches_what_the_addon_states():
    """the ctypes struct against sizeof / offsetof as the ADDON was compiled (a fresh Node child; no device needed), and the addon's surface"""
    js = "const a = require(%r).addon; console.log(JSON.stringify([a.logupTermLayout()].concat(['logupSumPlan', 'logupSumDev', 'logupSum', 'gsumColDev', 'bn128GsumColDev'].map((f) => typeof a[f]))));"
    out = subprocess.run([NODE, "-e", js % os.path.join(ROOT, "pil2-stark-js_amd", "js", "native.js")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    got = json.loads(out.stdout)
    T = _lib.LogupTerm
    assert got[0] == dict(size=C.sizeof(T), side=T.side.offset, k=T.k.offset, coef=T.coef.offset, busId=T.busId.offset)
    assert got[1:] == ["function"] * 5
    src = open(os.path.join(ROOT, "pil2-stark-js_amd", "js", "pil_checks.js")).read()
    assert re.search(r"module\.exports = \{[^}]*logupSum, logupSumDev", src)
    for f in ("polutils.js", "polutils_bn128.js"):
        src = open(os.path.join(ROOT, "pil2-stark-js_amd", "js", f)).read()
        assert "calculateSCol" in src and "calculateSColDev" in src, f


def test_term_layout_matches_the_header(tmp_path):
    exe = str(tmp_path / "dump")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", CSRC, os.path.join(ROOT, "tests", "logup_sum_plan_dump.cpp"), "-o", exe])
    (tmp_path / "c.txt").write_text("layout\n")
    got = json.loads(subprocess.run([exe, str(tmp_path / "c.txt")], capture_output=True, text=True, check=True).stdout)
    T = _lib.LogupTerm
    assert got == dict(size=C.sizeof(T), side=T.side.offset, k=T.k.offset, coef=T.coef.offset, busId=T.busId.offset)
    assert (got["size"], got["side"], got["k"], got["coef"], got["busId"]) == (120, 0, 48, 56, 88)


def _rand_terms(rng, q, n, shapes):
    terms = []
    for k, with_w in shapes:
        tuples = [[rng.randrange(q) for _ in range(k)] for _ in range(n)]
        w = [rng.choice((0, 1, 2, rng.randrange(q))) for _ in range(n)] if with_w else None
        terms.append((tuples, w, rng.choice((1, q - 1, 5, rng.randrange(q))), rng.randrange(q)))
    return terms


@pytest.mark.parametrize("field", ["gl", "bn128"])
def test_checker_identity(field):
    """(s[i] - s[i-1]) prod D_u = N on random small inputs, with the products over the non-zero D_u; and a forced zero adds nothing.
    A self-check of the CHECKER (tests/logup_sum_ref.py) only: it runs no library code, so it passes without the feature and is no
    evidence about the library -- the other tests of this file and the GPU tests are."""
    rng = random.Random(5)
    F = lref.FIELDS[field]
    q = F.q
    rand_ext = (lambda: tuple(rng.randrange(q) for _ in range(3))) if field == "gl" else (lambda: rng.randrange(q))
    neg = (lambda a: tuple((q - x) % q for x in a)) if field == "gl" else (lambda a: (q - a) % q)
    n = 12
    for shapes in ([(1, False)], [(3, True), (2, False)], [(1, True)] * 9, [(16, True), (1, False), (3, True)]):
        terms = _rand_terms(rng, q, n, shapes)
        alpha, beta = rand_ext(), rand_ext()
        s = lref.logup_sum(field, terms, alpha, beta, n)
        prev = F.zero
        for i in range(n):
            N, D, ratio = lref.row_fraction(F, terms, F.ext(alpha), F.ext(beta), i)
            step = F.add(s[i], neg(prev))
            assert step == ratio and F.mul(step, D) == N and D != F.zero
            prev = s[i]
    # one term of three forced to zero at row 4: beta = -(its compressed tuple + bus id); the sum is that of the other two there
    terms = _rand_terms(rng, q, n, [(2, True), (3, False), (1, True)])
    alpha = rand_ext()
    beta = neg(lref.denominator(F, terms[1][0][4], F.ext(alpha), F.zero, terms[1][3]))
    assert lref.denominator(F, terms[1][0][4], F.ext(alpha), F.ext(beta), terms[1][3]) == F.zero
    s3 = lref.logup_sum(field, terms, alpha, beta, n)
    others = [lref.row_fraction(F, [terms[0], terms[2]], F.ext(alpha), F.ext(beta), i)[2] for i in range(n)]
    full = [lref.row_fraction(F, terms, F.ext(alpha), F.ext(beta), i)[2] for i in range(n)]
    assert full[4] == others[4] and F.add(s3[4], neg(s3[3])) == others[4]
    # the Horner order: first column highest, the bus id the last Horner term
    if field == "gl":
        a = (3, 1, 4)
        want = [(x + y + z) % P for x, y, z in zip(mul3(mul3(a, a), (7, 0, 0)), mul3(a, (9, 0, 0)), (11 + 2, 5, 6))]
        assert lref.denominator(F, [7, 9], a, (2, 5, 6), 11) == tuple(want)
    else:
        assert lref.denominator(F, [7, 9], 3, 2, 11) == (7 * 9 + 9 * 3 + 11 + 2) % R
    # gsum_col: a constant column gives gsum's words
    den = [rand_ext() for _ in range(n)]
    one_num = F.ext(rand_ext())
    col = lref.gsum_col(field, [one_num] * n, den)
    acc = F.zero
    for i in range(n):
        acc = F.add(acc, F.mul(one_num, F.inv(F.ext(den[i]))))
        assert col[i] == acc


def test_planner_and_aliasing_rule_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "logup_sum_plan_dump")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                           os.path.join(ROOT, "tests", "logup_sum_plan_dump.cpp"), "-o", exe])
    refused = [((1 << 28) + 1, 1, 1), (8, 0, 1), (8, 10, 1), (8, 1, 3), ((1 << 64) - 1, 9, 4)]
    B = 1 << 40                                       # a byte address; never dereferenced
    big = 1 << 30                                     # 2^28 rows of 2^30 elements: n stride = 2^58, the largest that passes
    alias = [  # (n, words, oBase, oStride, oCol, rBase, rStride, cols) -> (ok, columns)
        ((8, 1, B, 8, 5, B, 8, [0, 2, 4]), (1, 1)),                              # three spare word columns of the same matrix
        ((8, 1, B, 8, 4, B, 8, [0, 2, 4]), (0, 1)),                              # the first of the three is read
        ((8, 1, B, 8, 2, B, 8, [0, 3]), (0, 1)),                                 # the middle one
        ((8, 1, B, 8, 2, B, 8, [0, 4]), (0, 1)),                                 # the last one
        ((8, 1, B, 8, 1, B, 8, [0, 4]), (1, 1)),                                 # between two read columns
        ((8, 4, B, 4, 1, B, 4, [3]), (1, 1)),                                    # Fr: one element column
        ((8, 4, B, 4, 3, B, 4, [3]), (0, 1)),
        ((8, 1, B, 8, 5, B, 9, [0]), (0, 1)),                                    # the same base, another stride
        ((8, 1, B + 8, 8, 1, B, 8, [0]), (0, 1)),                                # the same stride, another base
        ((8, 1, B + 8 * 57, 8, 0, B, 8, [0]), (1, 1)),                           # r ends with element (7, 0) at word 56: word 57 on is free
        ((8, 1, B + 8 * 56, 8, 0, B, 8, [0]), (0, 1)),                           # ... word 56 is not
        ((8, 1, B, 8, 0, B + 8 * 59, 8, [7]), (1, 1)),                           # the other way round: out's span ends with word 58
        ((8, 1, B, 8, 1, B + 8 * 59, 8, [7]), (0, 1)),                           # out's span reaches word 59 through its THIRD word
        ((1, 1, B, 3, 0, B + 24, 1, [0]), (1, 1)), ((1, 1, B, 3, 0, B + 16, 1, [0]), (0, 1)),      # one row
        ((8, 1, B, 8, 6, B, 8, [0]), (0, 0)), ((8, 1, B, 8, 5, B, 8, [0]), (1, 1)),              # oCol + 2 must stay below the stride
        ((8, 1, B, 1 << 32, 0, B, 4, [0]), (0, 0)), ((8, 1, B, 8, 0, B, 4, [4]), (0, 0)),
        ((8, 1, B, (1 << 32) - 1, (1 << 32) - 4, B, (1 << 32) - 1, [0, (1 << 32) - 5]), (1, 1)),   # the widest stride
        ((8, 1, B, (1 << 32) - 1, (1 << 32) - 3, B, (1 << 32) - 1, [0]), (0, 0)),
        ((1 << 28, 4, B, big, big - 1, B, big, [0, big - 2]), (1, 1)),           # the 2^58 limit: spans of 2^63 bytes, no overflow
        ((1 << 28, 4, B, big, big - 1, B, big, [big - 1]), (0, 1)),
        ((1 << 28, 1, B, big, big - 3, B, big, [0, big - 4]), (1, 1)),
        ((1 << 28, 1, B, big, big - 3, B, big, [big - 2]), (0, 1)),
        ((1 << 28, 4, B, big, 0, B + (1 << 62), big, [0]), (0, 1)),              # a foreign base inside that span
        ((1 << 28, 1, B, big + 1, 0, B, big, [0]), (0, 0)),                      # n stride above 2^58
        ((0, 1, B, 8, 2, B, 8, [2]), (1, 1)),                                    # no rows: nothing meets
    ]
    with open(tmp_path / "cmds.txt", "w") as f:
        f.write("".join("plan %d %d %d\n" % (n, nt, w) for n in SHAPES for nt, w in ((1, 1), (9, 4))))
        f.write("".join("plan %d %d %d\n" % r for r in refused))
        f.write("".join("alias %d %d %d %d %d %d %d %d %s\n" % (a[:7] + (len(a[7]), " ".join(map(str, a[7])))) for a, _ in alias))
        f.write("layout\n")
    run = subprocess.run([exe, str(tmp_path / "cmds.txt")], capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", "sanitizer report:\n" + run.stderr[-4000:]
    out = [json.loads(line) for line in run.stdout.splitlines()]
    assert len(out) == 2 * len(SHAPES) + len(refused) + len(alias) + 1
    for i, got in enumerate(out[:2 * len(SHAPES)]):
        want, nbytes = lref.plan(SHAPES[i // 2], (1, 9)[i % 2], ("gl", "bn128")[i % 2])
        assert got["ok"] == 1 and (got["threads"], got["items"], got["blocks"], got["launches"], got["depth"], got["width"]) == want
        assert got["bytes"] == nbytes
    at = 2 * len(SHAPES)
    assert all(g["ok"] == 0 and g["why"] for g in out[at:at + len(refused)])
    at += len(refused)
    assert [(g["ok"], g["columns"]) for g in out[at:-1]] == [w for _, w in alias]


def test_compute_entries_refuse_before_any_device_call(lib):
    buf = np.zeros(16384, np.uint64)
    base = buf.ctypes.data + (-buf.ctypes.data % 16)
    cols = np.array([2, 0, 1] + [0] * 14, np.uint64)
    bad_cols = np.array([2, 8, 1], np.uint64)
    n, stride = 8, 8
    ch = np.array([3, 4, 5, 6], np.uint64)
    for dev, host, words in ((lib.pil2gl_logup_sum_dev, lib.pil2gl_logup_sum, 1), (lib.pil2gl_bn128_logup_sum_dev, lib.pil2gl_bn128_logup_sum, 4)):
        span = n * stride * 8 * words
        t, f0, num, out = (base + i * span for i in range(4))
        assert out + span <= buf.ctypes.data + buf.nbytes
        top_ok = stride - (3 if words == 1 else 1)       # the highest column out may start at

        def call(fn=dev, dev_form=True, **kw):
            """the good call with named changes: t_*, f_* fields of a term's side, t_k / f_k / t_coef / t_bus; out, out_stride, out_col, n,
            n_terms, alpha, beta, T"""
            side = {"t": dict(base=t, stride=stride, hostCols=cols.ctypes.data, sel=num, selStride=stride, selCol=4),
                    "f": dict(base=f0, stride=stride, hostCols=cols.ctypes.data, sel=None, selStride=0, selCol=0)}
            extra = {"t": dict(k=3, coef=P - 1, bus=7), "f": dict(k=2, coef=1, bus=7)}
            top = dict(out=out, out_stride=stride, out_col=top_ok, n=n, n_terms=2, alpha=ch.ctypes.data, beta=ch.ctypes.data, T=0)
            for key, v in kw.items():
                if key in top:
                    top[key] = v
                else:
                    s, name = key.split("_", 1)
                    (extra if name in extra[s] else side)[s][name] = v
            T = (_lib.LogupTerm * 10)()
            for u in range(10):
                s = "f" if u % 2 == 0 else "t"
                T[u].side = _lib.TupleSide(**side[s])
                T[u].k = extra[s]["k"]
                T[u].coef[0] = extra[s]["coef"]
                T[u].busId[0] = extra[s]["bus"]
            args = [None if top["T"] is None else T, top["n_terms"], top["alpha"], top["beta"], top["out"], top["out_stride"], top["out_col"], top["n"]]
            return fn(*(args + ([None] if dev_form else [])))
        err = lib.pil2gl_last_error
        assert call(n=(1 << 28) + 1) == EINVAL and b"2^28" in err()
        assert call(n_terms=0) == EINVAL and call(n_terms=10) == EINVAL and b"1 .. 9" in err()
        assert call(t_k=0) == EINVAL and call(f_k=17) == EINVAL and b"1 .. 16" in err()
        assert call(t_hostCols=bad_cols.ctypes.data) == EINVAL and b"term 1: a column >= stride" in err()
        assert call(f_hostCols=bad_cols.ctypes.data, f_k=1) != EINVAL, "a term reads only its own k columns"
        assert call(f_stride=2) == EINVAL and call(t_stride=1 << 32) == EINVAL and b"stride" in err()
        assert call(f_stride=1 << 31, n=1 << 28) == EINVAL and b"2^58" in err()
        assert call(t_selCol=stride) == EINVAL and b"selTerm 1" in err()
        assert call(out_col=top_ok + 1) == EINVAL and b"out: a column >= stride" in err()
        assert call(out_stride=1 << 32) == EINVAL and b"out: " in err()
        for key in ("t_base", "f_base", "f_hostCols", "t_hostCols", "out", "alpha", "beta", "T"):
            assert call(**{key: None}) == EINVAL, key
        if words == 1:
            assert call(t_coef=P) == EINVAL and call(f_bus=(1 << 64) - 1) == EINVAL and b"canonical" in err()
        for key, v in (("t_base", t), ("f_base", f0), ("t_sel", num), ("out", out)):
            assert call(**{key: v + 8}) == EINVAL and b"aligned" in err(), key
        # the aliasing rule
        for where in (t, f0):
            assert call(out=where, out_col=0) == EINVAL and b"out overlaps" in err(), "columns 0 .. 2 are read"
            assert call(out=where + 16 * words, out_col=1) == EINVAL and b"out overlaps" in err(), "a foreign base"
            assert call(out=where, out_stride=stride + 1) == EINVAL and b"out overlaps" in err(), "another stride"
        if words == 1:
            assert call(out=t, out_col=1) == EINVAL and call(out=t, out_col=2) == EINVAL and b"out overlaps" in err(), "a read column under the second or third word"
            assert call(out=num, out_col=2) == EINVAL and call(out=num, out_col=4) == EINVAL and b"out overlaps" in err(), "the numerator's column is read too"
        else:
            assert call(out=num, out_col=4) == EINVAL and b"out overlaps" in err()
        assert call(n=0) == 0 and call(n=0, t_base=None, f_base=None, out=None) == 0, "n = 0: no device"
        hcall = lambda **kw: call(fn=host, dev_form=False, **kw)                 # noqa: E731
        assert hcall(n=(1 << 28) + 1) == EINVAL and hcall(t_k=17) == EINVAL and hcall(n_terms=10) == EINVAL
        assert hcall(t_hostCols=bad_cols.ctypes.data) == EINVAL and hcall(out_col=stride) == EINVAL and hcall(t_selCol=9) == EINVAL
        assert hcall(out=t, out_col=1) == EINVAL and b"out overlaps" in err()
        for key in ("t_base", "f_base", "t_hostCols", "out", "alpha", "beta", "T"):
            assert hcall(**{key: None}) == EINVAL, key
        assert hcall(n=0) == 0
        if not _have_gpu():
            assert call() == ENODEV and call(n_terms=9) == ENODEV and call(n_terms=1) == ENODEV
            assert call(out=t, out_col=top_ok) == ENODEV and call(out=f0, out_col=3) == ENODEV, "spare columns of a term's matrix: nothing to refuse"
            assert call(out=num, out_col=5 if words == 1 else 3) == ENODEV, "spare columns of the numerator's matrix"
            assert call(f_base=t, out=t, out_col=top_ok) == ENODEV, "one matrix on every term and out beside them"
            assert hcall() == ENODEV and hcall(out=out + 8) == ENODEV, "the host forms need no alignment"
    # gsum_col: its constant-numerator siblings' refusals
    assert lib.pil2gl_gsum_col_dev(None, 1, base, 1, 0, base, None) in (0, ENODEV)
    for args in ((None, 1, base, 1, 8, base + 4096), (base, 1, None, 1, 8, base + 4096), (base, 1, base + 1024, 1, 8, None), (base, 2, base + 1024, 1, 8, base + 4096)):
        assert lib.pil2gl_gsum_col_dev(*args, None) in (EINVAL, ENODEV)
    fr = lib.pil2gl_bn128_gsum_col_dev
    assert fr(base, 1, base + 1024, 1, 0, base + 4096, 1, None) == 0
    assert fr(None, 1, base + 1024, 1, 8, base + 4096, 1, None) == EINVAL and fr(base, 1, None, 1, 8, base + 4096, 1, None) == EINVAL
    assert fr(base, 0, base + 1024, 1, 8, base + 4096, 1, None) == EINVAL and fr(base, 1, base + 1024, 1, (1 << 28) + 1, base + 4096, 1, None) == EINVAL
    assert fr(base, 1, base + 1024, 1, 8, base + 32, 1, None) == EINVAL and b"overlaps" in lib.pil2gl_last_error(), "out inside num"
    assert fr(base, 1, base + 1024, 1, 8, base + 1024, 1, None) == EINVAL, "out is den"
    assert lib.pil2gl_bn128_gsum_col(base, 1, base + 1024, 1, 8, base + 1024 + 32, 1) == EINVAL
    a = np.zeros((8, 8), np.uint64)
    with pytest.raises(pil2gl.Pil2glError, match="out overlaps"):
        pilcheck.logup_sum([(a, [0, 1], None, 1, 0)], [1, 0, 0], [2, 0, 0], (a, 1), 8)
    with pytest.raises(pil2gl.Pil2glError, match="need more"):
        pilcheck.logup_sum([(a, [0, 1], None, 1, 0)], [1, 0, 0], [2, 0, 0], (a, 6), 8)
    if _have_gpu():
        import torch
        one, col = torch.zeros(1, dtype=torch.int64, device="cuda"), torch.ones(24, dtype=torch.int64, device="cuda")
        with pytest.raises(pil2gl.Pil2glError, match="num holds 1 words"):
            pil2gl.calculateS_col(one, col, 1, 3)                                 # calculateS's one-element numerator is no column
    with pytest.raises(pil2gl.Pil2glError, match="3 words"):
        pilcheck.logup_sum([(a, [0, 1], None, 1, 0)], [1, 0], [2, 0, 0], (a, 5), 8)
    with pytest.raises(pil2gl.Pil2glError, match="in place"):
        pilcheck.logup_sum([(a, [0, 1], None, 1, 0)], [1, 0, 0], [2, 0, 0], (a.astype(np.int64), 5), 8)
    if not _have_gpu():
        with pytest.raises(pil2gl.Pil2glError, match="-2"):
            pilcheck.logup_sum([(a, [0, 1], None, 1, 0), (a, [1], (a, 2), P - 1, 3)], [1, 0, 0], [2, 0, 0], (a, 5), 8)
        frm = np.zeros((8, 4, 4), np.uint64)
        with pytest.raises(pil2gl.Pil2glError, match="-2"):
            pilcheck.logup_sum([(frm, [0], (frm, 1), [1, 0, 0, 0], [0, 0, 0, 0])], [1, 0, 0, 0], [2, 0, 0, 0], (frm, 3), 8, field="bn128")
