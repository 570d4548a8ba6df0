"""The plookup argument without a device: the checker (tests/plookup_ref.py) against a direct transcription of grandProductPlookup.js
lines 42-77 and 120-164, the closing of valid lookups at sizes that pin the cyclic neighbour, the plan's numbers, the planner, its
validation and the packed job in a program of its own under the sanitizers (tests/plookup_plan_dump.cpp), the refusals of the compute
entries before any device call, n = 0, ENODEV otherwise, and the exported surface."""
import ctypes as C
import inspect
import json
import os
import random
import re
import subprocess

import numpy as np
import pytest

import plookup_ref as pref
import logup_sum_ref as lref
import bn128_hints_ref as bref
from hints_ref import P
from conftest import ROOT

import pil2gl  # noqa: E402  (a plain import: without the feature, or with a broken build, this file fails)
from pil2gl import _lib, pilcheck, bn128  # noqa: E402

EINVAL, ENODEV = -1, -2
R = bref.R
# name -> the declared argument count
NAMES = {"pil2gl_plookup_plan": 6,
         "pil2gl_plookup_fold_dev": 15, "pil2gl_bn128_plookup_fold_dev": 15, "pil2gl_plookup_fold": 14, "pil2gl_bn128_plookup_fold": 14,
         "pil2gl_plookup_prod_dev": 20, "pil2gl_bn128_plookup_prod_dev": 20, "pil2gl_plookup_prod": 19, "pil2gl_bn128_plookup_prod": 19}
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
    full = open(os.path.join(ROOT, "include", "pil2gl.h")).read()
    header = re.sub(r"/\*.*?\*/", "", full, flags=re.S)
    for n, argc in NAMES.items():
        m = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % n, header)
        assert m, n + " is not declared in pil2gl.h"
        assert len(m.group(1).split(",")) == argc, n + ": the header declares another argument count"
        assert n in _lib.SIGNATURES, n + " is not bound in _lib.py"
        assert len(_lib.SIGNATURES[n][1]) == argc, n + ": _lib.py binds another argument count"
        assert getattr(lib, n)
    for f in ("plookup_plan", "plookup_fold", "plookup_fold_dev", "plookup_prod", "plookup_prod_dev", "plookup_h1h2", "plookup_h1h2_dev"):
        assert callable(getattr(pilcheck, f))
    assert list(inspect.signature(pilcheck.plookup_prod_dev).parameters)[:10] == ["f", "t", "h1", "h2", "alpha", "beta", "gamma", "delta", "out", "n"]
    listed = full[full.index("only ENQUEUE work on that stream"):full.index("dev_upload_async / dev_download_async")]
    assert "plookup_fold, plookup_prod" in listed, "the header's list of enqueue-only calls"
    assert "plookup_plan" in full[full.index("Calls that need no device say so"):full.index("Calls are not thread-safe")]
    for cite in ("grandProductPlookup.js:10-11", ":42-50", ":51-55", ":64-72", ":73-77", ":120-135", ":143-164", "polutils.js:132-145"):
        assert cite in full, "the header cites " + cite


# ---- the checker against the reference's way of building the expressions ----
def _sub(F, a, b):
    return F.add(a, tuple((F.q - x) % F.q for x in b) if isinstance(b, tuple) else (F.q - b) % F.q)


def _transcribed(F, f, sel_f, t, sel_t, h1, h2, alpha, beta, gamma, delta):
    """grandProductPlookup.js, expression by expression; the line of the reference beside each step -> (fExp, tExp, num, den) columns"""
    n = len(t)
    t_col, f_col = [], []
    for i in range(n):
        t_exp = None                                                             # :42
        for e in t[i]:                                                           # :43
            t_exp = F.base(e) if t_exp is None else F.add(F.mul(alpha, t_exp), F.base(e))    # :46 / :48
        if sel_t is not None:                                                    # :51
            t_exp = _sub(F, t_exp, beta)                                         # :52
            t_exp = F.mul(t_exp, F.base(sel_t[i]))                               # :53
            t_exp = F.add(t_exp, beta)                                           # :54
        f_exp = None                                                             # :64
        for e in f[i]:                                                           # :65
            f_exp = F.base(e) if f_exp is None else F.add(F.mul(f_exp, alpha), F.base(e))    # :68 / :70
        if sel_f is not None:                                                    # :73
            f_exp = _sub(F, f_exp, t_exp)                                        # :74
            f_exp = F.mul(f_exp, F.base(sel_f[i]))                               # :75
            f_exp = F.add(f_exp, t_exp)                                          # :76
        t_col.append(t_exp)
        f_col.append(f_exp)
    one = F.one
    num, den = [], []
    for i in range(n):
        tp, h1p = t_col[(i + 1) % n], h1[(i + 1) % n]                            # :98, :94  the next row, cyclic
        num.append(F.mul(F.mul(F.add(f_col[i], gamma),                           # :122
                               F.add(F.add(t_col[i], F.mul(tp, delta)),          # :123-130
                                     F.mul(gamma, F.add(one, delta)))),          # :131
                         F.add(one, delta)))                                     # :134
        den.append(F.mul(F.add(F.add(h1[i], F.mul(h2[i], delta)),                # :144-151
                               F.mul(gamma, F.add(one, delta))),                 # :152
                         F.add(F.add(h2[i], F.mul(h1p, delta)),                  # :154-161
                               F.mul(gamma, F.add(one, delta)))))                # :162
    return f_col, t_col, num, den


def _calculate_z(F, num, den):
    """polutils.js calculateZ over the checker's field: one batch of inverses, then the serial walk"""
    inv = [F.zero if d == F.zero else F.inv(d) for d in den]
    z = [F.one]
    for i in range(len(num) - 1):
        z.append(F.mul(z[i], F.mul(num[i], inv[i])))
    return z


@pytest.mark.parametrize("field", ["gl", "bn128"])
def test_checker_against_the_transcription(field):
    """A self-check of the CHECKER only: it runs no library code."""
    rng = random.Random(11)
    F = lref.FIELDS[field]
    q = F.q
    ext = (lambda: tuple(rng.randrange(q) for _ in range(3))) if field == "gl" else (lambda: rng.randrange(q))
    for n, k_f, k_t, with_f, with_t in ((1, 1, 1, False, False), (2, 3, 3, True, True), (7, 2, 5, True, False), (12, 16, 16, False, True), (9, 1, 4, True, True)):
        f = [[rng.randrange(q) for _ in range(k_f)] for _ in range(n)]
        t = [[rng.randrange(q) for _ in range(k_t)] for _ in range(n)]
        sel_f = [rng.choice((0, 1, 2, rng.randrange(q))) for _ in range(n)] if with_f else None
        sel_t = [rng.choice((0, 1, q - 1)) for _ in range(n)] if with_t else None
        h1, h2 = [ext() for _ in range(n)], [ext() for _ in range(n)]
        alpha, beta, gamma, delta = ext(), ext(), ext(), ext()
        f_col, t_col, num, den = _transcribed(F, f, sel_f, t, sel_t, h1, h2, alpha, beta, gamma, delta)
        assert pref.fold(field, (f, sel_f), (t, sel_t), alpha, beta) == (f_col, t_col)
        assert pref.num_den(field, (f, sel_f), (t, sel_t), h1, h2, alpha, beta, gamma, delta) == (num, den)
        assert pref.plookup_z(field, (f, sel_f), (t, sel_t), h1, h2, alpha, beta, gamma, delta) == _calculate_z(F, num, den)
    # a zero den factor: the ratio of its row is 0 and every later z
    z = pref.z_of(field, [F.one] * 4, [F.one, F.zero, F.one, F.one])
    assert z == [F.one, F.one, F.zero, F.zero]


@pytest.mark.parametrize("field", ["gl", "bn128"])
@pytest.mark.parametrize("n", [1, 2, 3, 8, 9, 100])
def test_valid_lookups_close(field, n):
    """z[n-1] num[n-1] / den[n-1] = 1 for a lookup that holds, at sizes that are no power of two: the neighbour of row n - 1 is row 0"""
    rng = random.Random(100 * n + len(field))
    F = lref.FIELDS[field]
    ext = (lambda: tuple(rng.randrange(F.q) for _ in range(3))) if field == "gl" else (lambda: rng.randrange(F.q))
    for k_f, k_t, sel_f, sel_t in ((1, 1, False, False), (3, 3, True, True), (2, 5, True, False), (4, 2, False, True)):
        f, t, h1, h2, alpha, beta = pref.valid_lookup(rng, field, n, k_f, k_t, sel_f, sel_t)
        gamma, delta = ext(), ext()
        assert pref.closing(field, f, t, h1, h2, alpha, beta, gamma, delta) == F.one, (k_f, k_t, sel_f, sel_t)
    # an f value that is not in t does not close
    if n >= 3:
        f, t, h1, h2, alpha, beta = pref.valid_lookup(rng, field, n, 1, 1)
        f[0][0][0] = (max(r[0] for r in t[0]) + 1) % F.q
        if [f[0][0][0]] not in t[0]:
            assert pref.closing(field, f, t, h1, h2, alpha, beta, ext(), ext()) != F.one


def test_plan_values(lib):
    for n in SHAPES:
        for field in ("gl", "bn128"):
            want, nbytes = pref.plan(n, field)
            for k_f, k_t in ((1, 1), (16, 16), (2, 5)):
                got = pilcheck.plookup_plan(n, k_f, k_t, field)
                assert (got["threads"], got["items"], got["blocks"], got["launches"], got["depth"], got["outWidth"]) == want, (n, field)
                assert got["workBytes"] == nbytes, "the working memory does not grow with k"
    gl = pilcheck.plookup_plan(2048 * 256 + 1, 3, 3, "gl")
    assert (gl["blocks"], gl["depth"], gl["launches"]) == (257, 2, 3) and gl["workBytes"] == 24 * (2048 * 256 + 1) + 24 * 257, "gsum's slots"
    for n, levels in ((1, 1), (64, 1), (65, 2), (1025, 3), (16385, 4), (262145, 5)):
        fr = pilcheck.plookup_plan(n, 3, 3, "bn128")
        scan = bn128.scan_plan(n, "gprod")
        assert fr["depth"] == levels == scan["levels"] and fr["launches"] == 4 * levels - 1
        assert fr["workBytes"] == scan["scratchBytes"] + 64 * n, "bnscan::plan's bytes plus 64 n"
    info = (C.c_uint32 * 6)()
    b = C.c_uint64(7)
    for n, k_f, k_t, words, msg in (((1 << 28) + 1, 1, 1, 1, b"2^28"), (8, 0, 1, 1, b"kF"), (8, 17, 1, 4, b"kF"), (8, 1, 0, 1, b"kT"), (8, 1, 17, 4, b"kT"),
                                    (8, 1, 1, 3, b"elemWords"), (8, 1, 1, 0, b"elemWords")):
        assert lib.pil2gl_plookup_plan(n, k_f, k_t, words, info, C.byref(b)) == EINVAL and msg in lib.pil2gl_last_error()
        assert b.value == 0


def test_planner_validation_and_job_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "plookup_plan_dump")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                           os.path.join(ROOT, "tests", "plookup_plan_dump.cpp"), "-o", exe])
    refused = [((1 << 28) + 1, 1, 1, 1), (8, 0, 1, 1), (8, 1, 17, 1), (8, 1, 1, 3), ((1 << 64) - 1, 16, 16, 4)]
    B, O = 1 << 40, 1 << 50                          # byte addresses; never dereferenced
    big = 1 << 30                                    # 2^28 rows of 2^30 elements: n stride = 2^58, the largest that passes
    top = (1 << 32) - 1
    # (prod, n, words, dev, kF, kT, hDim, stride, selStride, hStride, base, step, oBase, oStride, oCol, oCol2) -> ok, or a word of the message
    calls = [
        ((1, 8, 1, 1, 16, 16, 3, 16, 8, 6, B, 4096, O, 8, 5, 0), 1), ((1, 8, 4, 1, 16, 16, 1, 16, 8, 2, B, 4096, O, 8, 7, 0), 1),     # k = 16 both sides
        ((1, 8, 1, 1, 2, 5, 1, 8, 0, 2, B, 4096, O, 3, 0, 0), 1), ((0, 8, 1, 1, 2, 5, 3, 8, 0, 0, B, 4096, O, 6, 0, 3), 1),
        ((0, 8, 1, 1, 1, 1, 1, 8, 0, 0, B, 4096, O, 2, 0, 1), 1),                                                   # hDim 1: the range-check shape
        ((0, 8, 1, 1, 2, 1, 1, 8, 0, 0, B, 4096, O, 2, 0, 1), "hDim = 1"), ((0, 8, 1, 1, 1, 1, 1, 8, 8, 0, B, 4096, O, 2, 0, 1), "hDim = 1"),
        ((1, 8, 1, 1, 2, 2, 1, 8, 8, 2, B, 4096, O, 3, 0, 0), 1),                                                   # the product takes hDim as given
        ((1, 8, 1, 1, 1, 1, 2, 8, 0, 4, B, 4096, O, 3, 0, 0), "hDim"), ((1, 8, 4, 1, 1, 1, 3, 8, 0, 4, B, 4096, O, 3, 0, 0), "hDim"),
        ((1, 8, 1, 1, 17, 1, 3, 32, 0, 6, B, 4096, O, 3, 0, 0), "kF"), ((1, 8, 1, 1, 1, 0, 3, 32, 0, 6, B, 4096, O, 3, 0, 0), "kT"),
        ((1, 8, 1, 1, 3, 1, 3, 2, 0, 6, B, 4096, O, 3, 0, 0), "f: a column >= stride"),
        ((1, 8, 1, 1, 1, 3, 3, 2, 0, 6, B, 4096, O, 3, 0, 0), "t: a column >= stride"),
        ((1, 8, 1, 1, 1, 1, 3, top, top, top, B, 1 << 36, O, top, top - 3, 0), 1),                                  # the widest stride, every matrix
        ((1, 8, 1, 1, 1, 1, 3, top + 1, 0, 6, B, 1 << 36, O, 8, 0, 0), "stride >= 2^32"),
        ((1, 8, 1, 1, 1, 1, 3, 8, top + 1, 6, B, 4096, O, 8, 0, 0), "selF"), ((1, 8, 1, 1, 1, 1, 3, 8, 0, top + 1, B, 4096, O, 8, 0, 0), "h1"),
        ((1, 8, 1, 1, 1, 1, 3, 8, 0, 5, B, 4096, O, 8, 0, 0), "h2: a column >= stride"), ((1, 8, 1, 1, 1, 1, 1, 8, 0, 2, B, 4096, O, 8, 0, 0), 1),
        ((1, 8, 1, 1, 1, 1, 3, 8, 0, 6, B, 4096, O, 8, 6, 0), "out: a column >= stride"), ((1, 8, 4, 1, 1, 1, 1, 8, 0, 2, B, 4096, O, 8, 7, 0), 1),
        ((0, 8, 1, 1, 1, 1, 3, 8, 0, 0, B, 4096, O, 8, 0, 6), "outT: a column >= stride"), ((0, 8, 1, 1, 1, 1, 3, 8, 0, 0, B, 4096, O, 8, 6, 0), "outF: a column >= stride"),
        ((1, 1 << 28, 4, 1, 1, 1, 1, big, big, big, B, 0, B, big, big - 2, 0), 1),                                  # the 2^58 limit: spans of 2^63 bytes, no overflow
        ((1, 1 << 28, 1, 1, 1, 1, 1, big, big, big, B, 0, B, big, big - 4, 0), 1),
        ((1, 1 << 28, 1, 1, 1, 1, 1, big, big, big, B, 0, B, big, big - 3, 0), "overlaps"),                         # the third word is the read column
        ((1, 1 << 28, 1, 1, 1, 1, 3, big + 1, 0, 6, B, 0, O, 8, 0, 0), "2^58"), ((1, 1 << 28, 1, 1, 1, 1, 3, 8, 0, big + 1, B, 0, O, 8, 0, 0), "2^58"),
        ((1, 8, 1, 1, 1, 1, 3, 8, 0, 6, B + 8, 4096, O, 8, 0, 0), "aligned"), ((1, 8, 1, 0, 1, 1, 3, 8, 0, 6, B + 8, 4096, O + 8, 8, 0, 0), 1),   # the host forms need no alignment
        ((1, 8, 1, 1, 1, 1, 3, 8, 0, 6, B, 4096, O + 8, 8, 0, 0), "aligned"),
        ((1, 8, 1, 1, 1, 1, 3, 8, 0, 6, 0, 0, O, 8, 0, 0), "null buffer"), ((1, 8, 1, 1, 1, 1, 3, 8, 0, 6, B, 4096, 0, 8, 0, 0), "null buffer"),
        ((1, 8, 1, 1, 2, 2, 1, 8, 0, 8, B, 0, B, 8, 2, 0), 1), ((1, 8, 1, 1, 2, 2, 1, 8, 0, 8, B, 0, B, 8, 4, 0), "overlaps"),     # f reads 6, 7; t and h 0, 1
        ((1, 8, 1, 1, 2, 2, 1, 8, 0, 8, B, 0, B, 8, 1, 0), "overlaps"),
        ((1, 8, 1, 1, 1, 1, 1, 8, 6, 2, B, 0, B, 8, 3, 0), "overlaps"),                                             # the selector's matrix (stride 6) is a read matrix
        ((1, 8, 1, 1, 1, 1, 1, 8, 0, 6, B, 0, B, 8, 3, 0), "overlaps"),                                             # and h's
        ((1, 8, 1, 1, 1, 1, 1, 8, 8, 8, B, 0, B, 9, 0, 0), "overlaps"),
        ((0, 8, 1, 1, 2, 2, 3, 16, 0, 0, B, 0, B, 16, 2, 5), 1), ((0, 8, 1, 1, 2, 2, 3, 16, 0, 0, B, 0, B, 16, 2, 4), "outF overlaps outT"),
        ((0, 8, 4, 1, 2, 2, 1, 16, 0, 0, B, 0, B, 16, 2, 2), "outF overlaps outT"), ((0, 8, 4, 1, 2, 2, 1, 16, 0, 0, B, 0, B, 16, 2, 3), 1),
        ((1, 0, 1, 1, 1, 1, 3, 8, 0, 6, 0, 0, 0, 8, 0, 0), 1),                                                      # no rows: nothing is looked at
    ]
    with open(tmp_path / "cmds.txt", "w") as f:
        f.write("".join("plan %d %d %d %d\n" % (n, kf, kt, w) for n in SHAPES for kf, kt, w in ((1, 1, 1), (16, 16, 4))))
        f.write("".join("plan %d %d %d %d\n" % r for r in refused))
        f.write("".join("call " + " ".join(map(str, c)) + "\n" for c, _ in calls))
        f.write("layout\n")
    run = subprocess.run([exe, str(tmp_path / "cmds.txt")], capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", "sanitizer report:\n" + run.stderr[-4000:]
    out = [json.loads(line) for line in run.stdout.splitlines()]
    assert len(out) == 2 * len(SHAPES) + len(refused) + len(calls) + 1
    for i, got in enumerate(out[:2 * len(SHAPES)]):
        want, nbytes = pref.plan(SHAPES[i // 2], ("gl", "bn128")[i % 2])
        assert got["ok"] == 1 and (got["threads"], got["items"], got["blocks"], got["launches"], got["depth"], got["width"]) == want
        assert got["bytes"] == nbytes
    at = 2 * len(SHAPES)
    assert all(g["ok"] == 0 and g["why"] for g in out[at:at + len(refused)])
    at += len(refused)
    for (c, want), got in zip(calls, out[at:-1]):
        if want == 1:
            assert got["ok"] == 1, (c, got)
            prod, words, k_f, k_t, h_dim, stride, sel_stride = c[0], c[2], c[4], c[5], c[6], c[7], c[8]
            assert (got["kF"], got["kT"], got["lastColF"], got["lastColT"], got["hDim"]) == (k_f, k_t, stride - k_f, k_t - 1, h_dim), (c, got)
            assert got["selColT"] == (sel_stride - 1 if sel_stride else 0) and got["h2Col"] == ((h_dim if words == 1 else 1) if prod else 0)
            assert got["jobBytes"] + 64 <= 4096, "the job and a kernel's other arguments fit 4 KB"
        else:
            assert got["ok"] == 0 and want in got["why"], (c, got)
    lay = out[-1]
    assert (lay["side"], lay["column"]) == (96, 16) and lay["glJob"] <= 4032 and lay["frJob"] <= 4032


def test_compute_entries_refuse_before_any_device_call(lib):
    buf = np.full(40000, 0x5A5A5A5A5A5A5A5A, np.uint64)
    before = buf.copy()
    base = buf.ctypes.data + (-buf.ctypes.data % 16)
    cols = np.array([2, 0, 1] + [0] * 14, np.uint64)
    bad_cols = np.array([2, 8, 1], np.uint64)
    n, stride = 8, 8
    ch = np.array([3, 4, 5, 6], np.uint64)
    for field, words in (("", 1), ("bn128_", 4)):
        fold_dev, fold, prod_dev, prod = (getattr(lib, "pil2gl_%splookup_%s" % (field, s)) for s in ("fold_dev", "fold", "prod_dev", "prod"))
        span = n * stride * 8 * words
        t, f0, sel, h, out = (base + i * span for i in range(5))
        assert out + span <= buf.ctypes.data + buf.nbytes
        h_dim = 3 if words == 1 else 1
        hw = h_dim if words == 1 else 1
        top_ok = stride - (3 if words == 1 else 1)       # the highest column z may start at

        def call(which="prod", dev_form=True, **kw):
            """the good call with named changes: t_* and f_* side fields and k; h1, h1_stride, h1_col, h2, ..; out, out_stride, out_col (the
            product's z and the fold's outF), out2, out2_stride, out2_col (the fold's outT); the challenges; F, T (the side pointers); n, h_dim"""
            side = {"t": dict(base=t, stride=stride, hostCols=cols.ctypes.data, sel=sel, selStride=stride, selCol=4),
                    "f": dict(base=f0, stride=stride, hostCols=cols.ctypes.data, sel=None, selStride=0, selCol=0)}
            top = dict(t_k=3, f_k=2, h1=h, h1_stride=stride, h1_col=0, h2=h, h2_stride=stride, h2_col=hw, h_dim=h_dim, out=out, out_stride=stride,
                       out_col=top_ok if which == "prod" else 0, out2=out, out2_stride=stride, out2_col=hw, n=n, alpha=ch.ctypes.data, beta=ch.ctypes.data,
                       gamma=ch.ctypes.data, delta=ch.ctypes.data, F=0, T=0)
            for key, v in kw.items():
                if key in top:
                    top[key] = v
                else:
                    s, name = key.split("_", 1)
                    side[s][name] = v
            sf, st = _lib.TupleSide(**side["f"]), _lib.TupleSide(**side["t"])
            args = [None if top["F"] is None else C.pointer(sf), top["f_k"], None if top["T"] is None else C.pointer(st), top["t_k"]]
            if which == "prod":
                args += [top[x] for x in ("h1", "h1_stride", "h1_col", "h2", "h2_stride", "h2_col", "h_dim", "alpha", "beta", "gamma", "delta", "out", "out_stride",
                                          "out_col", "n")]
                fn = prod_dev if dev_form else prod
            else:
                args += [top[x] for x in ("alpha", "beta", "h_dim", "out", "out_stride", "out_col", "out2", "out2_stride", "out2_col", "n")]
                fn = fold_dev if dev_form else fold
            return fn(*(args + ([None] if dev_form else [])))
        err = lib.pil2gl_last_error
        for which in ("prod", "fold"):
            for dev_form in (True, False):
                c = lambda **kw: call(which, dev_form, **kw)                     # noqa: E731
                assert c(n=(1 << 28) + 1) == EINVAL and b"2^28" in err()
                assert c(t_k=0) == EINVAL and b"kT" in err() and c(f_k=17) == EINVAL and b"kF" in err()
                assert c(h_dim=2) == EINVAL and c(h_dim=0) == EINVAL and b"hDim" in err()
                assert c(h_dim=4 - h_dim) == EINVAL if words == 4 or which == "fold" else True
                assert c(t_hostCols=bad_cols.ctypes.data) == EINVAL and b"t: a column >= stride" in err()
                assert c(f_hostCols=bad_cols.ctypes.data, f_k=1) != EINVAL, "a side reads only its own k columns"
                assert c(f_stride=2) == EINVAL and c(t_stride=1 << 32) == EINVAL and b"stride" in err()
                assert c(f_stride=1 << 31, n=1 << 28) == EINVAL and b"2^58" in err()
                assert c(t_selCol=stride) == EINVAL and b"selT" in err()
                assert c(out_col=stride - (hw if which == "fold" else 3 if words == 1 else 1) + 1) == EINVAL and b"a column >= stride" in err()
                assert c(out_stride=1 << 32) == EINVAL and b"out" in err()
                for key in ("t_base", "f_base", "f_hostCols", "t_hostCols", "out", "alpha", "beta", "F", "T"):
                    assert c(**{key: None}) == EINVAL, key
                assert c(n=0) == 0 and c(n=0, t_base=None, f_base=None, out=None, h1=None) == 0, "n = 0: no device"
            c = lambda **kw: call(which, True, **kw)                             # noqa: E731
            for key, v in (("t_base", t), ("f_base", f0), ("t_sel", sel), ("out", out)):
                assert c(**{key: v + 8}) == EINVAL and b"aligned" in err(), key
            # the aliasing rule, the selector's matrix counting as a read matrix
            for where in (t, f0):
                assert c(out=where, out_col=2) == EINVAL and b"overlaps" in err(), "column 2 is read of both"
                assert c(out=where + 16 * words, out_col=1) == EINVAL and b"overlaps" in err(), "a foreign base"
                assert c(out=where, out_stride=stride + 1) == EINVAL and b"overlaps" in err(), "another stride"
            assert c(out=sel, out_col=4) == EINVAL and b"overlaps" in err(), "the selector's column"
        c = lambda **kw: call("prod", True, **kw)                                # noqa: E731
        for key in ("gamma", "delta", "h1", "h2"):
            assert c(**{key: None}) == EINVAL, key
        assert c(h1=h + 8) == EINVAL and b"aligned" in err() and c(h2=h + 8) == EINVAL and b"aligned" in err()
        assert c(h2_col=stride - hw + 1) == EINVAL and b"h2: a column >= stride" in err()
        assert c(h1_stride=1 << 32) == EINVAL and b"h1" in err()
        assert c(out=h, out_col=hw) == EINVAL and b"overlaps" in err(), "h2's column"
        assert c(out=h, out_col=0) == EINVAL and b"overlaps" in err(), "h1's column"
        c = lambda **kw: call("fold", True, **kw)                                # noqa: E731
        assert c(out2=out + 8) == EINVAL and b"aligned" in err()
        assert c(out2=None) == EINVAL and b"null buffer" in err()
        assert c(out2_col=0) == EINVAL and b"outF overlaps outT" in err(), "one column for both"
        assert c(out2_stride=stride + 1) == EINVAL and b"outF overlaps outT" in err()
        assert c(out2=t, out2_col=2) == EINVAL and b"overlaps" in err(), "outT on a read column"
        if words == 1:
            assert c(out_col=0, out2_col=2) == EINVAL and b"outF overlaps outT" in err(), "three words each"
            assert c(h_dim=1) == EINVAL and b"hDim = 1" in err(), "kF = 2"
            assert c(h_dim=1, f_k=1, t_k=1) == EINVAL and b"hDim = 1" in err(), "selT"
            assert c(h_dim=1, f_k=1, t_k=1, t_sel=None, out2_col=1) != EINVAL, "the range-check shape"
            assert call("prod", True, h_dim=1, h2_col=1) != EINVAL, "the product takes hDim as given"
        if not _have_gpu():
            for which in ("prod", "fold"):
                assert call(which) == ENODEV and call(which, f_k=1, t_k=1) == ENODEV
                assert call(which, out=t, out_col=top_ok if which == "prod" else 3, out2=f0, out2_col=3) == ENODEV, "spare columns of a read matrix"
                assert call(which, False) == ENODEV and call(which, False, out=out + 8, out2=out + 8) == ENODEV, "the host forms need no alignment"
            assert (buf == before).all(), "a refused call and a call without a device leave every buffer as it was"
    a = np.zeros((8, 12), np.uint64)
    one = [1, 0, 0]
    with pytest.raises(pil2gl.Pil2glError, match="overlaps"):
        pilcheck.plookup_prod((a, [0, 1]), (a, [2, 3], (a, 5)), (a, 6), (a, 9), one, one, one, one, (a, 5), 8)
    with pytest.raises(pil2gl.Pil2glError, match="need more"):
        pilcheck.plookup_prod((a, [0, 1]), (a, [2, 3]), (a, 6), (a, 10), one, one, one, one, (a, 3), 8)
    with pytest.raises(pil2gl.Pil2glError, match="3 words"):
        pilcheck.plookup_prod((a, [0, 1]), (a, [2, 3]), (a, 6), (a, 9), [1, 0], one, one, one, (a, 3), 8)
    with pytest.raises(pil2gl.Pil2glError, match="hDim = 1"):
        pilcheck.plookup_fold((a, [0, 1]), (a, [2, 3]), one, one, (a, 6), (a, 7), 8, h_dim=1)
    if not _have_gpu():
        with pytest.raises(pil2gl.Pil2glError, match="-2"):
            pilcheck.plookup_prod((a, [0, 1]), (a, [2]), (a, 3), (a, 6), one, one, one, one, (a, 9), 8)
        with pytest.raises(pil2gl.Pil2glError, match="-2"):
            pilcheck.plookup_fold((a, [0]), (a, [1]), one, one, (a, 2), (a, 3), 8, h_dim=1)
        frm = np.zeros((8, 6, 4), np.uint64)
        one4 = [1, 0, 0, 0]
        with pytest.raises(pil2gl.Pil2glError, match="-2"):
            pilcheck.plookup_prod((frm, [0]), (frm, [1], (frm, 2)), (frm, 3), (frm, 4), one4, one4, one4, one4, (frm, 5), 8, field="bn128")
