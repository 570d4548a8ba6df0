"""The grand product of a permutation or a connection without a device: the checker (tests/grand_prod_ref.py) against an independent
restatement built the way the reference's two files build their expressions, the plan's numbers at the level and block thresholds, the
planner, its validation and the packed term table in a program of its own under the sanitizers (tests/grand_prod_plan_dump.cpp), the layout
of pil2gl_grand_prod_term against the header and the addon, the refusals of the compute entries before any device call, n = 0, ENODEV
otherwise, and the exported surface."""
import ctypes as C
import json
import os
import random
import re
import shutil
import subprocess

import numpy as np
import pytest

import grand_prod_ref as gref
import logup_sum_ref as lref
import bn128_hints_ref as bref
from hints_ref import P
from conftest import ROOT

import pil2gl  # noqa: E402  (a plain import: without the feature, or with a broken build, this file fails)
from pil2gl import _lib, pilcheck, bn128  # noqa: E402

EINVAL, ENODEV = -1, -2
R = bref.R
NAMES = ("pil2gl_grand_prod_plan", "pil2gl_grand_prod_dev", "pil2gl_bn128_grand_prod_dev", "pil2gl_grand_prod", "pil2gl_bn128_grand_prod")
CSRC = os.path.join(ROOT, "pil2-stark-js_amd", "csrc")
SHAPES = (0, 1, 8, 9, 2048, 2049, 2048 * 256 + 1, 64, 65, 1024, 1025, 16385, 262145, 1 << 28)
LAYOUT = ("size", "side", "k", "den", "id", "idStride", "idCol", "idCoef")
NODE = shutil.which("node")


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
    T = _lib.GrandProdTerm
    return dict(size=C.sizeof(T), **{f: getattr(T, f).offset for f in LAYOUT[1:]})


def test_entries_are_declared_bound_and_exported(lib):
    full = open(os.path.join(ROOT, "include", "pil2gl.h")).read()
    header = re.sub(r"/\*.*?\*/", "", full, flags=re.S)
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, header), n + " is not declared in pil2gl.h"
        assert n in _lib.SIGNATURES, n + " is not bound in _lib.py"
        assert getattr(lib, n)
    assert "pil2gl_grand_prod_term" in header
    for f in ("grand_prod_plan", "grand_prod", "grand_prod_dev", "perm_prod", "perm_prod_dev", "conn_prod", "conn_prod_dev"):
        assert callable(getattr(pilcheck, f))
    listed = full[full.index("only ENQUEUE work on that stream"):full.index("dev_upload_async / dev_download_async")]
    assert "grand_prod and bn128_grand_prod" in listed, "the header's list of enqueue-only calls"
    for cite in ("grandProductPermutation.js:35-48", "grandProductConnection.js:35-45", "polutils.js:132-145"):
        assert cite in full, "the header cites " + cite


# ---- the checker against the reference's way of building the two expressions ----
def _calculate_z(F, num, den):
    """polutils.js calculateZ over the checker's field: one batch of inverses, then the serial walk"""
    inv = [F.zero if d == F.zero else F.inv(d) for d in den]
    z = [F.one]
    for i in range(len(num) - 1):
        z.append(F.mul(z[i], F.mul(num[i], inv[i])))
    return z


def _sub(F, a, b):
    return F.add(a, tuple((F.q - x) % F.q for x in b) if isinstance(b, tuple) else (F.q - b) % F.q)


@pytest.mark.parametrize("field", ["gl", "bn128"])
def test_checker_against_the_reference_shaped_restatement(field):
    """A self-check of the CHECKER only: it runs no library code."""
    rng = random.Random(7)
    F = lref.FIELDS[field]
    q, n = F.q, 24
    ext = (lambda: tuple(rng.randrange(q) for _ in range(3))) if field == "gl" else (lambda: rng.randrange(q))
    for k in (1, 3):
        f = [[rng.randrange(q) for _ in range(k)] for _ in range(n)]
        t = [[rng.randrange(q) for _ in range(k)] for _ in range(n)]
        sel_f, sel_t = [rng.choice((0, 1, 2, rng.randrange(q))) for _ in range(n)], [rng.choice((0, 1, q - 1)) for _ in range(n)]
        alpha, beta, gamma = ext(), ext(), ext()
        num, den = [], []
        for i in range(n):                                                       # grandProductPermutation.js: tExp = alpha tExp + e, nested from the first
            t_exp = F.base(t[i][0])
            for e in t[i][1:]:
                t_exp = F.add(F.mul(alpha, t_exp), F.base(e))
            t_exp = F.add(F.mul(_sub(F, t_exp, beta), F.base(sel_t[i])), beta)   # (tExp - beta) selT + beta
            f_exp = F.base(f[i][0])
            for e in f[i][1:]:
                f_exp = F.add(F.mul(f_exp, alpha), F.base(e))
            f_exp = F.add(F.mul(_sub(F, f_exp, beta), F.base(sel_f[i])), beta)
            num.append(F.add(f_exp, gamma))
            den.append(F.add(t_exp, gamma))
        terms = [(f, sel_f, 0, None, None), (t, sel_t, 1, None, None)]
        assert gref.grand_prod(field, terms, alpha, beta, gamma, n) == _calculate_z(F, num, den)
        assert gref.num_den(field, terms, alpha, beta, gamma, n) == (num, den)
    # grandProductConnection.js: numExp and denExp as running products over the columns
    n_cols = 5
    a = [[rng.randrange(q) for _ in range(n_cols)] for _ in range(n)]
    S = [[rng.randrange(q) for _ in range(n_cols)] for _ in range(n)]
    x = [rng.randrange(q) for _ in range(n)]
    ks = [rng.randrange(q) for _ in range(n_cols - 1)]
    gamma, delta = ext(), ext()
    num, den = [], []
    for i in range(n):
        num_exp = F.add(F.add(F.base(a[i][0]), F.mul(delta, F.base(x[i]))), gamma)
        den_exp = F.add(F.add(F.base(a[i][0]), F.mul(delta, F.base(S[i][0]))), gamma)
        for j in range(1, n_cols):
            num_exp = F.mul(num_exp, F.add(F.add(F.base(a[i][j]), F.mul(F.mul(delta, F.base(ks[j - 1])), F.base(x[i]))), gamma))
            den_exp = F.mul(den_exp, F.add(F.add(F.base(a[i][j]), F.mul(delta, F.base(S[i][j]))), gamma))
        num.append(num_exp)
        den.append(den_exp)
    den[5] = F.zero                                                              # calculateZ's side of the zero convention is checked below
    terms = []
    for j in range(n_cols):
        terms.append(([[r[j]] for r in a], None, 0, x, F.mul(delta, F.base(1 if j == 0 else ks[j - 1]))))
        terms.append(([[r[j]] for r in a], None, 1, [r[j] for r in S], delta))
    got_num, got_den = gref.num_den(field, terms, gamma, gamma, gamma, n)
    assert got_num == num and got_den[:5] + got_den[6:] == den[:5] + den[6:]
    z = gref.grand_prod(field, terms, gamma, gamma, gamma, n)
    assert z == _calculate_z(F, got_num, got_den) and z[0] == F.one
    # a zero den factor: R = 0 and every later z is 0; an empty side is 1
    zero_g = _sub(F, F.zero, F.base(a[3][0]))
    z = gref.grand_prod(field, [([[r[0]] for r in a], None, 1, None, None)], gamma, gamma, zero_g, n)
    assert z[3] != F.zero and all(v == F.zero for v in z[4:])
    assert gref.grand_prod(field, terms, gamma, gamma, gamma, n, period=n) == gref.grand_prod(field, terms, gamma, gamma, gamma, n)


def test_plan_values(lib):
    for n in SHAPES:
        for field in ("gl", "bn128"):
            want, nbytes = gref.plan(n, field)
            for n_terms, sum_k in ((1, 1), (40, 64), (4, 64)):
                got = pilcheck.grand_prod_plan(n, n_terms, sum_k, field)
                assert (got["threads"], got["items"], got["blocks"], got["launches"], got["depth"], got["outWidth"]) == want, (n, field)
                assert got["workBytes"] == nbytes, "the working memory grows with neither nTerms nor k"
    gl = pilcheck.grand_prod_plan(2048 * 256 + 1, 36, 36, "gl")
    assert (gl["blocks"], gl["depth"], gl["launches"]) == (257, 2, 3) and gl["workBytes"] == 24 * (2048 * 256 + 1) + 24 * 257, "gsum's slots"
    for n, levels in ((1, 1), (64, 1), (65, 2), (1025, 3), (16385, 4), (262145, 5)):
        fr = pilcheck.grand_prod_plan(n, 3, 3, "bn128")
        scan = bn128.scan_plan(n, "gprod")
        assert fr["depth"] == levels == scan["levels"] and fr["launches"] == 4 * levels - 1
        assert fr["workBytes"] == scan["scratchBytes"] + 64 * n, "bnscan::plan's bytes plus 64 n"
    info = (C.c_uint32 * 6)()
    b = C.c_uint64(7)
    for n, n_terms, sum_k, words, msg in (((1 << 28) + 1, 1, 1, 1, b"2^28"), (8, 0, 0, 1, b"1 .. 40"), (8, 41, 41, 4, b"1 .. 40"), (8, 2, 1, 1, b"add up"),
                                           (8, 5, 65, 4, b"add up"), (8, 2, 33, 1, b"add up"), (8, 1, 1, 3, b"elemWords"), (8, 1, 1, 0, b"elemWords")):
        assert lib.pil2gl_grand_prod_plan(n, n_terms, sum_k, words, info, C.byref(b)) == EINVAL and msg in lib.pil2gl_last_error()
        assert b.value == 0


@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_term_layout_matches_what_the_addon_states():
    js = "const a = require(%r).addon; console.log(JSON.stringify([a.grandProdTermLayout()].concat(['grandProdPlan', 'grandProdDev', 'grandProd'].map((f) => typeof a[f]))));"
    out = subprocess.run([NODE, "-e", js % os.path.join(ROOT, "pil2-stark-js_amd", "js", "native.js")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    got = json.loads(out.stdout)
    assert got[0] == _layout() and got[1:] == ["function"] * 3
    src = open(os.path.join(ROOT, "pil2-stark-js_amd", "js", "pil_checks.js")).read()
    assert re.search(r"module\.exports = \{[^}]*grandProduct, grandProductDev, grandProductPlan", src)
    for f in ("polutils.js", "polutils_bn128.js"):
        src = open(os.path.join(ROOT, "pil2-stark-js_amd", "js", f)).read()
        for name in ("calculateZPermutation", "calculateZPermutationDev", "calculateZConnection", "calculateZConnectionDev"):
            assert name in src, (f, name)


def test_planner_validation_and_table_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "grand_prod_plan_dump")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                           os.path.join(ROOT, "tests", "grand_prod_plan_dump.cpp"), "-o", exe])
    refused = [((1 << 28) + 1, 1, 1, 1), (8, 0, 0, 1), (8, 41, 41, 1), (8, 1, 1, 3), (8, 4, 65, 4), (8, 3, 2, 1), ((1 << 64) - 1, 40, 64, 4)]
    B, O = 1 << 40, 1 << 50                          # byte addresses; never dereferenced
    big = 1 << 30                                    # 2^28 rows of 2^30 elements: n stride = 2^58, the largest that passes
    top = (1 << 32) - 1
    # (n, words, dev, nTerms, k, stride, selStride, idStride, base, step, oBase, oStride, oCol) -> ok, or a word of the message
    calls = [
        ((8, 1, 1, 40, 1, 8, 8, 8, B, 4096, O, 8, 5), 1), ((8, 4, 1, 40, 1, 8, 8, 8, B, 4096, O, 8, 7), 1),          # 40 terms
        ((8, 1, 1, 4, 16, 16, 0, 0, B, 4096, O, 3, 0), 1), ((8, 4, 0, 4, 16, 16, 0, 3, B, 4096, O, 1, 0), 1),       # sum k = 64 exactly
        ((8, 1, 1, 40, 2, 8, 0, 0, B, 4096, O, 8, 0), "add up"), ((8, 1, 1, 5, 13, 16, 0, 0, B, 4096, O, 8, 0), "add up"),
        ((8, 1, 1, 41, 1, 8, 0, 0, B, 4096, O, 8, 0), "1 .. 40"), ((8, 1, 1, 2, 17, 32, 0, 0, B, 4096, O, 8, 0), "1 .. 16"),
        ((8, 1, 1, 2, 0, 8, 0, 0, B, 4096, O, 8, 0), "1 .. 16"),
        ((8, 1, 1, 2, 3, 2, 0, 0, B, 4096, O, 8, 0), "column >= stride"),
        ((8, 1, 1, 2, 1, top, top, top, B, 1 << 36, O, top, top - 3), 1),                                            # the widest stride, every matrix
        ((8, 1, 1, 2, 1, top + 1, 0, 0, B, 1 << 36, O, 8, 0), "stride >= 2^32"),
        ((8, 1, 1, 2, 1, 8, top + 1, 0, B, 4096, O, 8, 0), "selTerm 0"), ((8, 1, 1, 2, 1, 8, 0, top + 1, B, 4096, O, 8, 0), "id of term 0"),
        ((8, 1, 1, 2, 1, 8, 0, 0, B, 4096, O, 8, 6), "out: a column >= stride"), ((8, 4, 1, 2, 1, 8, 0, 0, B, 4096, O, 8, 7), 1),
        ((1 << 28, 4, 1, 2, 1, big, big, big, B, 0, B, big, big - 2), 1),                                            # the 2^58 limit: spans of 2^63 bytes, no overflow
        ((1 << 28, 1, 1, 2, 1, big, big, big, B, 0, B, big, big - 4), 1),
        ((1 << 28, 1, 1, 2, 1, big, big, big, B, 0, B, big, big - 3), "out overlaps"),                               # the third word is the read column
        ((1 << 28, 1, 1, 2, 1, big + 1, 0, 0, B, 0, O, 8, 0), "2^58"), ((1 << 28, 1, 1, 2, 1, 8, 0, big + 1, B, 0, O, 8, 0), "2^58"),
        ((8, 1, 1, 2, 1, 8, 0, 0, B + 8, 4096, O, 8, 0), "aligned"), ((8, 1, 0, 2, 1, 8, 0, 0, B + 8, 4096, O + 8, 8, 0), 1),     # the host forms need no alignment
        ((8, 1, 1, 2, 1, 8, 0, 0, B, 4096, O + 8, 8, 0), "aligned"),
        ((8, 1, 1, 2, 1, 8, 0, 0, 0, 0, O, 8, 0), "null buffer"), ((8, 1, 1, 2, 1, 8, 0, 0, B, 4096, 0, 8, 0), "null buffer"),
        ((8, 1, 1, 2, 2, 8, 0, 0, B, 0, B, 8, 3), 1), ((8, 1, 1, 2, 2, 8, 0, 0, B, 0, B, 8, 4), "out overlaps"),              # columns 6, 7 are read
        ((8, 1, 1, 2, 1, 8, 6, 0, B, 0, B, 8, 3), "out overlaps"),                                                   # the selector's matrix (stride 6) is a read matrix
        ((8, 1, 1, 2, 1, 8, 0, 6, B, 0, B, 8, 3), "out overlaps"),                                                   # and the id column's
        ((8, 1, 1, 2, 1, 8, 8, 8, B, 0, B, 8, 4), 1), ((8, 1, 1, 2, 1, 8, 8, 8, B, 0, B, 9, 0), "out overlaps"),
        ((0, 1, 1, 2, 1, 8, 0, 0, 0, 0, 0, 8, 0), 1),                                                                # no rows: nothing is looked at
    ]
    with open(tmp_path / "cmds.txt", "w") as f:
        f.write("".join("plan %d %d %d %d\n" % (n, nt, sk, w) for n in SHAPES for nt, sk, w in ((1, 1, 1), (40, 64, 4))))
        f.write("".join("plan %d %d %d %d\n" % r for r in refused))
        f.write("".join("call " + " ".join(map(str, c)) + "\n" for c, _ in calls))
        f.write("layout\n")
    run = subprocess.run([exe, str(tmp_path / "cmds.txt")], capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", "sanitizer report:\n" + run.stderr[-4000:]
    out = [json.loads(line) for line in run.stdout.splitlines()]
    assert len(out) == 2 * len(SHAPES) + len(refused) + len(calls) + 1
    for i, got in enumerate(out[:2 * len(SHAPES)]):
        want, nbytes = gref.plan(SHAPES[i // 2], ("gl", "bn128")[i % 2])
        assert got["ok"] == 1 and (got["threads"], got["items"], got["blocks"], got["launches"], got["depth"], got["width"]) == want
        assert got["bytes"] == nbytes
    at = 2 * len(SHAPES)
    assert all(g["ok"] == 0 and g["why"] for g in out[at:at + len(refused)])
    at += len(refused)
    for (c, want), got in zip(calls, out[at:-1]):
        if want == 1:
            assert got["ok"] == 1, (c, got)
            n_terms, k, stride = c[3], c[4], c[5]
            assert got["sumK"] == n_terms * k and got["lastStart"] == (n_terms - 1) * k and got["lastCol"] == stride - k and got["den"] == (n_terms - 1) % 2
            assert got["jobBytes"] + 64 <= 4096, "the job and a kernel's other arguments fit 4 KB"
        else:
            assert got["ok"] == 0 and want in got["why"], (c, got)
    lay = out[-1]
    assert {k: lay[k] for k in LAYOUT} == _layout()
    assert tuple(lay[k] for k in LAYOUT) == (120, 0, 48, 56, 64, 72, 80, 88)
    assert (lay["glTerm"], lay["frTerm"]) == (72, 80) and lay["glJob"] <= 4032 and lay["frJob"] <= 4032


def test_compute_entries_refuse_before_any_device_call(lib):
    buf = np.full(32768, 0x5A5A5A5A5A5A5A5A, np.uint64)
    before = buf.copy()
    base = buf.ctypes.data + (-buf.ctypes.data % 16)
    cols = np.array([2, 0, 1] + [0] * 14, np.uint64)
    bad_cols = np.array([2, 8, 1], np.uint64)
    n, stride = 8, 8
    ch = np.array([3, 4, 5, 6], np.uint64)
    for dev, host, words in ((lib.pil2gl_grand_prod_dev, lib.pil2gl_grand_prod, 1), (lib.pil2gl_bn128_grand_prod_dev, lib.pil2gl_bn128_grand_prod, 4)):
        span = n * stride * 8 * words
        t, f0, ids, out = (base + i * span for i in range(4))
        assert out + span <= buf.ctypes.data + buf.nbytes
        top_ok = stride - (3 if words == 1 else 1)       # the highest column out may start at

        def call(fn=dev, dev_form=True, **kw):
            """the good call with named changes: t_*, f_* fields of a term (side fields, k, den, id, idStride, idCol, coef); out, out_stride,
            out_col, n, n_terms, alpha, beta, gamma, T"""
            side = {"t": dict(base=t, stride=stride, hostCols=cols.ctypes.data, sel=ids, selStride=stride, selCol=4),
                    "f": dict(base=f0, stride=stride, hostCols=cols.ctypes.data, sel=None, selStride=0, selCol=0)}
            extra = {"t": dict(k=3, den=1, id=ids, idStride=stride, idCol=5, coef=7), "f": dict(k=1, den=0, id=None, idStride=0, idCol=0, coef=1)}
            top = dict(out=out, out_stride=stride, out_col=top_ok, n=n, n_terms=2, alpha=ch.ctypes.data, beta=ch.ctypes.data, gamma=ch.ctypes.data, T=0)
            for key, v in kw.items():
                if key in top:
                    top[key] = v
                else:
                    s, name = key.split("_", 1)
                    (extra if name in extra[s] else side)[s][name] = v
            T = (_lib.GrandProdTerm * 41)()
            for u in range(41):
                s = "f" if u % 2 == 0 else "t"
                T[u].side = _lib.TupleSide(**side[s])
                T[u].k, T[u].den, T[u].id, T[u].idStride, T[u].idCol = (extra[s][x] for x in ("k", "den", "id", "idStride", "idCol"))
                T[u].idCoef[1] = extra[s]["coef"]
            args = [None if top["T"] is None else T, top["n_terms"], top["alpha"], top["beta"], top["gamma"], top["out"], top["out_stride"], top["out_col"], top["n"]]
            return fn(*(args + ([None] if dev_form else [])))
        err = lib.pil2gl_last_error
        assert call(n=(1 << 28) + 1) == EINVAL and b"2^28" in err()
        assert call(n_terms=0) == EINVAL and call(n_terms=41) == EINVAL and b"1 .. 40" in err()
        assert call(t_k=0) == EINVAL and call(f_k=17) == EINVAL and b"1 .. 16" in err()
        assert call(n_terms=40, t_k=3) == EINVAL and b"add up" in err(), "20 terms of 3 and 20 of 1: 80 columns"
        assert call(t_den=2) == EINVAL and b"den is 0" in err()
        assert call(t_hostCols=bad_cols.ctypes.data) == EINVAL and b"term 1: a column >= stride" in err()
        assert call(f_hostCols=bad_cols.ctypes.data) != EINVAL, "a term reads only its own k columns"
        assert call(f_stride=2) == EINVAL and call(t_stride=1 << 32) == EINVAL and b"stride" in err()
        assert call(f_stride=1 << 31, n=1 << 28) == EINVAL and b"2^58" in err()
        assert call(t_selCol=stride) == EINVAL and b"selTerm 1" in err()
        assert call(t_idCol=stride) == EINVAL and b"id of term 1: a column >= stride" in err()
        assert call(t_idStride=1 << 32) == EINVAL and b"id of term 1" in err()
        assert call(out_col=top_ok + 1) == EINVAL and b"out: a column >= stride" in err()
        assert call(out_stride=1 << 32) == EINVAL and b"out: " in err()
        for key in ("t_base", "f_base", "f_hostCols", "t_hostCols", "out", "alpha", "beta", "gamma", "T"):
            assert call(**{key: None}) == EINVAL, key
        assert call(f_base=None, f_id=ids, f_idStride=stride) == EINVAL and b"null buffer" in err(), "an id given with a null base"
        if words == 1:
            assert call(t_coef=P) == EINVAL and call(f_coef=(1 << 64) - 1) == EINVAL and b"canonical" in err()
        for key, v in (("t_base", t), ("f_base", f0), ("t_sel", ids), ("t_id", ids), ("out", out)):
            assert call(**{key: v + 8}) == EINVAL and b"aligned" in err(), key
        # the aliasing rule, the selector's and the id column's matrices counting as read matrices
        for where in (t, f0):
            assert call(out=where, out_col=2) == EINVAL and b"out overlaps" in err(), "column 2 is read of both"
            assert call(out=where + 16 * words, out_col=1) == EINVAL and b"out overlaps" in err(), "a foreign base"
            assert call(out=where, out_stride=stride + 1) == EINVAL and b"out overlaps" in err(), "another stride"
        assert call(out=ids, out_col=4) == EINVAL and b"out overlaps" in err(), "the selector's column"
        assert call(out=ids, out_col=5 if words == 4 else 3) == EINVAL and b"out overlaps" in err(), "the id column (under out's third word over Goldilocks)"
        assert call(t_sel=None, t_id=None, out=ids, out_col=4) != EINVAL, "a matrix no term reads"
        assert call(n=0) == 0 and call(n=0, t_base=None, f_base=None, out=None) == 0, "n = 0: no device"
        hcall = lambda **kw: call(fn=host, dev_form=False, **kw)                 # noqa: E731
        assert hcall(n=(1 << 28) + 1) == EINVAL and hcall(t_k=17) == EINVAL and hcall(n_terms=41) == EINVAL and hcall(t_den=7) == EINVAL
        assert hcall(t_hostCols=bad_cols.ctypes.data) == EINVAL and hcall(out_col=stride) == EINVAL and hcall(t_idCol=9) == EINVAL
        assert hcall(out=t, out_col=1) == EINVAL and b"out overlaps" in err()
        for key in ("t_base", "f_base", "t_hostCols", "out", "alpha", "beta", "gamma", "T"):
            assert hcall(**{key: None}) == EINVAL, key
        assert hcall(n=0) == 0
        if not _have_gpu():
            assert call() == ENODEV and call(n_terms=40, t_k=2) == ENODEV and call(n_terms=1) == ENODEV
            assert call(out=t, out_col=top_ok) == ENODEV and call(out=ids, out_col=6 if words == 4 else 0) == ENODEV, "spare columns of a read matrix"
            assert hcall() == ENODEV and hcall(out=out + 8) == ENODEV, "the host forms need no alignment"
            assert (buf == before).all(), "a refused call and a call without a device leave every buffer as it was"
    a = np.zeros((8, 8), np.uint64)
    with pytest.raises(pil2gl.Pil2glError, match="out overlaps"):
        pilcheck.perm_prod((a, [0, 1]), (a, [2, 3], (a, 5)), [1, 0, 0], [2, 0, 0], [3, 0, 0], (a, 5), 8)
    with pytest.raises(pil2gl.Pil2glError, match="need more"):
        pilcheck.perm_prod((a, [0, 1]), (a, [2, 3]), [1, 0, 0], [2, 0, 0], [3, 0, 0], (a, 6), 8)
    with pytest.raises(pil2gl.Pil2glError, match="3 words"):
        pilcheck.perm_prod((a, [0, 1]), (a, [2, 3]), [1, 0], [2, 0, 0], [3, 0, 0], (a, 5), 8)
    with pytest.raises(pil2gl.Pil2glError, match="idCoef is 3 words"):
        pilcheck.grand_prod([(a, [0], None, 0, (a, 1), [1, 2])], [1, 0, 0], [2, 0, 0], [3, 0, 0], (a, 5), 8)
    with pytest.raises(pil2gl.Pil2glError, match="as many S columns"):
        pilcheck.conn_terms([(a, 0), (a, 1)], [(a, 2)], (a, 3), [5], [1, 0, 0])
    # conn_terms: delta ks'_j word by word, ks' = 1, ks[0], ..
    terms = pilcheck.conn_terms([(a, 0), (a, 1)], [(a, 2), (a, 3)], (a, 4), [P - 1], [3, 0, P - 5])
    assert [t[3] for t in terms] == [0, 1, 0, 1] and terms[0][5] == [3, 0, P - 5] and terms[2][5] == [P - 3, 0, 5] and terms[1][5] == terms[3][5] == [3, 0, P - 5]
    assert terms[2][4] == (a, 4) and terms[3][4] == (a, 3) and terms[3][1] == [1]
    fr_terms = pilcheck.conn_terms([(a, 0), (a, 1)], [(a, 2), (a, 3)], (a, 4), [R - 1], [5, 0, 0, 0], "bn128")
    assert bn128._ints(fr_terms[2][5])[0] == R - 5
    if not _have_gpu():
        with pytest.raises(pil2gl.Pil2glError, match="-2"):
            pilcheck.conn_prod([(a, 0), (a, 1)], [(a, 2), (a, 3)], (a, 4), [7], [1, 0, 0], [2, 0, 0], (a, 5), 8)
        frm = np.zeros((8, 4, 4), np.uint64)
        with pytest.raises(pil2gl.Pil2glError, match="-2"):
            pilcheck.perm_prod((frm, [0]), (frm, [1], (frm, 2)), [1, 0, 0, 0], [2, 0, 0, 0], [3, 0, 0, 0], (frm, 3), 8, field="bn128")
