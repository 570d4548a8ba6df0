"""The clustered logUp sum without a device: the exported surface and the layout of pil2gl_logup_im_col against the header, the plan's words,
the checker (tests/logup_cluster_ref.py) against itself, the cleared constraint and logup_sum_ref / range_sum_ref, the refusals of the
compute entries before any device call, OK for n = 0, ENODEV otherwise, and the planner with the rule of several outputs in a program of its
own under the sanitizers (tests/logup_cluster_plan_dump.cpp)."""
import ctypes as C
import json
import os
import random
import re
import subprocess

import numpy as np
import pytest

import logup_sum_ref as lref
import range_sum_ref as rref
import logup_cluster_ref as cref
from hints_ref import P
from conftest import ROOT

import pil2gl  # noqa: E402  (a plain import: without the feature, or with a broken build, this file fails)
from pil2gl import _lib, pilcheck  # noqa: E402

EINVAL, ENODEV = -1, -2
NAMES = ("pil2gl_logup_cluster_plan", "pil2gl_logup_cluster_dev", "pil2gl_bn128_logup_cluster_dev", "pil2gl_logup_cluster", "pil2gl_bn128_logup_cluster")
CSRC = os.path.join(ROOT, "pil2-stark-js_amd", "csrc")
SHAPES = (0, 1, 8, 9, 2048, 2049, 2048 * 256 + 1, 64, 65, 1024, 1025, 16385, 262145, 1 << 28)
D = cref.DIRECT


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
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, header), n + " is not declared in pil2gl.h"
        assert n in _lib.SIGNATURES, n + " is not bound in _lib.py"
        assert getattr(lib, n)
    assert "pil2gl_logup_im_col" in header and re.search(r"#define\s+PIL2GL_LOGUP_DIRECT\s+\(~\(uint64_t\)0\)", header)
    assert pilcheck.DIRECT == (1 << 64) - 1
    for f in ("logup_cluster_plan", "logup_cluster", "logup_cluster_dev", "range_logup_clustered"):
        assert callable(getattr(pilcheck, f))
    listed = full[full.index("only ENQUEUE work on that stream"):full.index("dev_upload_async / dev_download_async")]
    assert "logup_cluster and bn128_logup_cluster" in listed, "the header's list of enqueue-only calls"
    assert "logup_cluster_plan" in full[full.index("Calls that need no device"):full.index("Calls are not thread-safe")]


def test_im_col_layout_matches_the_header(tmp_path):
    exe = str(tmp_path / "dump")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", CSRC, os.path.join(ROOT, "tests", "logup_cluster_plan_dump.cpp"), "-o", exe])
    (tmp_path / "c.txt").write_text("layout\n")
    got = json.loads(subprocess.run([exe, str(tmp_path / "c.txt")], capture_output=True, text=True, check=True).stdout)
    T = _lib.LogupImCol
    assert got == dict(size=C.sizeof(T), base=T.base.offset, stride=T.stride.offset, col=T.col.offset) == dict(size=24, base=0, stride=8, col=16)


def test_plan_words(lib):
    for n in SHAPES:
        for field in ("gl", "bn128"):
            want, nbytes = cref.plan(n, field)
            logup = pilcheck.logup_sum_plan(n, 1, field)
            for n_f, n_r, n_im in ((1, 0, 1), (0, 8, 4), (8, 1, 9), (2, 0, 1), (5, 4, 3)):
                got = pilcheck.logup_cluster_plan(n, n_f, n_r, n_im, field)
                assert (got["threads"], got["items"], got["blocks"], got["launches"], got["depth"], got["outWidth"]) == want, (n, field)
                assert got["workBytes"] == nbytes, "the working memory grows with neither the terms nor nIm"
                if field == "gl":
                    assert got == logup, "cluster_scan1 keeps logup_scan1's geometry: eight rows a lane"
                elif n:
                    assert got["workBytes"] == logup["workBytes"] - 32 * n and got["launches"] == logup["launches"] + 1
    info = (C.c_uint32 * 6)()
    b = C.c_uint64(7)
    bad = (((1 << 28) + 1, 1, 0, 1, 1, b"2^28"), (8, 0, 0, 1, 1, b"1 .. 9"), (8, 8, 2, 1, 1, b"1 .. 9"), (8, 2, 8, 1, 4, b"1 .. 9"), (8, 9, 0, 1, 1, b"at most 8"),
           (8, 0, 9, 1, 1, b"at most 8"), (8, 1, 0, 0, 1, b"nIm"), (8, 1, 0, 10, 4, b"nIm"), (8, 1, 0, 1, 3, b"elemWords"), (8, 1, 0, 1, 0, b"elemWords"))
    for n, n_f, n_r, n_im, words, msg in bad:
        assert lib.pil2gl_logup_cluster_plan(n, n_f, n_r, n_im, words, info, C.byref(b)) == EINVAL and msg in lib.pil2gl_last_error(), (n, n_f, n_r, n_im, words)
        assert b.value == 0
    assert lib.pil2gl_logup_cluster_plan(8, 8, 1, 9, 1, info, C.byref(b)) == 0 and lib.pil2gl_logup_cluster_plan(8, 0, 8, 4, 4, info, C.byref(b)) == 0


# ---- the checker ----
def _sub(F, a, b):
    return F.add(a, F.mul(b, F.base(F.q - 1)))


def _rand_ext(rng, field):
    return tuple(rng.randrange(P) for _ in range(3)) if field == "gl" else rng.randrange(lref.FIELDS[field].q)


def _rand_case(rng, field, n, n_f, windows):
    q = lref.FIELDS[field].q
    terms = []
    for u in range(n_f):
        k = (1, 3, 16)[u % 3]
        terms.append(([[rng.randrange(q) for _ in range(k)] for _ in range(n)], [rng.randrange(4) for _ in range(n)] if u % 2 else None, rng.choice((1, q - 1, 5)), rng.randrange(q)))
    ranges = []
    for lo, size, row0 in windows:
        m = [rng.choice((0, 1, 2, rng.randrange(q))) if row0 <= i < row0 + size else None for i in range(n)]
        ranges.append((m, lo, size, row0, rng.choice((q - 1, 1)), rng.randrange(q)))
    return terms, ranges


CASES = ((3, ((-4, 9, 2),), [0, 0, D, 1]), (0, ((0, 5, 0), (7, 6, 5), (1 << 40, 11, 0), (-9, 3, 8)), [0, 0, 1, 1]), (4, (), [2, 0, 1, D]), (2, ((5, 11, 0),), [D, D, 0]))


@pytest.mark.parametrize("field", ("gl", "bn128"))
def test_checker_against_itself_and_the_plain_sums(field):
    """sum_c im_c + direct = s[i] - s[i-1]; s is logup_sum_ref's / range_sum_ref's on the same terms; im_c the differences of that sum on
    cluster c's terms alone"""
    F = lref.FIELDS[field]
    rng = random.Random(field)
    n = 11
    for n_f, windows, cluster in CASES:
        terms, ranges = _rand_case(rng, field, n, n_f, windows)
        alpha, beta = _rand_ext(rng, field), _rand_ext(rng, field)
        n_im = 1 + max(c for c in cluster if c != D)
        s, im = cref.cluster_sum(field, terms, ranges, cluster, n_im, alpha, beta, n)
        plain = rref.range_sum(field, terms, ranges, alpha, beta, n) if ranges else lref.logup_sum(field, terms, alpha, beta, n)
        assert s == plain
        dt, dr = cref.members(terms, ranges, cluster, D)
        direct = rref.range_sum(field, dt, dr, alpha, beta, n) if dt or dr else [F.zero] * n
        for i in range(n):
            inc = _sub(F, direct[i], direct[i - 1]) if i else direct[0]
            for c in range(n_im):
                inc = F.add(inc, im[c][i])
            assert inc == (_sub(F, s[i], s[i - 1]) if i else s[0])
        for c in range(n_im):
            ct, cr = cref.members(terms, ranges, cluster, c)
            sc = rref.range_sum(field, ct, cr, alpha, beta, n)
            assert im[c] == [_sub(F, sc[i], sc[i - 1]) if i else sc[0] for i in range(n)]


@pytest.mark.parametrize("field", ("gl", "bn128"))
def test_checker_meets_the_cleared_constraint(field):
    """im_c prod_u D_u - sum_u coef_u w_u prod_{v != u} D_v = 0 over cluster c's terms at rows without a zero denominator"""
    F = lref.FIELDS[field]
    rng = random.Random(field + "c")
    n = 9
    for n_f, windows, cluster in CASES:
        terms, ranges = _rand_case(rng, field, n, n_f, windows)
        alpha, beta = _rand_ext(rng, field), _rand_ext(rng, field)
        n_im = 1 + max(c for c in cluster if c != D)
        _, im = cref.cluster_sum(field, terms, ranges, cluster, n_im, alpha, beta, n)
        for c in range(n_im):
            ct, cr = cref.members(terms, ranges, cluster, c)
            for i in range(n):
                N, Dn, _ = rref.row_fraction(F, ct, cr, F.ext(alpha), F.ext(beta), i)
                assert _sub(F, F.mul(im[c][i], Dn), N) == F.zero


# ---- the entries' refusals, with no device ----
def _call(lib, words, n, terms, ranges, cluster, im, out, dev=True, alpha=True):
    """terms: (base, stride, cols); ranges: (m, stride, col, size, row0); im: (base, stride, col); out: (base, stride, col); bases are addresses"""
    T = (_lib.LogupTerm * 10)()
    keep = []
    for u, (base, stride, cols) in enumerate(terms):
        c = np.array(cols, np.uint64)
        keep.append(c)
        T[u].side = _lib.TupleSide(base, stride, c.ctypes.data, None, 0, 0)
        T[u].k = len(cols)
        T[u].coef[0] = 1
    Rg = (_lib.RangeTerm * 10)()
    for r, (m, stride, col, size, row0) in enumerate(ranges):
        Rg[r].m, Rg[r].mStride, Rg[r].mCol, Rg[r].lo, Rg[r].size, Rg[r].row0 = m, stride, col, 0, size, row0
        Rg[r].coef[0] = 1
    Im = (_lib.LogupImCol * 12)()
    for c, (base, stride, col) in enumerate(im or ()):
        Im[c].base, Im[c].stride, Im[c].col = base, stride, col
    cl = None if cluster is None else np.array(cluster, np.uint64)
    ch = np.array([1, 2, 3, 4], np.uint64)
    chp = C.c_void_p(ch.ctypes.data) if alpha else None
    name = ("pil2gl_logup_cluster" if words == 1 else "pil2gl_bn128_logup_cluster") + ("_dev" if dev else "")
    args = [T if terms else None, len(terms), Rg if ranges else None, len(ranges), None if cl is None else C.c_void_p(cl.ctypes.data), None if im is None else Im,
            2 if im is None else len(im), chp, chp, C.c_void_p(out[0]), out[1], out[2], n]
    if dev:
        args.append(None)
    return getattr(lib, name)(*args), lib.pil2gl_last_error()


A, B, M = 0x10000, 0x90000, 0x50000                  # matrices far apart: 8 rows of stride <= 16 elements stay below 0x1000 bytes over either field


@pytest.mark.parametrize("words", (1, 4))
def test_refusals_before_any_device_call(lib, words):
    w = 3 if words == 1 else 1
    n = 8
    t = [(A, 16, [0, 1]), (A, 16, [2])]
    r = [(M, 4, 0, 8, 0)]
    out, im = (B, 16, 0), [(B, 16, w), (B, 16, 2 * w)]
    good = dict(terms=t, ranges=r, cluster=[0, 1, D], im=im, out=out)

    def refused(msg, **kw):
        for dev in (True, False):
            rc, why = _call(lib, words, n, dev=dev, **dict(good, **kw))
            assert rc == EINVAL and msg in why, (kw, dev, rc, why)
    refused(b"has no term", cluster=[0, 0, D])                                 # an unused cluster id
    refused(b"0 .. nIm - 1", cluster=[0, 2, 1])                                # an id >= nIm
    refused(b"0 .. nIm - 1", cluster=[0, 1, (1 << 64) - 2])
    refused(b"null cluster", cluster=None)
    refused(b"nIm must be", im=[], cluster=[D, D, D])                          # nIm = 0
    refused(b"nIm must be", im=[(B, 16, 0)] * 10)                              # nIm = 10
    refused(b"null im", im=None)
    refused(b"1 .. 9", terms=[], ranges=[], cluster=[])                        # nF + nR = 0
    refused(b"1 .. 9", terms=t * 4, ranges=r * 2, cluster=[0] * 10)            # nF + nR = 10
    refused(b"two outputs overlap", im=[(B, 16, w), (B, 16, 2 * w - 1)] if words == 1 else [(B, 16, 1), (B, 16, 1)])     # two im columns share a word
    refused(b"two outputs overlap", im=[(B, 16, w - 1), (B, 16, 2 * w)])       # s and an im column share a word
    refused(b"two outputs overlap", im=[(B, 16, w), (B + 16, 16, 2 * w)])      # the same rows through another base
    refused(b"two outputs overlap", im=[(B, 16, w), (B, 15, 2 * w)])           # another stride
    refused(b"im 1: out overlaps a matrix that is read", im=[(B, 16, w), (A, 16, 1)])       # an im column on a read column
    refused(b"im 0: out overlaps an m matrix", im=[(M, 4, 0), (B, 16, 2 * w)])        # on m's own column
    refused(b"out overlaps a matrix that is read", out=(A, 16, 2))             # s on a read column
    if words == 1:
        refused(b"im 1: a column >= stride", im=[(B, 16, w), (B, 16, 14)])     # col + 2 >= stride
    refused(b"im 1: a column >= stride", im=[(B, 16, w), (B, 16, 16)])
    refused(b"im 0: stride >= 2^32", im=[(B, 1 << 32, w), (B, 16, 2 * w)])
    refused(b"null buffer", im=[(0, 16, w), (B, 16, 2 * w)])
    refused(b"null alpha", alpha=False)
    rc, why = _call(lib, words, n, **dict(good, im=[(B + 8, 16, w), (B, 16, 2 * w)]))
    assert rc == EINVAL and b"16-byte aligned" in why                          # a misaligned base: the resident form only
    rc, why = _call(lib, words, n, **dict(good, out=(B + 8, 16, 0)))
    assert rc == EINVAL and b"16-byte aligned" in why
    # accepted by the checks: s and the im columns in ONE matrix, and as spare columns of t's matrix; then the device is missing or the call runs
    if not _have_gpu():
        for kw in (good, dict(good, out=(A, 16, 3), im=[(A, 16, 3 + w), (A, 16, 3 + 2 * w)]), dict(good, im=[(B, 16, 2 * w), (B, 16, w)])):
            for dev in (True, False):
                rc, why = _call(lib, words, n, dev=dev, **kw)
                assert rc == ENODEV, (kw, rc, why)
    # n = 0 is OK, touches nothing and needs no device; hostTerms may be null when nF = 0 and hostRanges when nR = 0
    for kw in (good, dict(good, terms=[], cluster=[0], im=im[:1]), dict(good, ranges=[], cluster=[0, 1])):
        for dev in (True, False):
            rc, why = _call(lib, words, 0, dev=dev, **dict(kw, out=(0, 16, 0), im=[(0, 16, w), (0, 16, 2 * w)][:len(kw["im"])]))
            assert rc == 0, (kw, rc, why)


def test_planner_under_sanitizers(tmp_path):
    """the output rule over edge strides and the 2^58 span, in a program of its own: no sanitizer on anything loaded into Python"""
    exe = str(tmp_path / "dump_san")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                           os.path.join(ROOT, "tests", "logup_cluster_plan_dump.cpp"), "-o", exe])
    big = 1 << 28
    lines, want = [], []

    def add(line, **kv):
        lines.append(line)
        want.append(kv)
    for n in SHAPES:
        for ew, field in ((1, "gl"), (4, "bn128")):
            info, nbytes = cref.plan(n, field)
            add("plan %d 2 1 2 %d" % (n, ew), ok=1, threads=info[0], items=info[1], blocks=info[2], launches=info[3], depth=info[4], width=info[5], bytes=nbytes)
    add("plan 8 0 0 1 1", ok=0)
    add("plan 8 1 0 10 1", ok=0)
    # call n words tBase tStride oBase oStride oCol nIm (imBase imStride imCol)..
    add("call 8 1 65536 16 589824 16 0 2 589824 16 3 589824 16 6", ok=1)                 # one matrix, neighbouring columns
    add("call 8 1 65536 16 65536 16 2 2 65536 16 5 65536 16 8", ok=1)                    # spare columns of t's matrix
    add("call 8 1 65536 16 65536 16 2 1 65536 16 4", ok=0)                               # s and im share word column 4
    add("call 8 1 65536 16 65536 16 2 1 65536 16 0", ok=0)                               # im on a read column (its word 1)
    add("call 8 4 65536 16 65536 16 2 1 65536 16 3", ok=1)
    add("call 8 4 65536 16 65536 16 2 1 65536 16 2", ok=0)
    add("call 8 1 65536 16 589824 16 0 1 589824 16 13", ok=1)                            # col + 2 = stride - 1
    add("call 8 1 65536 16 589824 16 0 1 589824 16 14", ok=0)                            # col + 2 = stride
    add("call 8 1 65536 16 589824 16 0 1 1048576 4294967295 4294967292", ok=1)           # the widest stride
    add("call 8 1 65536 16 589824 16 0 1 1048576 4294967296 3", ok=0)
    add("call %d 1 65536 3 4611686018427387904 4 0 1 6917529027641081856 1073741824 5" % big, ok=1)        # n stride = 2^58 exactly
    add("call %d 1 65536 3 4611686018427387904 4 0 1 6917529027641081856 1073741825 5" % big, ok=0)        # above it
    add("call 8 1 65536 16 589824 16 0 1 589832 16 3", ok=0)                             # a misaligned im base
    add("call 8 1 65536 16 589824 16 0 1 0 16 3", ok=0)                                  # a null one
    # apart n words aBase aStride aCol bBase bStride bCol
    add("apart 8 1 4096 16 0 4096 16 3", apart=1)
    add("apart 8 1 4096 16 0 4096 16 2", apart=0)
    add("apart 8 1 4096 16 3 4096 16 0", apart=1)
    add("apart 8 1 4096 16 0 4096 17 8", apart=0)
    add("apart 8 1 4096 16 0 4104 16 8", apart=0)
    add("apart 8 1 4096 16 0 5096 16 0", apart=1)                                        # behind the last word written: (7 * 16 + 3) * 8 = 920 bytes
    add("apart 8 1 4096 16 0 5015 16 0", apart=0)
    add("apart 8 4 4096 16 0 4096 16 1", apart=1)
    add("apart 8 4 4096 16 1 4096 16 1", apart=0)
    add("apart 1 1 4096 4294967295 0 4096 4294967295 4294967292", apart=1)
    # groups n words oBase oStride oCol nIm (imBase imStride imCol)..: one matrix staged once, to the last word any output writes
    add("groups 8 1 4096 16 0 3 4096 16 6 8192 5 1 4096 16 3", group=[0, 0, 2, 0], words=[7 * 16 + 9, 0, 7 * 5 + 4, 0])
    add("groups 8 4 4096 16 5 1 4096 16 2", group=[0, 0], words=[(7 * 16 + 6) * 4, 0])
    (tmp_path / "c.txt").write_text("\n".join(lines) + "\n")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([exe, str(tmp_path / "c.txt")], capture_output=True, text=True, env=env)
    assert out.returncode == 0, out.stderr[-3000:]
    got = [json.loads(line) for line in out.stdout.splitlines()]
    assert len(got) == len(want)
    for line, g, w in zip(lines, got, want):
        for k, v in w.items():
            assert g[k] == v, (line, g)
