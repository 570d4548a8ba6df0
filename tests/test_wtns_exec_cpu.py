"""The recursion witness expansion without a device: the checker (tests/wtns_exec_ref.py) against a second formulation of itself, the file
readers of pil2gl.wtns against the checker's writers, the planner through the library's host-only call, the ABI surface (every refusal
before any device call, ENODEV otherwise), and the planner header and the header it shares with the connection polynomials under the
sanitizers, each in a program of its own.
The reference tree ships no .exec or .wtns and its setups need pilcom / circom_runtime, which are not available, so no reference-written
fixture exists; the writers restate writeExecFile (compressor/exec_helpers.js:26-47, final/exec_helpers.js:93-187)."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import wtns_exec_ref as ref
from wtns_exec_ref import P, R
from conftest import ROOT

import pil2gl  # noqa: E402  (a plain import: without the feature, or with a broken build, this file fails)
from pil2gl import _lib, wtns  # noqa: E402

CSRC = os.path.join(ROOT, "pil2-stark-js_amd", "csrc")
EINVAL, ENODEV = -1, -2


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _have_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


def flat(adds):
    return np.array([x for r in adds for x in r], np.uint64)


def plan_of(adds, n_witness):
    t = flat(adds)
    return wtns.adds_plan(t, n_witness, t[2:], 1, 4, 4)


# ---- the checker against a second formulation ----
@pytest.mark.parametrize("q", [P, R])
def test_level_order_gives_the_serial_result_on_random_dags(q):
    for seed in range(30):
        rng = ref.rng(seed)
        n_w = rng.randrange(1, 12)
        adds = ref.random_dag(rng, n_w, rng.randrange(0, 80), q, back=rng.random())
        w = [rng.randrange(q) for _ in range(n_w)]
        assert ref.additions(w, adds, q) == ref.additions_by_level(w, adds, q), seed


# ---- file formats ----
def test_exec_and_wtns_readers_against_the_writers(tmp_path):
    rng = ref.rng(1)
    adds = ref.random_dag(rng, 9, 17, P)
    s_map = [rng.randrange(9 + 17) for _ in range(8 * 5)]
    path = str(tmp_path / "c12.exec")
    ref.write_compressor_exec(path, adds, s_map, 8, 5)
    e = wtns.read_exec_file(path, 5, "gl")
    assert (e["nAdds"], e["nSMap"], e["nCols"], e["field"]) == (17, 8, 5, "gl")
    assert e["adds"].tolist() == flat(adds).tolist() and e["sMap"].tolist() == s_map
    adds_r = ref.random_dag(rng, 9, 17, R)
    path = str(tmp_path / "final.exec")
    ref.write_final_exec(path, adds_r, s_map, 8, 5)
    e = wtns.read_exec_file(path, 5, "bn128")
    assert (e["nAdds"], e["nSMap"]) == (17, 8) and e["sMap"].tolist() == s_map
    assert e["addsIdx"].tolist() == [x for a, b, _, _ in adds_r for x in (a, b)]
    assert ref.fr_ints(e["addsCoef"]) == [ref.to_mont(c) for _, _, ca, cb in adds_r for c in (ca, cb)]
    w = [rng.randrange(R) for _ in range(9)] + [R - 1, 0]
    path = str(tmp_path / "final.wtns")
    ref.write_wtns(path, w)
    got = wtns.read_wtns(path)
    assert (got["n8"], got["prime"], got["nWitness"]) == (32, R, 11) and ref.fr_ints(got["w"]) == w
    ref.write_wtns(path, [5, P - 1], P, 8)
    got = wtns.read_wtns(path)
    assert (got["n8"], got["prime"]) == (8, P) and got["w"].reshape(-1).tolist() == [5, P - 1]


def test_truncated_files_are_refused_with_name_found_and_expected_size(tmp_path):
    rng = ref.rng(2)
    adds = ref.random_dag(rng, 9, 4, P)
    s_map = list(range(12))
    cases = []
    path = str(tmp_path / "c.exec")
    ref.write_compressor_exec(path, adds, s_map, 4, 3)
    cases.append((path, lambda p: wtns.read_exec_file(p, 3, "gl"), 8 * (2 + 16 + 12)))
    path = str(tmp_path / "f.exec")
    ref.write_final_exec(path, adds, s_map, 4, 3)
    cases.append((path, lambda p: wtns.read_exec_file(p, 3, "bn128"), os.path.getsize(path)))
    path = str(tmp_path / "w.wtns")
    ref.write_wtns(path, [1, 2, 3])
    cases.append((path, wtns.read_wtns, os.path.getsize(path)))
    for path, read, full in cases:
        assert os.path.getsize(path) == full
        read(path)
        with open(path, "r+b") as f:
            f.truncate(full - 5)
        with pytest.raises(pil2gl.Pil2glError) as e:
            read(path)
        msg = str(e.value)
        assert path in msg and "%d bytes found" % (full - 5) in msg and "%d expected" % full in msg, msg
    # a compressor file read with more columns than it was written with is short, too
    path = str(tmp_path / "c2.exec")
    ref.write_compressor_exec(path, adds, s_map, 4, 3)
    with pytest.raises(pil2gl.Pil2glError, match="%d bytes found, %d expected" % (8 * 30, 8 * 34)):
        wtns.read_exec_file(path, 4, "gl")


# ---- the planner through the host-only call ----
def test_levels_of_a_hand_made_case():
    """nWitness = 4 (signals 0..3); additions, with the signal each defines:
         0 (4): w0, w1           level 0
         1 (5): s4, w2           level 1      -- one operand an addition
         2 (6): w3, w3           level 0
         3 (7): s5, s6           level 2      -- two additions of different levels: 1 + the higher
         4 (8): s4, s6           level 1
         5 (9): s7, s7           level 3
       sorted by level, stable: 0 2 | 1 4 | 3 | 5, levelStart 0 2 4 5 6"""
    adds = [(0, 1, 11, 12), (4, 2, 13, 14), (3, 3, 15, 16), (5, 6, 17, 18), (4, 6, 19, 20), (7, 7, 21, 22)]
    p = plan_of(adds, 4)
    assert p["nLevels"] == 4 and p["levelStart"].tolist() == [0, 2, 4, 5, 6]
    assert p["adds"].tolist() == [[0, 1, 4, 0], [3, 3, 6, 2], [4, 2, 5, 1], [4, 6, 8, 4], [5, 6, 7, 3], [7, 7, 9, 5]]
    assert p["coefs"].tolist() == [11, 12, 15, 16, 13, 14, 19, 20, 17, 18, 21, 22]
    info = wtns.plan_info(flat(adds), 4, 4)
    assert (info["levels"], info["launches"], info["widest"], info["widths"]) == (4, 4, 2, [2, 2, 1, 1])
    # Fr-shaped tables: two indices an addition, two 4-word coefficients
    idx = np.array([x for a, b, _, _ in adds for x in (a, b)], np.uint64)
    coef = np.arange(8 * len(adds), dtype=np.uint64)
    q = wtns.adds_plan(idx, 4, coef, 4)
    assert q["adds"].tolist() == p["adds"].tolist() and q["levelStart"].tolist() == p["levelStart"].tolist()
    assert q["coefs"].reshape(-1, 8).tolist() == [list(range(8 * i, 8 * i + 8)) for i in (0, 2, 1, 4, 3, 5)]


def test_planner_matches_the_checker_and_is_stable():
    for seed in range(20):
        rng = ref.rng(100 + seed)
        n_w = rng.randrange(1, 9)
        adds = ref.random_dag(rng, n_w, rng.randrange(1, 200), P, back=rng.random())
        recs, start, order = ref.plan(adds, n_w)
        p = plan_of(adds, n_w)
        assert [tuple(r) for r in p["adds"].tolist()] == recs and p["levelStart"].tolist() == start
        assert p["coefs"].tolist() == [c for i in order for c in adds[i][2:]]
        for l in range(p["nLevels"]):
            pos = p["adds"][start[l]:start[l + 1], 3].tolist()
            assert pos == sorted(pos) and pos, "source order within a level, no empty level"


def test_deep_chain_queue_reduction_and_empty_table():
    chain = [(0, 1, 2, 3)] + [(2 + i, 0, 1, 1) for i in range(299)]
    info = wtns.plan_info(flat(chain), 2, 4)
    assert info["levels"] == 300 and info["launches"] == 300 and info["widths"] == [1] * 300
    comb = ref.queue_reduction(list(range(33)), 40)
    assert len(comb) == 32
    assert wtns.plan_info(flat(comb), 40, 4)["levels"] == 6                 # ceil(log2 33)
    p = wtns.adds_plan(np.zeros(0, np.uint64), 7)
    assert p["nLevels"] == 0 and p["levelStart"].tolist() == [0] and p["adds"].shape == (0, 4)


def test_planner_refusals(lib):
    n = C.c_uint32(99)
    for k, bad in ((2, 5 + 2), (2, 5 + 3), (0, 5), (4, 1 << 33)):            # self, forward, self at 0, far away
        adds = [(0, 1, 1, 1)] * 5
        adds[k] = (1, bad, 1, 1)
        with pytest.raises(pil2gl.Pil2glError, match=r"error -1: addition %d: operand b = %d" % (k, bad)):
            plan_of(adds, 5)
    t = flat([(0, 1, 1, 1)])
    tp = t.ctypes.data_as(C.c_void_p)
    assert lib.pil2gl_wtns_adds_plan(tp, 4, 1, (1 << 32) - 1, None, 0, 1, None, None, None, 0, C.byref(n)) == EINVAL       # nW = 2^32
    assert b"2^32" in lib.pil2gl_last_error() and n.value == 0
    assert lib.pil2gl_wtns_adds_plan(tp, 4, 1, (1 << 32) - 2, None, 0, 1, None, None, None, 0, C.byref(n)) == 0 and n.value == 1
    assert lib.pil2gl_wtns_adds_plan(tp, 4, 1, 2, None, 0, 2, None, None, None, 0, C.byref(n)) == EINVAL                 # coefWords
    assert lib.pil2gl_wtns_adds_plan(tp, 1, 1, 2, None, 0, 1, None, None, None, 0, C.byref(n)) == EINVAL                 # idxStride
    assert lib.pil2gl_wtns_adds_plan(None, 4, 1, 2, None, 0, 1, None, None, None, 0, C.byref(n)) == EINVAL
    assert lib.pil2gl_wtns_adds_plan(tp, 4, 1, 2, None, 0, 1, None, None, None, 0, None) == EINVAL
    recs = (C.c_uint32 * 4)(); start = (C.c_uint32 * 2)()
    assert lib.pil2gl_wtns_adds_plan(tp, 4, 1, 2, None, 0, 1, recs, None, start, 1, C.byref(n)) == EINVAL                # levelCap
    assert lib.pil2gl_wtns_adds_plan(tp, 4, 1, 2, None, 0, 1, recs, None, None, 2, C.byref(n)) == EINVAL
    assert lib.pil2gl_wtns_adds_plan(tp, 4, 1, 2, None, 0, 1, recs, None, start, 2, C.byref(n)) == 0 and list(start) == [0, 1]
    assert lib.pil2gl_debug_wtns_plan(tp, 4, 1, 2, None, None, 0) == EINVAL


# ---- the ABI: every refusal before any device call ----
def test_compute_entries_refuse_before_any_device_call(lib):
    buf = np.zeros(64, np.uint64)
    a = buf.ctypes.data
    start = (C.c_uint32 * 2)(0, 1)
    stream = None
    # additions: null pointers, a level table that does not tile, w inside a table, nW = 2^32
    assert lib.pil2gl_wtns_adds_dev(None, 2, a + 128, a + 256, 1, start, 1, stream) == EINVAL
    assert lib.pil2gl_wtns_adds_dev(a, 2, None, a + 256, 1, start, 1, stream) == EINVAL
    assert lib.pil2gl_wtns_adds_dev(a, 2, a + 128, a + 256, 1, None, 1, stream) == EINVAL
    assert lib.pil2gl_wtns_adds_dev(a, 2, a + 128, a + 256, 2, start, 1, stream) == EINVAL
    assert lib.pil2gl_bn128_wtns_adds_dev(a, 2, a + 64, a + 256, 1, start, 1, stream) == EINVAL and b"overlaps" in lib.pil2gl_last_error()
    assert lib.pil2gl_wtns_adds_dev(a, 2, a + 16, a + 256, 1, start, 1, stream) == EINVAL and b"overlaps" in lib.pil2gl_last_error()
    assert lib.pil2gl_wtns_adds_dev(a, 2, a + 132, a + 256, 1, start, 1, stream) == EINVAL and b"aligned" in lib.pil2gl_last_error()
    assert lib.pil2gl_wtns_adds_dev(a, (1 << 32) - 1, a + 128, a + 256, 1, start, 1, stream) == EINVAL
    assert lib.pil2gl_wtns_adds_dev(a, 2, None, None, 0, None, 0, stream) == 0                                          # nothing to do, no device
    # gather: dstCols < nCols, nW, null pointers, overlap
    bad = C.c_uint64(5)
    for fn, tail in ((lib.pil2gl_wtns_gather_dev, ()), (lib.pil2gl_bn128_wtns_gather_dev, (1,))):
        assert fn(a, 4, a + 256, 2, 3, a + 320, 2, *tail, C.byref(bad), stream) == EINVAL and bad.value == (1 << 64) - 1
        assert fn(a, 1 << 32, a + 256, 2, 3, a + 320, 3, *tail, None, stream) == EINVAL
        assert fn(None, 4, a + 256, 2, 3, a + 320, 3, *tail, None, stream) == EINVAL
        assert fn(a, 4, None, 2, 3, a + 320, 3, *tail, None, stream) == EINVAL
        assert fn(a, 4, a + 256, 2, 3, None, 3, *tail, None, stream) == EINVAL
        assert fn(a, 4, a + 256, 2, 3, a + 16, 3, *tail, None, stream) == EINVAL and b"overlaps" in lib.pil2gl_last_error()
        assert fn(a, 4, a + 256, 2, 3, a + 240, 3, *tail, None, stream) == EINVAL and b"overlaps" in lib.pil2gl_last_error()
        assert fn(a, 4, a + 256, 0, 3, a + 320, 3, *tail, C.byref(bad), stream) == 0 and bad.value == (1 << 64) - 1      # no rows, no device
    # the host forms
    w = np.array([1, 2, 3], np.uint64)
    tab = flat([(0, 1, 1, 1), (3, 2, 1, 1)])
    s_map = np.array([0, 4, 1, 2], np.uint64)
    dst = np.zeros(4, np.uint64)
    p = lambda x: x.ctypes.data                                                                                        # noqa: E731
    ok = (p(w), 3, p(tab), p(tab) + 16, 2, p(s_map), 2, 2, p(dst))
    assert lib.pil2gl_wtns_exec(None, *ok[1:]) == EINVAL
    assert lib.pil2gl_wtns_exec(*ok[:8], None) == EINVAL
    assert lib.pil2gl_wtns_exec(*ok[:5], None, *ok[6:]) == EINVAL
    assert lib.pil2gl_wtns_exec(*ok[:8], p(w)) == EINVAL and b"overlaps" in lib.pil2gl_last_error()
    s_bad = np.array([0, 4, 5, 2], np.uint64)
    assert lib.pil2gl_wtns_exec(*ok[:5], p(s_bad), *ok[6:]) == EINVAL and b"sMap[2] = 5" in lib.pil2gl_last_error()
    t_bad = flat([(0, 1, 1, 1), (4, 2, 1, 1)])
    assert lib.pil2gl_wtns_exec(*ok[:2], p(t_bad), p(t_bad) + 16, *ok[4:]) == EINVAL and b"addition 1" in lib.pil2gl_last_error()
    assert lib.pil2gl_wtns_exec(p(w), (1 << 32) - 2, *ok[2:]) == EINVAL and b"2^32" in lib.pil2gl_last_error()
    if not _have_gpu():
        assert lib.pil2gl_wtns_exec(*ok) == ENODEV
        w4 = np.zeros(12, np.uint64); c4 = np.zeros(32, np.uint64); d4 = np.zeros(16, np.uint64)
        idx = np.array([0, 1, 3, 2], np.uint64)
        assert lib.pil2gl_bn128_wtns_exec(p(w4), 3, p(idx), p(c4), 2, p(s_map), 2, 2, p(d4), 1) == ENODEV
        assert lib.pil2gl_wtns_adds_dev(a, 2, a + 128, a + 256, 1, start, 1, stream) == ENODEV
        assert lib.pil2gl_wtns_gather_dev(a, 4, a + 256, 2, 3, a + 320, 3, None, stream) == ENODEV
        assert lib.pil2gl_bn128_wtns_gather_dev(a, 2, a + 256, 1, 1, a + 320, 1, 1, None, stream) == ENODEV
        with pytest.raises(pil2gl.Pil2glError, match="-2"):
            wtns.exec_gl(w, {"field": "gl", "adds": tab, "nAdds": 2, "nSMap": 2, "nCols": 2, "sMap": s_map})


# ---- the planner headers under the sanitizers, each in a program of its own ----
def test_shared_smap_header_under_the_sanitizers(tmp_path):
    """csrc/smap_plan.h: the narrowing of a host sMap in both layouts against a transposition made here, the overlap test, the grid"""
    exe = str(tmp_path / "smap_plan_dump")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                           os.path.join(ROOT, "tests", "smap_plan_dump.cpp"), "-o", exe])
    rng = ref.rng(900)
    narrow = []                                                               # (colsU32, colLen, nRows, nCols, nW, values in memory order, rows)
    for n_rows, n_cols in ((4, 3), (5, 3), (1, 1), (7, 6), (0, 3), (3, 0)):   # 15 and 1 cells are odd counts: a padding half-word
        n_w = 1 << 20
        rows = [[rng.randrange(n_w) for _ in range(n_cols)] for _ in range(n_rows)]
        narrow.append((0, 0, n_rows, n_cols, n_w, [v for r in rows for v in r], rows))
        col_len = n_rows + 3                                                  # the setups' columns are N long, rows past nRows are not read
        cols = [[rows[i][j] if i < n_rows else 0xFFFFFFFF for i in range(col_len)] for j in range(n_cols)]
        narrow.append((1, col_len, n_rows, n_cols, n_w, [v for c in cols for v in c], rows))
    refused = [((0, 0, 2, 3, 9, [1, 2, 3, 4, 9, 0]), (4, 9)),                 # a value equal to nW, at its position; cell 5 is never read
               ((0, 0, 2, 2, 3, [1, 2, (1 << 32) + 1, 0]), (2, (1 << 32) + 1)),  # the 64-bit value decides: its low half, 1, names a signal
               ((1, 2, 2, 2, 9, [1, 2, 9, 4]), (1, 9)),                       # columns of u32: memory position 2 is row 0, column 1 = cell 1
               ((0, 0, 1, 2, 1, [0, 1]), (1, 1))]
    accepted = (0, 0, 1, 3, 9, [8, 0, 8], [[8, 0, 8]])                        # nW - 1
    meets = [((0, 0, 0, 8), 0), ((0, 8, 4, 0), 0), ((8, 0, 8, 0), 0),         # a zero length on either side, inside the other range or not
             ((0, 8, 8, 8), 0), ((8, 8, 0, 8), 0),                            # touching
             ((0, 9, 8, 8), 1), ((8, 8, 0, 9), 1), ((0, 64, 20, 1), 1), ((0, 8, 16, 8), 0)]      # one byte shared, either order; inside; apart
    blocks = [(0, 1), (1, 1), (256, 1), (257, 2), (2048 * 256, 2048), (2048 * 256 + 1, 2048), (1 << 40, 2048)]
    with open(tmp_path / "cmds.txt", "w") as f:
        f.write("consts\n")
        for c in narrow + [accepted] + [r for r, _ in refused]:
            f.write("narrow %d %d %d %d %d %s\n" % (*c[:5], " ".join(map(str, c[5]))))
        f.write("".join("meets %d %d %d %d\n" % m for m, _ in meets) + "".join("blocks %d\n" % b for b, _ in blocks))
    run = subprocess.run([exe, str(tmp_path / "cmds.txt")], capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", "sanitizer report:\n" + run.stderr[-4000:]
    out = [json.loads(l) for l in run.stdout.splitlines()]
    assert out[0] == {"threads": 256, "maxBlocks": 2048} and len(out) == 1 + len(narrow) + 1 + len(refused) + len(meets) + len(blocks)
    for c, got in zip(narrow + [accepted], out[1:]):
        flat = [v for r in c[6] for v in r]
        halves = [h for word in got["words"] for h in (word & 0xFFFFFFFF, word >> 32)]
        assert got["ok"] == 1 and len(got["words"]) == ((len(flat) + 1) // 2 + 1) // 2 * 2, c[:5]     # whole words, an even number of them
        assert halves[:len(flat)] == flat and not any(halves[len(flat):]), c[:5]
    at = 2 + len(narrow)
    for (c, (cell, value)), got in zip(refused, out[at:]):
        assert got == {"ok": 0, "cell": cell, "value": value}, c
    at += len(refused)
    assert [g["meets"] for g in out[at:at + len(meets)]] == [m for _, m in meets]
    assert [g["blocks"] for g in out[at + len(meets):]] == [b for _, b in blocks]


def test_planner_header_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "wtns_plan_dump")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                           os.path.join(ROOT, "tests", "wtns_plan_dump.cpp"), "-o", exe])
    cases = []
    for seed in range(25):
        rng = ref.rng(500 + seed)
        n_w = rng.randrange(1, 9)
        cases.append((n_w, ref.random_dag(rng, n_w, rng.randrange(0, 120), P, back=rng.random())))
    cases.append((2, [(0, 1, 2, 3)] + [(2 + i, 0, 1, 1) for i in range(299)]))
    cases.append((40, ref.queue_reduction(list(range(33)), 40)))
    cases.append((3, [(0, 1, 1, 1), (5, 1, 1, 1)]))                            # a forward reference
    cases.append(((1 << 32) - 1, [(0, 1, 1, 1)]))                              # nW = 2^32
    with open(tmp_path / "cases.txt", "w") as f:
        for n_w, adds in cases:
            f.write("%d %d\n" % (n_w, len(adds)) + "".join("%d %d %d %d\n" % r for r in adds))
    run = subprocess.run([exe, str(tmp_path / "cases.txt")], capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", "sanitizer report or a broken invariant:\n" + run.stderr[-4000:]
    out = [json.loads(l) for l in run.stdout.splitlines()]
    assert len(out) == len(cases)
    for (n_w, adds), got in zip(cases[:-2], out):
        recs, start, order = ref.plan(adds, n_w)
        assert got["ok"] == 1 and got["nLevels"] == len(start) - 1 and got["levelStart"] == start
        assert got["adds"] == [x for r in recs for x in r] and got["coefs"] == [c for i in order for c in adds[i][2:]]
    assert out[-3]["nLevels"] == 6 and out[-4]["nLevels"] == 300
    assert out[-2]["ok"] == 0 and "addition 1: operand a = 5" in out[-2]["error"]
    assert out[-1]["ok"] == 0 and "2^32" in out[-1]["error"]
