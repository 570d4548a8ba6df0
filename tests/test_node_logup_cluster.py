"""The clustered logUp sum from Node: js/pil_checks.js logupCluster (host matrices as words and as bytes) and logupClusterDev (DevBuffer
sections), js/polutils.js and js/polutils_bn128.js calculateSClustered / calculateSClusteredDev, both fields, on a case file written here:
every word of every matrix after the call, from the checker (tests/logup_cluster_ref.py), which the Python forms are tested against too.
One small case a field: two f terms and two ranges on one m matrix, a cluster of an f term and a range, a cluster of a range, a DIRECT
term; s and the im columns as spare columns of m's matrix, in descending order with a column between them that must survive.  Also the
addon's layout of pil2gl_logup_im_col against the ctypes struct and the header's, and its surface, which need no device.  Node runs as a
fresh child process."""
import ctypes as C
import json
import os
import random
import shutil
import subprocess

import numpy as np
import pytest

import logup_cluster_ref as lcref
import bn128_hints_ref as bref
import conn_pols_ref as cref
from hints_ref import P
from conftest import ROOT
from test_node_range_sum import words, value, elem_hex, chal_hex

from pil2gl import _lib, pilcheck

NODE = shutil.which("node")
R, MONT = bref.R, bref.MONT
CSRC = os.path.join(ROOT, "pil2-stark-js_amd", "csrc")


def _layout():
    T = _lib.LogupImCol
    return dict(size=C.sizeof(T), base=T.base.offset, stride=T.stride.offset, col=T.col.offset)


@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_im_col_layout_matches_what_the_addon_and_the_header_state(tmp_path):
    """the ctypes struct against sizeof / offsetof as the ADDON was compiled (a fresh Node child; no device needed) and as the header
    compiles, and the addon's surface"""
    js = "const a = require(%r).addon; console.log(JSON.stringify([a.logupImColLayout()].concat(['logupClusterPlan', 'logupClusterDev', 'logupCluster'].map((f) => typeof a[f])).concat([a.logupClusterPlan(2049, 0, 8, 4, 1), a.logupClusterPlan(2049, 8, 1, 9, 4)])));"
    out = subprocess.run([NODE, "-e", js % os.path.join(ROOT, "pil2-stark-js_amd", "js", "native.js")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    got = json.loads(out.stdout)
    assert got[0] == _layout()
    assert got[1:4] == ["function"] * 3
    assert got[4] == pilcheck.logup_cluster_plan(2049, 0, 8, 4, "gl") and got[5] == pilcheck.logup_cluster_plan(2049, 8, 1, 9, "bn128")
    exe = str(tmp_path / "dump")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", CSRC, os.path.join(ROOT, "tests", "logup_cluster_plan_dump.cpp"), "-o", exe])
    (tmp_path / "c.txt").write_text("layout\n")
    assert json.loads(subprocess.run([exe, str(tmp_path / "c.txt")], capture_output=True, text=True, check=True).stdout) == got[0]
    src = open(os.path.join(ROOT, "pil2-stark-js_amd", "js", "pil_checks.js")).read()
    assert "logupCluster, logupClusterDev, logupClusterPlan" in src[src.index("module.exports = {"):]
    for f in ("polutils.js", "polutils_bn128.js"):
        src = open(os.path.join(ROOT, "pil2-stark-js_amd", "js", f)).read()
        assert "calculateSClustered" in src and "calculateSClusteredDev" in src, f


def case(name, field, mats, terms, ranges, cluster, im, alpha, beta, out):
    """test_node_range_sum.case's arguments, with cluster (ids, or "D") and im: {"mat", "col"} a cluster"""
    n = len(mats[out["mat"]])
    width = 3 if field == "gl" else 1
    ref_terms = []
    for t in terms:
        tuples = [[value(field, row[c]) for c in t["cols"]] for row in mats[t["mat"]]]
        w = None if not t.get("sel") else [value(field, row[t["sel"]["col"]]) for row in mats[t["sel"]["mat"]]]
        ref_terms.append((tuples, w, t["coef"], t["busId"]))
    ref_ranges = [([value(field, mats[r["mat"]][i][r["col"]]) if r["row0"] <= i < r["row0"] + r["size"] else None for i in range(n)], r["lo"], r["size"], r["row0"],
                   r["coef"], r["busId"]) for r in ranges]
    s, ims = lcref.cluster_sum(field, ref_terms, ref_ranges, [lcref.DIRECT if c == "D" else c for c in cluster], len(im), alpha, beta, n)
    after = {k: words(field, rows).copy() for k, rows in mats.items()}
    for o, col in [(out, s)] + list(zip(im, ims)):
        w = np.array(col, np.uint64).reshape(n, 3) if field == "gl" else cref.fr_words([v * MONT % R for v in col]).reshape(n, 1, 4)
        after[o["mat"]][:, o["col"]:o["col"] + width] = w
    plan = lcref.plan(n, field)[0]
    return {"name": name, "field": field, "n": n, "mats": {k: {"words": words(field, rows).tobytes().hex(), "stride": len(rows[0])} for k, rows in mats.items()},
            "terms": [dict(t, coef=elem_hex(field, t["coef"]), busId=elem_hex(field, t["busId"])) for t in terms],
            "ranges": [dict(r, lo=str(r["lo"]), coef=elem_hex(field, r["coef"]), busId=elem_hex(field, r["busId"])) for r in ranges], "cluster": cluster, "im": im,
            "alpha": chal_hex(field, alpha), "beta": chal_hex(field, beta), "out": out, "after": {k: w.tobytes().hex() for k, w in after.items()}, "plan": [plan[3], plan[5]]}


@pytest.mark.gpu
@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_js_logup_cluster_matches_the_checker(tmp_path):
    cases = []
    for field, q in (("gl", P), ("bn128", R)):
        rng = random.Random(81 if field == "gl" else 83)
        n, width = 80, 3 if field == "gl" else 1
        top = (1 << 64) if field == "gl" else (1 << 256)
        # M: two multiplicity columns, non-zero in every row and past the modulus in some, then room for im_1, a column that must survive, s, im_0
        mm = [[1 + rng.randrange(q - 1) + (q if i % 3 == 0 and 2 * q < top else 0), 1 + rng.randrange(5)] + [q - 9 - j for j in range(3 * width + 1)] for i in range(n)]
        f0 = [[rng.randrange(q), rng.randrange(q), i % 3] for i in range(n)]
        alpha = tuple(rng.randrange(P) for _ in range(3)) if field == "gl" else rng.randrange(R)
        beta = tuple(rng.randrange(P) for _ in range(3)) if field == "gl" else rng.randrange(R)
        R0 = {"mat": "M", "col": 0, "lo": -3, "size": 38, "row0": 13, "coef": q - 1, "busId": 6}       # rows 13 .. 50: both ends mid-lane, crosses zero
        R1 = {"mat": "M", "col": 1, "lo": (1 << 63) - 20, "size": 20, "row0": 60, "coef": 5, "busId": 7}
        F0 = {"mat": "F0", "cols": [1, 0], "sel": {"mat": "F0", "col": 2}, "coef": 1, "busId": 6}
        K1 = {"mat": "F0", "cols": [1], "sel": None, "coef": 1, "busId": 7}
        im = [{"mat": "M", "col": 3 + 2 * width}, {"mat": "M", "col": 2}]
        cases.append(case(field + " two f terms and two ranges, s and two im columns in m's matrix", field, {"M": mm, "F0": f0}, [F0, K1], [R0, R1], [0, "D", 0, 1], im,
                          alpha, beta, {"mat": "M", "col": 3 + width}))
        own = {"M": mm, "S": [[q - 1 - i - j for j in range(width + 2)] for i in range(n)], "I": [[q - 50 - i - j for j in range(width + 1)] for i in range(n)]}
        cases.append(case(field + " no f term, outputs in matrices of their own", field, own, [], [R0, R1], [0, 0], [{"mat": "I", "col": 0}], alpha, beta, {"mat": "S", "col": 1}))
    jpath = tmp_path / "job.json"
    jpath.write_text(json.dumps({"cases": cases, "layout": _layout()}))
    out = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "logup_cluster_parity.js"), str(jpath)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "logup cluster parity OK" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
