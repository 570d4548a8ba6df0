"""The range-check grand sum from Node: js/pil_checks.js rangeSum (host matrices as words and as bytes) and rangeSumDev (DevBuffer
sections), js/polutils.js and js/polutils_bn128.js calculateSRange / calculateSRangeDev, both fields, on a case file written here: every
word of every matrix after the call, from the checker (tests/range_sum_ref.py).  The cases: no f term with a window that starts and ends
mid-lane and a negative lo (m poisoned outside it, out as spare columns of m's matrix); two f terms and two ranges on one m matrix, out of
its own with stride gaps; a zero denominator inside a window.  Node runs as a fresh child process."""
import json
import os
import random
import shutil
import subprocess

import numpy as np
import pytest

import logup_sum_ref as lref
import range_sum_ref as rref
import bn128_hints_ref as bref
import conn_pols_ref as cref
from hints_ref import P
from conftest import ROOT

NODE = shutil.which("node")
R, MONT = bref.R, bref.MONT


def words(field, rows):
    if field == "gl":
        return np.array(rows, np.uint64).reshape(len(rows), -1)
    return cref.fr_words([v for row in rows for v in row]).reshape(len(rows), -1, 4)


def value(field, pat):
    return pat % P if field == "gl" else bref.unmont(pat % R)


def elem_hex(field, v):
    """a base-field VALUE as the words the call takes"""
    return np.array([v % P], np.uint64).tobytes().hex() if field == "gl" else cref.fr_words([v % R * MONT % R]).tobytes().hex()


def chal_hex(field, v):
    return np.array(v, np.uint64).tobytes().hex() if field == "gl" else elem_hex(field, v)


def case(name, field, mats, terms, ranges, alpha, beta, out):
    """mats: name -> rows of bit patterns; terms: {"mat", "cols", "sel": {"mat", "col"} | None, "coef", "busId"}; ranges: {"mat", "col", "lo",
    "size", "row0", "coef", "busId"}; coef and busId VALUES; out: {"mat", "col"}"""
    n = len(mats[out["mat"]])
    width = 3 if field == "gl" else 1
    ref_terms = []
    for t in terms:
        tuples = [[value(field, row[c]) for c in t["cols"]] for row in mats[t["mat"]]]
        w = None if not t.get("sel") else [value(field, row[t["sel"]["col"]]) for row in mats[t["sel"]["mat"]]]
        ref_terms.append((tuples, w, t["coef"], t["busId"]))
    ref_ranges = [([value(field, mats[r["mat"]][i][r["col"]]) if r["row0"] <= i < r["row0"] + r["size"] else None for i in range(n)], r["lo"], r["size"], r["row0"],
                   r["coef"], r["busId"]) for r in ranges]
    s = rref.range_sum(field, ref_terms, ref_ranges, alpha, beta, n)
    after = {k: words(field, rows).copy() for k, rows in mats.items()}
    col = np.array(s, np.uint64).reshape(n, 3) if field == "gl" else cref.fr_words([v * MONT % R for v in s]).reshape(n, 1, 4)
    after[out["mat"]][:, out["col"]:out["col"] + width] = col
    plan = rref.plan(n, len(terms), len(ranges), field)[0]
    return {"name": name, "field": field, "n": n, "mats": {k: {"words": words(field, rows).tobytes().hex(), "stride": len(rows[0])} for k, rows in mats.items()},
            "terms": [dict(t, coef=elem_hex(field, t["coef"]), busId=elem_hex(field, t["busId"])) for t in terms],
            "ranges": [dict(r, lo=str(r["lo"]), coef=elem_hex(field, r["coef"]), busId=elem_hex(field, r["busId"])) for r in ranges], "alpha": chal_hex(field, alpha),
            "beta": chal_hex(field, beta), "out": out, "after": {k: w.tobytes().hex() for k, w in after.items()}, "plan": [plan[3], plan[5]]}


@pytest.mark.gpu
@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_js_range_sum_matches_the_checker(tmp_path):
    cases = []
    for field, q in (("gl", P), ("bn128", R)):
        rng = random.Random(71 if field == "gl" else 73)
        n, width = 80, 3 if field == "gl" else 1
        top = (1 << 64) if field == "gl" else (1 << 256)
        # M: two multiplicity columns, non-zero in every row and past the modulus in some, then spare columns for s and one that must survive
        mm = [[1 + rng.randrange(q - 1) + (q if i % 3 == 0 and 2 * q < top else 0), 1 + rng.randrange(5)] + [q - 9 - j for j in range(width + 1)] for i in range(n)]
        f0 = [[rng.randrange(q), rng.randrange(q), i % 3] for i in range(n)]
        alpha = tuple(rng.randrange(P) for _ in range(3)) if field == "gl" else rng.randrange(R)
        beta = tuple(rng.randrange(P) for _ in range(3)) if field == "gl" else rng.randrange(R)
        R0 = {"mat": "M", "col": 0, "lo": -3, "size": 38, "row0": 13, "coef": q - 1, "busId": 6}       # rows 13 .. 50: both ends mid-lane, crosses zero
        R1 = {"mat": "M", "col": 1, "lo": (1 << 63) - 20, "size": 20, "row0": 60, "coef": 5, "busId": 7}
        F0 = {"mat": "F0", "cols": [1, 0], "sel": {"mat": "F0", "col": 2}, "coef": 1, "busId": 6}
        K1 = {"mat": "F0", "cols": [1], "sel": None, "coef": 1, "busId": 7}
        cases.append(case(field + " no f term, one window, out in m's matrix", field, {"M": mm}, [], [R0], alpha, beta, {"mat": "M", "col": 2}))
        own = {"M": mm, "F0": f0, "S": [[q - 1 - i - j for j in range(width + 2)] for i in range(n)]}
        cases.append(case(field + " two f terms and two ranges, out of its own with stride gaps", field, own, [F0, K1], [R0, R1], alpha, beta, {"mat": "S", "col": 1}))
        F = lref.FIELDS[field]
        d0 = rref.range_denominator(F, (None, -3, 38, 13, q - 1, 6), F.ext(alpha), F.zero, 16)           # a lane's first row inside the window
        zb = tuple((P - x) % P for x in d0) if field == "gl" else (R - d0) % R
        cases.append(case(field + " a zero denominator", field, own, [K1], [R0, R1], alpha, zb, {"mat": "S", "col": 0}))
    jpath = tmp_path / "job.json"
    jpath.write_text(json.dumps({"cases": cases}))
    out = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "range_sum_parity.js"), str(jpath)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "range sum parity OK" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
