"""The lookup grand sum and the column-numerator gsum from Node: js/pil_checks.js logupSum (host matrices as words and as bytes) and
logupSumDev (DevBuffer sections; out a matrix of its own and spare columns of t's matrix), js/polutils.js and js/polutils_bn128.js
calculateSCol / calculateSColDev, both fields, on a case file written here: every word of every matrix after the call, from the checker
(tests/logup_sum_ref.py).  Node runs as a fresh child process."""
import json
import os
import random
import shutil
import subprocess

import numpy as np
import pytest

import logup_sum_ref as lref
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


def case(name, field, mats, terms, alpha, beta, out):
    """mats: name -> rows of bit patterns; terms: {"mat", "cols", "sel": {"mat", "col"} | None, "coef", "busId"} with VALUES; out: {"mat", "col"}"""
    n = len(mats[out["mat"]])
    width = 3 if field == "gl" else 1
    ref_terms = []
    for t in terms:
        tuples = [[value(field, row[c]) for c in t["cols"]] for row in mats[t["mat"]]]
        w = None if not t.get("sel") else [value(field, row[t["sel"]["col"]]) for row in mats[t["sel"]["mat"]]]
        ref_terms.append((tuples, w, t["coef"], t["busId"]))
    s = lref.logup_sum(field, ref_terms, alpha, beta, n)
    after = {k: words(field, rows).copy() for k, rows in mats.items()}
    col = np.array(s, np.uint64).reshape(n, 3) if field == "gl" else cref.fr_words([v * MONT % R for v in s]).reshape(n, 1, 4)
    after[out["mat"]][:, out["col"]:out["col"] + width] = col
    plan = lref.plan(n, len(terms), field)[0]
    return {"name": name, "field": field, "n": n, "mats": {k: {"words": words(field, rows).tobytes().hex(), "stride": len(rows[0])} for k, rows in mats.items()},
            "terms": [dict(t, coef=elem_hex(field, t["coef"]), busId=elem_hex(field, t["busId"])) for t in terms], "alpha": chal_hex(field, alpha),
            "beta": chal_hex(field, beta), "out": out, "after": {k: w.tobytes().hex() for k, w in after.items()}, "plan": [plan[3], plan[5]]}


@pytest.mark.gpu
@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_js_logup_sum_and_gsum_col_match_the_checker(tmp_path):
    cases, gsum_col = [], []
    for field, q in (("gl", P), ("bn128", R)):
        rng = random.Random(31 if field == "gl" else 37)
        n, width = 80, 3 if field == "gl" else 1
        top = (1 << 64) if field == "gl" else (1 << 256)
        # t: the tuple in columns 2, 0, the multiplicities in column 1, then spare columns for s and one that must survive
        tm = [[rng.randrange(q), rng.choice((0, 1, 2, 5)), rng.randrange(q)] + [q - 9 - j for j in range(width + 1)] for _ in range(n)]
        f0 = [[q - 5, rng.randrange(q), rng.randrange(q)] for _ in range(n)]
        f1 = [[rng.randrange(q) + (q if i % 2 and 2 * q < top else 0), rng.randrange(q), i % 3, 77] for i in range(n)]   # patterns past the modulus, a selector in column 2
        alpha = tuple(rng.randrange(P) for _ in range(3)) if field == "gl" else rng.randrange(R)
        beta = tuple(rng.randrange(P) for _ in range(3)) if field == "gl" else rng.randrange(R)
        T = {"mat": "T", "cols": [2, 0], "sel": {"mat": "T", "col": 1}, "coef": q - 1, "busId": 6}
        F0 = {"mat": "F0", "cols": [1, 2], "sel": None, "coef": 1, "busId": 6}
        F1 = {"mat": "F1", "cols": [0, 1], "sel": {"mat": "F1", "col": 2}, "coef": 1, "busId": 6}
        K1 = {"mat": "F1", "cols": [3], "sel": None, "coef": 5, "busId": 0}                     # a k of its own
        mats = {"T": tm, "F0": f0, "F1": f1}
        cases.append(case(field + " three terms, out in t's matrix", field, mats, [F0, F1, T], alpha, beta, {"mat": "T", "col": 3}))
        own = dict(mats, S=[[q - 1 - i - j for j in range(width + 2)] for i in range(n)])
        cases.append(case(field + " four terms, out of its own with stride gaps", field, own, [F0, F1, K1, T], alpha, beta, {"mat": "S", "col": 1}))
        # a zero denominator: beta cancels F0's row 7
        F = lref.FIELDS[field]
        d0 = lref.denominator(F, [value(field, f0[7][1]), value(field, f0[7][2])], F.ext(alpha), F.zero, 6)
        zb = tuple((P - x) % P for x in d0) if field == "gl" else (R - d0) % R
        cases.append(case(field + " a zero denominator", field, own, [F0, T], alpha, zb, {"mat": "S", "col": 0}))
        # gsum_col
        if field == "gl":
            for dn, dd in ((1, 3), (3, 1)):
                num = [[rng.randrange(P) for _ in range(dn)] for _ in range(n)]
                den = [[0] * dd if i in (0, 9, n - 1) else [rng.randrange(P) for _ in range(dd)] for i in range(n)]
                e3 = lambda r: tuple(r) + (0,) * (3 - len(r))                    # noqa: E731
                want = lref.gsum_col("gl", [e3(r) for r in num], [e3(r) for r in den])
                gsum_col.append({"name": "gl gsum_col %d %d" % (dn, dd), "field": "gl", "n": n, "dimNum": dn, "dimDen": dd, "num": np.array(num, np.uint64).tobytes().hex(),
                                 "den": np.array(den, np.uint64).tobytes().hex(), "want": np.array(want, np.uint64).tobytes().hex()})
        else:
            num = [rng.randrange(R) for _ in range(n)]
            den = [0 if i in (0, 9, n - 1) else rng.randrange(R) for i in range(n)]
            gsum_col.append({"name": "bn128 gsum_col", "field": "bn128", "n": n, "num": bref.mont_words(num).tobytes().hex(), "den": bref.mont_words(den).tobytes().hex(),
                             "want": bref.mont_words(lref.gsum_col("bn128", num, den)).tobytes().hex()})
    jpath = tmp_path / "job.json"
    jpath.write_text(json.dumps({"cases": cases, "gsumCol": gsum_col}))
    out = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "logup_sum_parity.js"), str(jpath)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "logup sum parity OK" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
