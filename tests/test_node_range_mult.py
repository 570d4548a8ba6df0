"""The range-check multiplicities from Node: js/pil_checks.js rangeMultiplicities (host matrices as words and as bytes) and
rangeMultiplicitiesDev (DevBuffer sections, m a spare column of an f's matrix and a matrix of its own) on a case file written here:
`matched`, the missing pair with the message INTEGRATION.md states, and every word of every matrix after the call, from the checker
(tests/range_mult_ref.py).  Node runs as a fresh child process."""
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import range_mult_ref as rref
import conn_pols_ref as ref
from conn_pols_ref import P, R
from conftest import ROOT

NODE = shutil.which("node")


def words(field, rows):
    if field == "gl":
        return np.array(rows, np.uint64).reshape(len(rows), -1)
    return ref.fr_words([v for row in rows for v in row]).reshape(len(rows), -1, 4)


def case(name, field, mats, fs, lo, size, m, row0=0):
    """mats: name -> rows of bit patterns; fs: {"mat", "cols": [c], "sel": {"mat", "col"} | None}; m: {"mat", "col"}"""
    q = P if field == "gl" else R
    n = len(mats[m["mat"]])
    col = lambda s: [row[s["cols"][0]] for row in mats[s["mat"]]]                                    # noqa: E731
    sel = lambda s: None if not s.get("sel") else [row[s["sel"]["col"]] for row in mats[s["sel"]["mat"]]]      # noqa: E731
    counts, rep = rref.multiplicities([col(s) for s in fs], lo, size, n, q, [sel(s) for s in fs], row0)
    want = {"matched": rep[3], "missing": None}
    if rep[0]:
        v = col(fs[rep[1]])[rep[2]]
        want["missing"] = {"side": rep[1], "row": rep[2],
                           "message": "range: f side %d row %d = %d is outside [%d, %d]" % (rep[1], rep[2], rref.value(v, q), lo, lo + size - 1)}
    after = {k: [list(r) for r in rows] for k, rows in mats.items()}
    for j, cnt in enumerate(counts):
        after[m["mat"]][j][m["col"]] = rref.element(cnt, q)
    pack = lambda rows: words(field, rows).tobytes().hex()                                           # noqa: E731
    return {"name": name, "field": field, "n": n, "lo": str(lo), "size": size, "row0": row0,
            "mats": {k: {"words": pack(rows), "stride": len(rows[0])} for k, rows in mats.items()},
            "fs": fs, "m": m, "want": want, "after": {k: pack(rows) for k, rows in after.items()}}


def test_the_wording_is_the_one_integration_md_states():
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "range: f side S row R = V is outside [LO, HI]" in text
    assert "rangeMultiplicitiesDev" in text and "logupSumDev" in text
    js = open(os.path.join(ROOT, "pil2-stark-js_amd", "js", "pil_checks.js")).read()
    assert re.search(r'"range: f side " \+ x\.side \+ " row " \+ x\.row \+ " = " \+ value \+ " is outside \[" \+ lo \+ ", " \+', js)


@pytest.mark.gpu
@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_js_range_multiplicities_match_the_checker(tmp_path):
    cases = []
    for field, q in (("gl", P), ("bn128", R)):
        n = 300                                                                  # the widest range below has 256 values
        pat = lambda v: rref.pattern(v, q)                                       # noqa: E731
        # F0: the value in column 1, a spare column 2; F1: the value in column 0 (every other one lifted past the modulus), its selector in column 2
        f0 = [[q - 5, pat(-128 + (i * 37) % 256), q - 9] for i in range(n)]
        top = 1 << (64 if field == "gl" else 256)                                 # a pattern fits its words
        f1 = [[pat(-3 + i % 7) + (q if i % 2 and pat(-3 + i % 7) + q < top else 0), 77, i % 3, 78] for i in range(n)]
        F0 = {"mat": "F0", "cols": [1], "sel": None}
        F1 = {"mat": "F1", "cols": [0], "sel": {"mat": "F1", "col": 2}}
        mats = {"F0": f0, "F1": f1}
        cases.append(case(field + " clean, negative lo, m in an f's matrix", field, mats, [F0, F1], -128, 256, {"mat": "F1", "col": 3}))
        cases.append(case(field + " clean, the table at the end of m", field, mats, [F1], -3, 7, {"mat": "F0", "col": 2}, row0=n - 7))
        bad0 = [list(r) for r in f0]
        bad0[61][1] = pat(128)                                                   # lo + size
        bad1 = [list(r) for r in f1]
        bad1[10][0] = pat(-129)
        bad1[9][0] = pat(1 << 40)                                                # row 9: 9 % 3 = 0, not selected; row 10 is
        mats = {"F0": bad0, "F1": bad1, "M": [[q - 1 - i, 5] for i in range(n)]}
        cases.append(case(field + " out of range in two sides, m of its own", field, mats, [F0, F1], -128, 256, {"mat": "M", "col": 0}))
        cases.append(case(field + " out of range in the second side alone", field, dict(mats, F0=f0), [F0, F1], -128, 256, {"mat": "M", "col": 1}))
        cases.append(case(field + " lo at the end of the signed range", field, {"F0": [[0, pat((1 << 63) - 4 + i % 5), 0] for i in range(n)]}, [F0],
                          (1 << 63) - 4, 4, {"mat": "F0", "col": 2}))
    assert [c["want"]["missing"] is None for c in cases] == [True, True, False, False, False] * 2
    assert cases[2]["want"]["missing"]["message"] == "range: f side 0 row 61 = 128 is outside [-128, 127]"
    assert cases[3]["want"]["missing"]["message"] == "range: f side 1 row 10 = %d is outside [-128, 127]" % (P - 129)
    assert cases[8]["want"]["missing"]["message"] == "range: f side 1 row 10 = %d is outside [-128, 127]" % (R - 129), "V as F.toString prints it"
    assert cases[4]["want"]["missing"]["message"] == "range: f side 0 row 4 = %d is outside [%d, %d]" % (1 << 63, (1 << 63) - 4, (1 << 63) - 1)
    jpath = tmp_path / "job.json"
    jpath.write_text(json.dumps({"cases": cases}))
    out = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "range_mult_parity.js"), str(jpath)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "range mult parity OK" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
