"""The lookup multiplicities from Node: js/pil_checks.js lookupMultiplicities (host matrices as words and as bytes) and
lookupMultiplicitiesDev (DevBuffer sections, m a spare column of t's matrix, of an f's, and a matrix of its own) on a case file written
here: `matched`, the missing pair with the message INTEGRATION.md states, and every word of every matrix after the call, from the checker
(tests/lookup_mult_ref.py).  Node runs as a fresh child process."""
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import lookup_mult_ref as mref
import conn_pols_ref as ref
from conn_pols_ref import P, R, MONT
from conftest import ROOT

NODE = shutil.which("node")


def words(field, rows):
    if field == "gl":
        return np.array(rows, np.uint64).reshape(len(rows), -1)
    return ref.fr_words([v for row in rows for v in row]).reshape(len(rows), -1, 4)


def decimal(v, q):
    """what js prints for a bit pattern: the value mod p, the normal form of Montgomery words"""
    return str(v % P) if q == P else str(v % R * pow(MONT, -1, R) % R)


def case(name, field, mats, fs, t, m):
    """mats: name -> rows of bit patterns; fs, t: {"mat", "cols", "sel": {"mat", "col"} | None}; m: {"mat", "col"}"""
    q = P if field == "gl" else R
    n = len(mats[t["mat"]])
    tup = lambda s: [[row[c] for c in s["cols"]] for row in mats[s["mat"]]]                          # noqa: E731
    sel = lambda s: None if not s.get("sel") else [row[s["sel"]["col"]] for row in mats[s["sel"]["mat"]]]      # noqa: E731
    counts, rep = mref.multiplicities([tup(s) for s in fs], tup(t), q, [sel(s) for s in fs], sel(t))
    want = {"matched": rep[3], "missing": None}
    if rep[0]:
        row = tup(fs[rep[1]])[rep[2]]
        want["missing"] = {"side": rep[1], "row": rep[2],
                           "message": "lookup: f side %d row %d = (%s) occurs in no selected row of t" % (rep[1], rep[2], ", ".join(decimal(v, q) for v in row))}
    after = {k: [list(r) for r in rows] for k, rows in mats.items()}
    for j, cnt in enumerate(counts):
        after[m["mat"]][j][m["col"]] = mref.element(cnt, q)
    pack = lambda rows: words(field, rows).tobytes().hex()                                           # noqa: E731
    return {"name": name, "field": field, "n": n, "mats": {k: {"words": pack(rows), "stride": len(rows[0])} for k, rows in mats.items()},
            "fs": fs, "t": t, "m": m, "want": want, "after": {k: pack(rows) for k, rows in after.items()}}


def test_the_wording_is_the_one_integration_md_states():
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "lookup: f side S row R = (v0, v1, ..) occurs in no selected row of t" in text
    js = open(os.path.join(ROOT, "pil2-stark-js_amd", "js", "pil_checks.js")).read()
    assert re.search(r'"lookup: f side " \+ x\.side \+ " row " \+ x\.row \+ " = \(" \+ values\.join\(", "\) \+ "\) occurs in no selected row of t"', js)


@pytest.mark.gpu
@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_js_lookup_multiplicities_match_the_checker(tmp_path):
    cases = []
    for field, q in (("gl", P), ("bn128", R)):
        n = 80
        table = [[(i * 7919) % 10007, i % 5] for i in range(n)]
        # t: the tuple in columns 2, 0, a selector in column 1 that unselects row 3, a spare column 3
        tm = [[r[1], 0 if i == 3 else 1, r[0], q - 9] for i, r in enumerate(table)]
        f0 = [[q - 5, table[(i * 3) % 20][0], table[(i * 3) % 20][1]] for i in range(n)]                # rows 0, 3, 6 .. of the table: row 3's tuple is not selected in t
        f0 = [r if r[1:] != table[3] else [r[0]] + table[6] for r in f0]
        f1 = [[table[i % 7 + 30][0] + (q if i % 2 else 0), table[i % 7 + 30][1], i % 3, 77] for i in range(n)]      # patterns past the modulus, its own selector in column 2
        T = {"mat": "T", "cols": [2, 0], "sel": {"mat": "T", "col": 1}}
        F0 = {"mat": "F0", "cols": [1, 2], "sel": None}
        F1 = {"mat": "F1", "cols": [0, 1], "sel": {"mat": "F1", "col": 2}}
        mats = {"T": tm, "F0": f0, "F1": f1}
        cases.append(case(field + " clean, m in t's matrix", field, mats, [F0, F1], T, {"mat": "T", "col": 3}))
        cases.append(case(field + " clean, m in an f's matrix", field, mats, [F0, F1], T, {"mat": "F1", "col": 3}))
        bad0 = [list(r) for r in f0]
        bad0[61] = [q - 5] + table[3]                                            # the tuple t holds at an unselected row only
        bad1 = [list(r) for r in f1]
        bad1[10][0] += 20000
        bad1[9][0] += 20000                                                      # row 9: 9 % 3 = 0, not selected; row 10 is
        mats = {"T": tm, "F0": bad0, "F1": bad1, "M": [[q - 1 - i, 5] for i in range(n)]}
        cases.append(case(field + " missing in two sides, m of its own", field, mats, [F0, F1], T, {"mat": "M", "col": 0}))
        cases.append(case(field + " missing in the second side alone", field, dict(mats, F0=f0), [F0, F1], T, {"mat": "M", "col": 1}))
    assert [c["want"]["missing"] is None for c in cases] == [True, True, False, False] * 2
    assert cases[2]["want"]["missing"]["side"] == 0 and cases[2]["want"]["missing"]["row"] == 61 and (cases[3]["want"]["missing"]["side"], cases[3]["want"]["missing"]["row"]) == (1, 10)
    jpath = tmp_path / "job.json"
    jpath.write_text(json.dumps({"cases": cases}))
    out = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "lookup_mult_parity.js"), str(jpath)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "lookup mult parity OK" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
