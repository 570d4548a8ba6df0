"""The grand product of a permutation and of a 12-column connection from Node: js/pil_checks.js grandProduct (host matrices as words and as
bytes) and grandProductDev (DevBuffer sections), and the spellings calculateZPermutation[Dev] / calculateZConnection[Dev] of
js/polutils.js and js/polutils_bn128.js, both fields, on a case file written here: every word of every matrix after the call, from the
checker (tests/grand_prod_ref.py).  Node runs as a fresh child process."""
import json
import os
import random
import shutil
import subprocess

import numpy as np
import pytest

import grand_prod_ref as gref
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


def chal_hex(field, v):
    """an extension element's VALUE as the words the call takes"""
    return np.array(v, np.uint64).tobytes().hex() if field == "gl" else cref.fr_words([v % R * MONT % R]).tobytes().hex()


def case(name, field, mats, terms, alpha, beta, gamma, out, **more):
    """mats: name -> rows of bit patterns; terms: {"mat", "cols", "sel": {"mat", "col"} | None, "den", "id": {"mat", "col"} | None, "idCoef"}
    with idCoef a VALUE; out: {"mat", "col"}"""
    n = len(mats[out["mat"]])
    width = 3 if field == "gl" else 1
    ref_terms = []
    for t in terms:
        col = lambda c: None if not c else [value(field, row[c["col"]]) for row in mats[c["mat"]]]      # noqa: E731
        ref_terms.append(([[value(field, row[c]) for c in t["cols"]] for row in mats[t["mat"]]], col(t.get("sel")), t["den"], col(t.get("id")), t.get("idCoef")))
    z = gref.grand_prod(field, ref_terms, alpha, beta, gamma, n)
    after = {k: words(field, rows).copy() for k, rows in mats.items()}
    after[out["mat"]][:, out["col"]:out["col"] + width] = np.array(z, np.uint64).reshape(n, 3) if field == "gl" else cref.fr_words([v * MONT % R for v in z]).reshape(n, 1, 4)
    plan = gref.plan(n, field)[0]
    return dict({"name": name, "field": field, "n": n, "mats": {k: {"words": words(field, rows).tobytes().hex(), "stride": len(rows[0])} for k, rows in mats.items()},
                 "terms": [dict(t, idCoef=chal_hex(field, t["idCoef"]) if t.get("id") else None) for t in terms], "alpha": chal_hex(field, alpha),
                 "beta": chal_hex(field, beta), "gamma": chal_hex(field, gamma), "out": out, "after": {k: w.tobytes().hex() for k, w in after.items()},
                 "plan": [plan[3], plan[5]], "sumK": sum(len(t["cols"]) for t in terms)}, **more)


@pytest.mark.gpu
@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_js_grand_product_matches_the_checker(tmp_path):
    cases = []
    for field, q in (("gl", P), ("bn128", R)):
        rng = random.Random(41 if field == "gl" else 43)
        F = lref.FIELDS[field]
        width = 3 if field == "gl" else 1
        top = (1 << 64) if field == "gl" else (1 << 256)
        ch = lambda: tuple(rng.randrange(P) for _ in range(3)) if field == "gl" else rng.randrange(R)      # noqa: E731
        # a permutation of two columns with selectors that are field values; z in spare columns of t's matrix, one more column that must survive
        n = 80
        f = [[rng.randrange(q) + (q if i % 2 and 2 * q < top else 0), rng.randrange(q), rng.choice((0, 1, 2, q - 1))] for i in range(n)]
        t = [[rng.randrange(q), rng.randrange(q), rng.choice((0, 1, 5))] + [q - 9 - j for j in range(width + 1)] for _ in range(n)]
        pf = {"mat": "F", "cols": [1, 0], "sel": {"mat": "F", "col": 2}}
        pt = {"mat": "T", "cols": [0, 1], "sel": {"mat": "T", "col": 2}}
        cases.append(case(field + " permutation, out in t's matrix", field, {"F": f, "T": t}, [dict(pf, den=0), dict(pt, den=1)], ch(), ch(), ch(), {"mat": "T", "col": 3},
                          perm={"f": pf, "t": pt}))
        # a 12-column connection: a, S and x of a small sMap, z in a matrix of its own with stride gaps
        n_bits, n_cols = 5, 12
        N = 1 << n_bits
        s_map = [rng.randrange(24) for _ in range(N * n_cols)]
        wit = [rng.randrange(q) for _ in range(24)]
        w, ks = cref.root(q, n_bits), cref.get_ks(q, n_cols - 1)
        S = cref.rows(cref.conn_pols(s_map, N, n_cols, N, w, ks, q))
        pat = (lambda v: v) if field == "gl" else (lambda v: v * MONT % R)
        a = [[pat(wit[s_map[i * n_cols + j]]) for j in range(n_cols)] for i in range(N)]
        mats = {"A": a, "S": [[pat(v) for v in row] for row in S], "X": [[pat(pow(w, i, q)), 7] for i in range(N)],
                "Z": [[q - 1 - i - j for j in range(width + 2)] for i in range(N)]}
        gamma, delta = ch(), ch()
        dks = [F.mul(F.ext(delta), F.base(1 if j == 0 else ks[j - 1])) for j in range(n_cols)]
        terms = []
        for j in range(n_cols):
            terms.append({"mat": "A", "cols": [j], "sel": None, "den": 0, "id": {"mat": "X", "col": 0}, "idCoef": dks[j]})
            terms.append({"mat": "A", "cols": [j], "sel": None, "den": 1, "id": {"mat": "S", "col": j}, "idCoef": delta})
        conn = {"a": [{"mat": "A", "col": j} for j in range(n_cols)], "S": [{"mat": "S", "col": j} for j in range(n_cols)], "x": {"mat": "X", "col": 0},
                "delta": chal_hex(field, delta), "deltaKs": [chal_hex(field, d) for d in dks]}
        cases.append(case(field + " connection of 12 columns", field, mats, terms, gamma, gamma, gamma, {"mat": "Z", "col": 1}, conn=conn))
    jpath = tmp_path / "job.json"
    jpath.write_text(json.dumps({"cases": cases}))
    out = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "grand_prod_parity.js"), str(jpath)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "grand product parity OK" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
