"""The lookup and permutation checks from Node: js/pil_checks.js checkLookup / checkPermutation (host matrices as words and as bytes) and
checkLookupDev / checkPermutationDev (DevBuffer sections with column lists, f and t of one matrix among them) on a case file written
here: null when clean, else the checker's five words and the message INTEGRATION.md states, which names the reported row, the tuple's
values and both counts.  Node runs as a fresh child process."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import tuple_check_ref as tref
import conn_pols_ref as ref
from conn_pols_ref import P, R, MONT
from conftest import ROOT

NODE = shutil.which("node")
L, M = tref.LOOKUP, tref.PERMUTATION


def words(field, rows):
    if field == "gl":
        return np.array(rows, np.uint64).reshape(len(rows), -1)
    return ref.fr_words([v for row in rows for v in row]).reshape(len(rows), -1, 4)


def decimal(v, q):
    """what js prints for a bit pattern: the value mod p, the normal form of Montgomery words"""
    return str(v % P) if q == P else str(v % R * pow(MONT, -1, R) % R)


def message(rep, mode, f, t, q):
    kind, row, partner, cnt_f, cnt_t = rep
    name = "lookup" if mode == L else "permutation"
    tup = "(" + ", ".join(decimal(v, q) for v in (t if kind == 3 else f)[row]) + ")"
    counts = " (cntF = %d, cntT = %d)" % (cnt_f, cnt_t)
    if kind == 1:
        return "%s: f row %d = %s occurs in no selected row of t%s" % (name, row, tup, counts)
    if kind == 2:
        return "%s: f row %d = %s occurs %d times in f and %d times in t, first in t at row %d%s" % (name, row, tup, cnt_f, cnt_t, partner, counts)
    where = "nowhere in f" if partner == tref.NONE else "first in f at row %d" % partner
    return "%s: t row %d = %s occurs %d times in t and %d times in f, %s%s" % (name, row, tup, cnt_t, cnt_f, where, counts)


def case(name, field, mode, fm, f_cols, tm, t_cols, sel_f=None, sel_t=None, one=False):
    """fm, tm: rows of bit patterns, whole matrices; sel_*: (rows, col) or None"""
    q = P if field == "gl" else R
    n = len(fm)
    fw, tw = words(field, fm), words(field, tm)
    f, t = tref.tuples(fw, f_cols, q), tref.tuples(tw, t_cols, q)
    sel = lambda s: None if s is None else tref.column(words(field, s[0]), s[1], q)      # noqa: E731
    rep = tref.check(f, t, mode, q, sel(sel_f), sel(sel_t))
    want = None
    if rep[0]:
        want = {"kind": rep[0], "row": rep[1], "partner": None if rep[2] == tref.NONE else rep[2], "cntF": rep[3], "cntT": rep[4],
                "side": "t" if rep[0] == 3 else "f", "message": message(rep, mode, f, t, q)}
    side = lambda w, cols: {"words": w.tobytes().hex(), "stride": w.shape[1], "cols": cols}      # noqa: E731
    selector = lambda s: None if s is None else {"words": words(field, s[0]).tobytes().hex(), "stride": len(s[0][0]), "col": s[1]}      # noqa: E731
    return {"name": name, "field": field, "mode": mode, "n": n, "f": side(fw, f_cols), "t": side(tw, t_cols), "selF": selector(sel_f),
            "selT": selector(sel_t), "one": one, "want": want}


@pytest.mark.gpu
@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_js_lookup_and_permutation_checks_match_the_checker(tmp_path):
    from pil2gl import pilcheck
    cases = []
    for field, q in (("gl", P), ("bn128", R)):
        n = 80
        t = [[(i * 7919) % 10007, i % 5, (i * i) % 97] for i in range(n)]
        f = list(t)
        ref.rng(n).shuffle(f)
        wide = lambda rows, cols, width: [[row[cols.index(c)] if c in cols else q - 1 - c for c in range(width)] for row in rows]      # noqa: E731
        fc, tc = [4, 0, 2], [1, 2, 5]
        for mode in (L, M):
            tag = "%s %s " % (field, "lookup" if mode == L else "permutation")
            cases.append(case(tag + "clean", field, mode, wide(f, fc, 6), fc, wide(t, tc, 7), tc))
            g = [list(r) for r in f]
            g[41][2] += 1000                                                     # kind 1: a tuple of no row of t
            cases.append(case(tag + "kind 1", field, mode, wide(g, fc, 6), fc, wide(t, tc, 7), tc))
            g = [list(r) for r in f]
            g[60] = list(g[7])                                                   # kind 2 in a permutation, clean in a lookup
            g[7][0] += q                                                         # the reported row holds a pattern past the modulus: printed as its value
            cases.append(case(tag + "kind 2", field, mode, wide(g, fc, 6), fc, wide(t, tc, 7), tc))
            sel = [[5, 0 if i == 13 else 1] for i in range(n)]                   # kind 3: f deselects a row, its tuple stays t's alone
            cases.append(case(tag + "kind 3", field, mode, wide(f, fc, 6), fc, wide(t, tc, 7), tc, sel_f=(sel, 1)))
            sel_t = [[0 if tuple(r) == tuple(f[13]) else 3] for r in t]          # ... until t deselects it too
            cases.append(case(tag + "both selectors", field, mode, wide(f, fc, 6), fc, wide(t, tc, 7), tc, sel_f=(sel, 1), sel_t=(sel_t, 0)))
            both = [[tr[0], tr[1], tr[2], q - 9, fr[2], fr[1], fr[0]] for fr, tr in zip(g, t)]
            cases.append(case(tag + "one matrix", field, mode, both, [6, 5, 4], both, [0, 1, 2], one=True))
    kinds = {(c["mode"], c["want"]["kind"]) for c in cases if c["want"]}
    assert kinds == {(L, 1), (M, 1), (M, 2), (M, 3)} and sum(c["want"] is None for c in cases) >= 8
    assert all(str(c["want"]["row"]) in c["want"]["message"] and "cntF = %d, cntT = %d" % (c["want"]["cntF"], c["want"]["cntT"]) in c["want"]["message"]
               for c in cases if c["want"])
    homes = [{"words": [i, 0, 5], "k": 3, "capacity": 32, "bn128": False, "home": pilcheck.tuple_home(np.array([i, 0, 5], np.uint64), 3, "gl", 32)} for i in range(4)]
    homes.append({"words": list(range(8)), "k": 2, "capacity": 1 << 20, "bn128": True, "home": pilcheck.tuple_home(np.arange(8, dtype=np.uint64), 2, "bn128", 1 << 20)})
    jpath = tmp_path / "job.json"
    jpath.write_text(json.dumps({"cases": cases, "homes": homes}))
    out = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "tuple_check_parity.js"), str(jpath)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "tuple check parity OK" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
