"""The multiplicity sessions from Node: js/pil_checks.js LookupSession and RangeSession on DevBuffer matrices, both fields, on a case file
written here.  What Node must give is what pilcheck's sessions give on the same words -- every add's report, the total and every byte of
every matrix after the write -- and pilcheck's m is checked against tests/mult_session_ref.py first.  One lookup and one range session a
field, two adds each with sides of other lengths than the table, a failing row in the first.  Node runs as a fresh child process."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import mult_session_ref as sref
import range_mult_ref as rref
import conn_pols_ref as cref
from conn_pols_ref import P, R
from conftest import ROOT

from pil2gl import pilcheck

NODE = shutil.which("node")
NONE = sref.NONE


def words(field, rows):
    if field == "gl":
        return np.array(rows, np.uint64).reshape(len(rows), -1)
    return cref.fr_words([v for row in rows for v in row]).reshape(len(rows), -1, 4)


def js_report(rep):
    return {"matched": rep[3], "missing": None if rep[0] == 0 else {"side": rep[1], "row": rep[2]}}


@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_addon_surface_and_plans():
    """no device needed: the addon's entries and its plans against pilcheck's"""
    names = [k + "Session" + e for k in ("lookup", "range") for e in ("Plan", "OpenDev", "AddDev", "WriteDev")]
    js = "const a = require(%r).addon; console.log(JSON.stringify([%s.map((f) => typeof a[f]), a.lookupSessionPlan(1000, 3, 4), a.rangeSessionPlan(8193, 1)]));"
    out = subprocess.run([NODE, "-e", js % (os.path.join(ROOT, "pil2-stark-js_amd", "js", "native.js"), json.dumps(names))], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    got = json.loads(out.stdout)
    assert got[0] == ["function"] * 8
    pack = lambda p: {k: v for k, v in p.items() if not k.endswith("Launches")}                                  # noqa: E731
    launches = lambda p: p["openLaunches"] | p["addLaunches"] << 8 | p["writeLaunches"] << 16                    # noqa: E731
    for g, want in ((got[1], pilcheck.lookup_session_plan(1000, 3, "bn128")), (got[2], pilcheck.range_session_plan(8193, "gl"))):
        assert g == dict(pack(want), launches=launches(want))


@pytest.mark.gpu
@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_js_sessions_give_pilchecks_m(tmp_path):
    import torch
    to_dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()                           # noqa: E731
    cases = []
    for field, q in (("gl", P), ("bn128", R)):
        rng = np.random.default_rng(7 if field == "gl" else 9)
        top = 1 << (64 if field == "gl" else 256)
        pat = lambda v, bump=False: rref.pattern(v, q) + (q if bump and rref.pattern(v, q) + q < top else 0)     # noqa: E731
        n_t, lo, size, row0 = 37, -4, 30, 5
        T = [[pat(int(a), i % 3 == 0), pat(int(b)), q - 3 - i] for i, (a, b) in enumerate(rng.integers(0, 5, (n_t, 2)))]       # column 2: m
        A = [[pat(int(a)), pat(int(b), i % 4 == 1), i % 3] for i, (a, b) in enumerate(rng.integers(0, 6, (150, 2)))]           # column 2: a selector
        B = [[pat(lo + int(v), i % 5 == 0), i % 2] for i, v in enumerate(rng.integers(-1, size, 90))]
        M = [[q - 7 - i, q - 8 - i] for i in range(n_t)]
        mats = {"T": T, "A": A, "B": B, "M": M}
        host = {k: words(field, rows) for k, rows in mats.items()}
        for kind in ("lookup", "range"):
            dev = {k: to_dev(w) for k, w in host.items()}
            if kind == "lookup":
                s, r = pilcheck.LookupSession((dev["T"], [0, 1]), n_t, field), sref.LookupSession([row[:2] for row in T], q)
                adds = [([("A", [0, 1], None), ("A", [1, 0], ("A", 2))], [150, 3]), ([("A", [0, 1], ("A", 2))], [64])]
                out, rows_of = ("T", 2), lambda sp, n: [[A[i][c] for c in sp[1]] for i in range(n)]                # noqa: E731
            else:
                s, r = pilcheck.RangeSession(lo, size, field), sref.RangeSession(lo, size, q)
                adds = [([("B", [0], None), ("B", [0], ("B", 1))], [90, 65]), ([("B", [0], None)], [1])]
                out, rows_of = ("M", 1), lambda sp, n: [B[i][0] for i in range(n)]                                # noqa: E731
            jadds = []
            for specs, rows in adds:
                rep = s.add([(dev[m], cols, None if sel is None else (dev[sel[0]], sel[1])) for m, cols, sel in specs], rows)
                want = r.add([rows_of(sp, n) for sp, n in zip(specs, rows)], [None if sp[2] is None else [mats[sp[2][0]][i][sp[2][1]] for i in range(n)] for sp, n in zip(specs, rows)])
                assert rep == want
                jadds.append({"fs": [{"mat": m, "cols": cols, "sel": None if sel is None else {"mat": sel[0], "col": sel[1]}} for m, cols, sel in specs], "rows": rows,
                              "want": js_report(rep)})
            total = s.write((dev[out[0]], out[1])) if kind == "lookup" else s.write((dev[out[0]], out[1]), n_t, row0)
            after = {k: d.cpu().numpy().view(np.uint64).reshape(host[k].shape) for k, d in dev.items()}
            want_m = r.m() if kind == "lookup" else r.m(n_t, row0)
            assert total == r.total and (after[out[0]][:, out[1]] == words(field, [[sref.element(c, q)] for c in want_m])[:, 0]).all()
            assert all((after[k] == host[k]).all() for k in host if k != out[0])
            cases.append({"name": field + " " + kind, "field": field, "kind": kind, "nT": n_t, "nM": n_t, "lo": str(lo), "size": size, "row0": row0,
                          "t": {"mat": "T", "cols": [0, 1], "sel": None}, "m": {"mat": out[0], "col": out[1]}, "adds": jadds, "total": total,
                          "scratchBytes": s.plan["scratchBytes"], "mats": {k: {"words": w.tobytes().hex(), "stride": w.shape[1]} for k, w in host.items()},
                          "after": {k: np.ascontiguousarray(w).tobytes().hex() for k, w in after.items()}})
    jpath = tmp_path / "job.json"
    jpath.write_text(json.dumps({"cases": cases}))
    out = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "mult_session_parity.js"), str(jpath)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "mult session parity OK" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
