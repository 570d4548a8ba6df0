"""The connection check from Node: js/witness_exec.js checkConnections (host matrices, both shapes) and checkConnectionsDev (resident
columns of a wider matrix) on the reference-written cases of tests/golden/conn_pols.json, with a trace filled from the same sMap, and on
one small Fr case made by the checkers here: null when clean, the failing cell and the message INTEGRATION.md states for one altered
cell and for an S value that names no cell.  Node runs as a fresh child process."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import conn_check_ref as cref
import conn_pols_ref as ref
from conn_pols_ref import P, R
from conftest import ROOT

NODE = shutil.which("node")
GOLDEN = os.path.join(ROOT, "tests", "golden", "conn_pols.json")


def report(rep, a, S, n_cols):
    """the checker's words and the VALUES of a and S -> what js returns, message included"""
    cell, to, kind = rep
    if kind == 0:
        return None
    row, col = divmod(cell, n_cols)
    to_row, to_col = divmod(to, n_cols) if to != cref.NONE else (None, None)
    at = "[%d][%d]" % (col, row)
    if kind == 1:
        msg = "connect: S%s = %d names no cell (a%s = %d)" % (at, S[cell], at, a[cell])
    else:
        msg = "connect: a%s = %d differs from a[%d][%d] = %d, the cell S%s names" % (at, a[cell], to_col, to_row, a[to], at)
    return {"row": row, "col": col, "toRow": to_row, "toCol": to_col, "kind": kind, "message": msg}


def case(name, field, flat, S, n_cols, N, w, ks, seed):
    """S, flat sMap: N * n_cols values in flat order -> the job's case: a clean trace, one altered cell, and (through S) nothing more"""
    q = P if field == "gl" else R
    rng = ref.rng(seed)
    wit = [0] + [rng.randrange(q) for _ in range(max(flat))]
    a = [wit[s] for s in flat]
    enc = (lambda v: str(v)) if q == P else (lambda v: ref.fr_words([ref.to_mont(v)]).tobytes().hex())
    words = (lambda v: np.array(v, np.uint64)) if q == P else (lambda v: ref.fr_words([ref.to_mont(x) for x in v]))
    groups = {}
    for c, s in enumerate(flat):
        if s:
            groups.setdefault(s, []).append(c)
    big = max(groups.values(), key=len)
    assert len(big) >= 3
    broken = list(a)
    broken[big[1]] = (broken[big[1]] + 1) % q
    traces = []
    for t in (a, broken):
        rep = cref.check(t, S, n_cols, N, w, [1] + ks, q)
        traces.append({"a": words(t).tobytes().hex(), "want": report(rep, t, S, n_cols)})
    assert traces[0]["want"] is None and traces[1]["want"]["kind"] == 2 and (traces[1]["want"]["col"], traces[1]["want"]["row"]) == divmod(big[1], n_cols)[::-1]
    return {"name": name, "field": field, "N": N, "nCols": n_cols, "w": enc(w), "ks": [enc(k) for k in ks], "one": enc(1), "S": words(S).tobytes().hex(),
            "traces": traces}


@pytest.mark.gpu
@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_js_connection_check_matches_the_checker(tmp_path):
    cases = []
    for k, c in enumerate(json.load(open(GOLDEN))["cases"]):
        n_rows, n_cols, N = c["nRows"], c["nCols"], 1 << c["nBits"]
        flat = [c["sMap"][j][i] if i < n_rows else 0 for i in range(N) for j in range(n_cols)]
        S = [int(c["S"][j][i]) for i in range(N) for j in range(n_cols)]
        cases.append(case(c["name"], "gl", flat, S, n_cols, N, int(c["w"]), [int(x) for x in c["ks"]], k))
    # an S value that names no cell, on the first golden case: cell 1 <- 0
    first = cases[0]
    c = json.load(open(GOLDEN))["cases"][0]
    n_cols, N = c["nCols"], 1 << c["nBits"]
    S = [int(c["S"][j][i]) for i in range(N) for j in range(n_cols)]
    S[1] = 0
    a = [int(v) for v in np.frombuffer(bytes.fromhex(first["traces"][0]["a"]), np.uint64)]
    rep = cref.check(a, S, n_cols, N, int(c["w"]), [1] + [int(x) for x in c["ks"]], P)
    assert rep == (1, cref.NONE, 1)
    cases.append(dict(first, name=first["name"] + ", S[1] = 0", S=np.array(S, np.uint64).tobytes().hex(),
                      traces=[{"a": first["traces"][0]["a"], "want": report(rep, a, S, n_cols)}]))
    # Fr: 32 rows x 4 columns, a heavy signal, groups of a few cells, zeros
    rng = ref.rng(44)
    N, n_cols = 32, 4
    flat = [rng.choice((0, 1, 1, 1, 2 + rng.randrange(8))) for _ in range(N * n_cols)]
    w, ks = ref.root(R, 5), ref.get_ks(R, n_cols - 1)
    S = [v for row in ref.rows(ref.conn_pols(flat, N, n_cols, N, w, ks, R)) for v in row]
    cases.append(case("fr 32 x 4", "bn128", flat, S, n_cols, N, w, ks, 9))
    jpath = tmp_path / "job.json"
    jpath.write_text(json.dumps({"cases": cases}))
    out = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "conn_check_parity.js"), str(jpath)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "conn check parity OK" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
