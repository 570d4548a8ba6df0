"""The connection polynomials from Node: js/witness_exec.js connectionPols on a setup-shaped sMap and connectionPolsDev on the resident
table of prepareExec (the exec files are written by tests/wtns_exec_ref.py, without additions), both fields, against the words of the
Python checker's sequential swaps (tests/conn_pols_ref.py).  Node runs as a fresh child process."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import conn_pols_ref as ref
import wtns_exec_ref as xref
from conn_pols_ref import P, R
from conftest import ROOT

NODE = shutil.which("node")


@pytest.mark.gpu
@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_js_connection_pols_match_the_checker(tmp_path):
    rng = ref.rng(5)
    job = {}
    for name, q, n_rows, n_cols, N in (("gl", P, 150, 12, 256), ("bn128", R, 70, 6, 128)):
        n_w = 60
        heavy = [1, n_w - 1, 7]
        flat = [rng.choice((0, rng.choice(heavy), rng.randrange(1, n_w))) for _ in range(n_rows * n_cols)]
        flat[0] = flat[-1] = 9
        w, ks = ref.root(q, N.bit_length() - 1), ref.get_ks(q, n_cols - 1)
        S = ref.words(ref.conn_pols(flat, n_rows, n_cols, N, w, ks, q), q)
        path = str(tmp_path / (name + ".exec"))
        (xref.write_compressor_exec if q == P else xref.write_final_exec)(path, [], flat, n_rows, n_cols)
        enc = (lambda v: str(v)) if q == P else (lambda v: ref.fr_words([ref.to_mont(v)]).tobytes().hex())
        s_map = [[flat[i * n_cols + j] if i < n_rows else 0 for i in range(N)] for j in range(n_cols)]
        job[name] = {"N": N, "nCols": n_cols, "nW": n_w, "exec": path, "sMap": s_map, "w": enc(w), "ks": [enc(k) for k in ks], "one": enc(1),
                     "S": np.ascontiguousarray(S).tobytes().hex()}
    jpath = tmp_path / "job.json"
    jpath.write_text(json.dumps(job))
    out = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "conn_pols_parity.js"), str(jpath)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "conn pols parity OK" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
