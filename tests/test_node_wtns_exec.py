"""The recursion witness expansion from Node: js/witness_exec.js reads the files this test writes (a compressor .exec, a final .exec, a
.wtns; writers restated in tests/wtns_exec_ref.py), runs the array drop-ins and the resident forms for both fields and compares bytes
with the Python checker's trace.  Node runs as a fresh child process."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import wtns_exec_ref as ref
from wtns_exec_ref import P, R
from conftest import ROOT

NODE = shutil.which("node")


@pytest.mark.gpu
@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_js_witness_exec_matches_the_checker(tmp_path):
    rng = ref.rng(42)
    job = {}
    # Goldilocks, compressor shape: edge words in the witness, a queue-reduced combination among the additions
    n_rows, n_cols = 130, 12
    w = [P - 1, P, (1 << 64) - 1, 0, 1] + [rng.randrange(1 << 64) for _ in range(40)]
    adds = ref.queue_reduction(list(range(1, 34)), len(w)) + [(1, 1, P - 1, P - 1)]
    adds += [(a + 33 if a >= len(w) else a, b + 33 if b >= len(w) else b, ca, cb) for a, b, ca, cb in ref.random_dag(rng, len(w), 60, 1 << 64)]
    n_w = len(w) + len(adds)
    s_map = [rng.choice((0, rng.randrange(n_w))) for _ in range(n_rows * n_cols)]
    s_map[:4] = [0, 1, n_w - 1, 0]
    path = str(tmp_path / "c12.exec")
    ref.write_compressor_exec(path, adds, s_map, n_rows, n_cols)
    cut = str(tmp_path / "cut.exec")
    shutil.copy(path, cut)
    with open(cut, "r+b") as f:
        f.truncate(os.path.getsize(path) - 8)
    full = ref.additions(w, adds, P)
    job["gl"] = {"exec": path, "nCols": n_cols, "nRows": n_rows, "nAdds": len(adds), "nWitness": len(w), "nLevels": max(ref.levels(adds, len(w))) + 1,
                 "w": np.array(w, np.uint64).tobytes().hex(),
                 "trace": np.array(ref.gather(full, s_map, n_rows, n_cols, n_cols, P), np.uint64).tobytes().hex(),
                 "wide": np.array(ref.gather(full, s_map, n_rows, n_cols, n_cols + 3, P), np.uint64).tobytes().hex(),
                 "truncated": cut, "truncatedMessage": "%d bytes found, %d expected" % (os.path.getsize(cut), os.path.getsize(path))}
    # BN254 Fr, final shape: the coefficients are VALUES here, the file holds their Montgomery words
    n_rows, n_cols = 70, 6
    w = [R - 1, 0, 1] + [rng.randrange(R) for _ in range(30)] + [(k + 1) | ((k + 1001) << 128) for k in range(4)]
    adds = ref.random_dag(rng, len(w), 50, R)
    n_w = len(w) + len(adds)
    s_map = [rng.choice((0, rng.randrange(n_w))) for _ in range(n_rows * n_cols)]
    s_map[:4] = [0, 1, n_w - 1, 0]
    path, wpath = str(tmp_path / "final.exec"), str(tmp_path / "final.wtns")
    ref.write_final_exec(path, adds, s_map, n_rows, n_cols)
    ref.write_wtns(wpath, w)
    rows = ref.trace(w, adds, s_map, n_rows, n_cols, R)
    job["bn128"] = {"exec": path, "wtns": wpath, "nCols": n_cols, "nRows": n_rows, "nAdds": len(adds), "nWitness": len(w), "prime": str(R),
                    "normal": ref.fr_words([v for r in rows for v in r]).tobytes().hex(),
                    "mont": ref.fr_words([ref.to_mont(v) for r in rows for v in r]).tobytes().hex()}
    jpath = tmp_path / "job.json"
    jpath.write_text(json.dumps(job))
    out = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "wtns_exec_parity.js"), str(jpath)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "wtns exec parity OK" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
