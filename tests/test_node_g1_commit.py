"""The BN254 G1 stage commit from Node: js/g1_msm.js multiExpPacked over Uint8Arrays and DevBuffers, against bytes the Python checker
(tests/bn128_g1_packed_ref.py) wrote.  Node runs as a fresh child process."""
import json
import os
import random
import shutil
import subprocess

import numpy as np
import pytest

import bn128_g1_ref as ref
import bn128_g1_packed_ref as pref
from conftest import ROOT

NODE = shutil.which("node")


def _hex(words):
    return np.ascontiguousarray(words).astype("<u8").tobytes().hex()


def _job():
    rng = random.Random(2026)
    pts, logs = ref.known_log_bases(2048, seed=78)
    pts[3] = None                                                    # a point at infinity among them
    cases = []
    for stride, mont, polys in ((4, True, [(0, 300, [2, None, 0, 3]), (4, 100, [1]), (0, 512, [3, 0, 1, 2])]),      # K = 3, one empty slot
                                (1, False, [(0, 500, [0]), (500, 500, [0]), (1000, 24, [0])]),
                                (3, True, [(0, 0, [0]), (0, 7, [None, None])])):
        n_elems = max([first + (rows - 1) * stride + max([c for c in slots if c is not None], default=0) + 1
                       for first, rows, slots in polys if rows] + [1])
        matrix = [rng.randrange(ref.R) for _ in range(n_elems)]
        want = [pref.expected(matrix, p, stride, logs, pts) for p in polys]
        cases.append({"stride": stride, "montgomery": mont, "bases": _hex(ref.point_words(pts)), "coefs": _hex(ref.scalar_words(matrix, mont)),
                      "polys": [{"first": first, "rows": rows, "slots": slots} for first, rows, slots in polys],
                      "expected": [_hex(ref.point_words([w])) for w in want]})
    return {"cases": cases}


@pytest.mark.gpu
@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_js_multi_exp_packed_matches_the_checker(tmp_path):
    job = tmp_path / "g1_commit_job.json"
    job.write_text(json.dumps(_job()))
    out = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "g1_commit_parity.js"), str(job)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "g1 commit parity OK" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
