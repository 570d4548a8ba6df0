"""The BN254 G1 multi-scalar multiplication from Node: js/g1_msm.js multiExpAffine over Uint8Arrays and DevBuffers, against bytes the
Python checker (tests/bn128_g1_ref.py) wrote.  Node runs as a fresh child process."""
import json
import os
import random
import shutil
import subprocess

import numpy as np
import pytest

import bn128_g1_ref as ref
from conftest import ROOT

NODE = shutil.which("node")


def _hex(words):
    return np.ascontiguousarray(words).astype("<u8").tobytes().hex()


def _job():
    cases = []
    rng = random.Random(2025)
    pts, logs = ref.known_log_bases(4096, seed=77)
    pts[3] = None                                                    # a point at infinity among them
    for n, stride, mont in ((257, 1, True), (257, 2, True), (4096, 1, True), (4096, 2, False)):
        s = [rng.randrange(ref.R) for _ in range(n)]
        cols = np.zeros((n, stride, 4), np.uint64)
        cols[:, 0, :] = ref.scalar_words(s, mont)
        if stride > 1:                                               # the other column: something that must not be read
            cols[:, 1, :] = ref.scalar_words([rng.randrange(ref.R) for _ in range(n)], mont)
        want = ref.expected_from_logs([0 if p is None else x for x, p in zip(s, pts)], logs[:n])
        cases.append({"n": n, "stride": stride, "montgomery": mont, "bases": _hex(ref.point_words(pts[:n])), "scalars": _hex(cols),
                      "expected": _hex(ref.point_words([want]))})
    return {"cases": cases}


@pytest.mark.gpu
@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_js_multi_exp_affine_matches_the_checker(tmp_path):
    job = tmp_path / "g1_msm_job.json"
    job.write_text(json.dumps(_job()))
    out = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "g1_msm_parity.js"), str(job)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "g1 msm parity OK" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
