"""The BN254 Fr polynomial operations from Node: js/polynomial_bn128.js divZh (divisible and not), divByXNSubValue and evaluate on
DevBuffers and staged arrays, against the Python checker's bytes (tests/bn128_poly_ref.py).  The test writes a job, Node runs it as a
fresh child process and compares bytes."""
import json
import os
import shutil
import subprocess

import pytest

import bn128_poly_ref as ref
from bn128_poly_ref import R
from conftest import ROOT

NODE = shutil.which("node")


def hx(vals):
    return ref.words(vals).tobytes().hex()


@pytest.mark.gpu
@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_js_polynomial_operations_match_the_checker(tmp_path):
    N, n = 64, 256
    q = ref.rand_elems(n - N, 1)
    c = ref.mul_back(q, [0] * N, N, 1)
    spoilt = list(c)
    spoilt[N + 5] ^= 1
    job = {"divzh": {"N": N, "c": hx(c), "want": hx(ref.scan(c, N, 1)), "spoilt": hx(spoilt)}, "div": []}
    for k, beta, stride, col in ((1, 12345, 1, 0), (5, R - 1, 3, 1), (300, ref.rand_elems(1, 2)[0], 2, 1)):
        rows = 1200
        m = ref.rand_elems(rows * stride, k)
        want = list(m)
        want[col::stride] = ref.scan(m[col::stride], k, beta)
        job["div"].append({"k": k, "beta": hx([ref.mont(beta)]), "stride": stride, "col": col, "n": rows, "m": hx(m), "want": hx(want)})
    pc = ref.rand_elems(2000, 3)
    zs = [0, 1, R - 1] + ref.rand_elems(2, 4)
    job["eval"] = {"c": hx(pc), "points": [hx([ref.mont(z)]) for z in zs], "want": [hx([ref.evaluate(pc, z)]) for z in zs]}
    path = tmp_path / "job.json"
    path.write_text(json.dumps(job))
    out = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "poly_bn128_parity.js"), str(path)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "poly bn128 parity OK" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
