"""Setup -> prove from Node (tests/js/jit_cache.js): js/prover_helpers.js precompileExps in one process, callCalculateExps in the next,
which must compile nothing and write the words the Python-driven evaluation writes."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

NODE = shutil.which("node")
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(NODE is None, reason="node not installed")]


def _node(mode, job, env):
    out = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "jit_cache.js"), mode, str(job)], capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    return json.loads(out.stdout.strip().splitlines()[-1])


def test_precompile_exps_then_call_calculate_exps(tmp_path):
    """the constraint program of fibonacci_air(50) on 2^16 extended rows: the first node process knows neither publics nor challenges nor
    evaluations (and sees no GPU), the second has the proof's and finds the kernel the first one stored"""
    import evalpath
    pr = evalpath.fibonacci_program(50, 0, 16, 3, seed=9)
    d = pr["secs"][pr["dest"]].shape
    sections = {}
    for name, a in zip(pr["names"], pr["secs"]):
        f = tmp_path / (name.replace("#", "_") + ".u64")
        a.tofile(f)
        sections[name.split("#")[0]] = str(f)                   # js: one Zi_ext buffer, a block of rows per boundary (this AIR has one)
    c = pr["ctx"]
    job = {"dir": str(tmp_path / "cache"), "pilInfo": pr["info"], "code": pr["code"], "nBits": 13, "nBitsExt": 16, "sections": sections,
           "publics": [str(v) for v in c["publics"]], "challenges": [[[str(v) for v in ch] for ch in st] for st in c["challenges"]],
           "evals": [[str(v) for v in e] for e in c["evals"]], "dest": pr["names"][pr["dest"]], "out": str(tmp_path / "out.u64")}
    (tmp_path / "job.json").write_text(json.dumps(job))
    env = {k: v for k, v in os.environ.items() if not k.startswith("PIL2GL_")}
    a = _node("precompile", tmp_path / "job.json", dict(env, HIP_VISIBLE_DEVICES=""))
    assert a["result"]["routed"] == "jit" and a["result"]["origin"] == "compiled" and a["stats"]["diskWrites"] == 1, a
    b = _node("eval", tmp_path / "job.json", env)
    assert b["stats"]["compiles"] == 0 and b["stats"]["diskHits"] == 1 and b["stats"]["rejected"] == 0, b
    got = np.fromfile(tmp_path / "out.u64", dtype=np.uint64).reshape(d)
    want = evalpath.run_device(pr["ops"], pr["n_tmp"], pr["secs"], pr["scalars"], 16, 3, pr["dest"]).reshape(d)
    assert (got == want).all()
