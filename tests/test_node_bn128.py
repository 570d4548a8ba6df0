"""The Node.js side of the BN128 hash family: device-resident trees through the MerkleHash drop-in (tests/js/bn128_resident.js) and a
whole BN128 proof driven from Node (tests/js/prove_bn128.js) that must equal the Python-driven proof of the same witness."""
import hashlib
import json
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

NODE = shutil.which("node")
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(NODE is None, reason="node not installed")]


def test_resident_bn128_trees_from_node():
    """resident merkelize = host merkelize word for word and tree.nodes is a DevBuffer; getGroupProofs (resident) = getGroupProof (host) for
    every row; verifyGroupProofs accepts them and refuses a changed word; writeToFile (resident) -> readFromFile({device: true}) keeps root
    and openings.  Shapes 2^6 x 9 arity 16 and 37 x 20 arity 4 custom"""
    out = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "bn128_resident.js")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "bn128 resident OK" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]


def _canon(v):
    """the proof's canonical text, as tests/js/prove_c3.js writes it"""
    if isinstance(v, (list, tuple)):
        return "[" + ",".join(_canon(x) for x in v) + "]"
    if isinstance(v, dict):
        return "{" + ",".join('"%s":%s' % (k, _canon(x)) for k, x in v.items()) + "}"
    return '"%d"' % int(v)


def _strs(v):
    if isinstance(v, dict):
        return {k: _strs(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [_strs(x) for x in v]
    if isinstance(v, int) and not isinstance(v, bool):
        return str(v)
    return v


@pytest.mark.parametrize("arity,custom", [(16, False), (4, True)])
def test_node_driven_bn128_proof_equals_python_driven_proof(tmp_path, arity, custom):
    """2^10 rows x 8 columns (four Fibonacci machines), blow-up 8, FRI 13/9/5, 8 queries, verificationHashType BN128: the stage loop in
    Python (pil2gl.stark.stark_gen on GpuBackend) and the stage loop in Node (tests/js/prove_bn128.js over the JS drop-ins, every tree
    resident) write the same proof -- same digest of the canonical text, same query positions -- and the JS verifier drop-in accepts it"""
    import numpy as np
    import torch
    import bench
    from pil2gl import stark
    n_bits, n_cols = 10, 8
    ss = {"nBits": n_bits, "nBitsExt": n_bits + 3, "nQueries": 8, "verificationHashType": "BN128", "merkleTreeArity": arity, "merkleTreeCustom": custom,
          "steps": [{"nBits": b} for b in (13, 9, 5)]}
    info, exprs, vinfo = stark.fibonacci_air(n_cols // 2, ss)
    gpu = stark.GpuBackend(0, False, hash_type="BN128", arity=arity, custom=custom)
    cm, consts, publics = bench.fibonacci_trace_gpu(torch.device("cuda", 0), n_bits, n_cols // 2, 0)
    start = [int(v) for v in cm[:n_cols].cpu().numpy().view(np.uint64)]
    setup = stark.build_const_tree(gpu, consts, info)
    res = stark.stark_gen(gpu, cm, setup, info, exprs, publics)
    torch.cuda.synchronize()
    digest = hashlib.sha256(_canon(res["proof"]).encode()).hexdigest()
    job = {"pilInfo": info, "expressionsInfo": exprs, "verifierInfo": {"qVerifier": vinfo["qVerifier"], "queryVerifier": stark.query_verifier_of(info, exprs)}, "start": [str(v) for v in start], "publics": [str(v) for v in publics],
           "constRoot": _strs(setup["constRoot"]), "queries": res["queries"], "merkleTreeArity": arity, "merkleTreeCustom": custom}
    f = tmp_path / "job.json"
    f.write_text(json.dumps(job))
    out = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "prove_bn128.js"), str(f), "1"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "prove bn128 OK" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
    line = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    assert line["queries"] == [int(q) for q in res["queries"]]
    assert line["proofSha256"] == digest
    assert line["verified"] is True
