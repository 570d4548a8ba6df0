"""The BN254 Fr hint operators from Node: js/polutils_bn128.js calculateZ / calculateS / batchInverse on arrays of Uint8Array(32) and on
resident DevBuffer columns, against the Python checker's bytes (tests/bn128_hints_ref.py).  The test writes a job, Node runs it as a
fresh child process and compares bytes."""
import json
import os
import shutil
import subprocess

import pytest

import bn128_hints_ref as ref
from conftest import ROOT

NODE = shutil.which("node")


def hx(vals):
    return ref.mont_words(vals).tobytes().hex()


def columns(n, seed, zeros=()):
    num, den = ref.rand_elems(n, seed), [v or 1 for v in ref.rand_elems(n, seed + 1000)]
    for i in zeros:
        den[i] = 0
    return num, den


@pytest.mark.gpu
@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_js_hint_operators_match_the_checker(tmp_path):
    job = {"arrays": []}
    for n, zeros in ((5, ()), (3000, (1234,))):
        num, den = columns(n, n, zeros)
        job["arrays"].append({"n": n, "num": hx(num), "den": hx(den), "z": hx(ref.gprod(num, den)), "s": hx(ref.gsum(num[0], den)),
                              "inv": hx(ref.batch_inverse(den))})
    n, width, dst_width = 1500, 3, 2
    num, den = columns(n, 7, (700,))
    section = ref.rand_elems(n * width, 8)
    section[0::width], section[2::width] = num, den
    dst = ref.rand_elems(n * dst_width, 9)
    want_dst = list(dst)
    z = ref.gprod(num, den)
    want_dst[1::dst_width], want_dst[0::dst_width] = z, ref.gsum(num[5], den)
    want_section = list(section)
    want_section[2::width] = ref.batch_inverse(den)
    job["resident"] = {"n": n, "width": width, "numCol": 0, "denCol": 2, "dstWidth": dst_width, "zCol": 1, "sCol": 0,
                       "section": hx(section), "dst": hx(dst), "numElem": hx([num[5]]), "wantDst": hx(want_dst), "wantResult": hx([z[n - 1]]),
                       "wantSection": hx(want_section)}
    path = tmp_path / "job.json"
    path.write_text(json.dumps(job))
    out = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "hints_bn128_parity.js"), str(path)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "hints bn128 parity OK" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
