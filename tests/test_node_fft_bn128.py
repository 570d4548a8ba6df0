"""The BN254 Fr transforms from Node: the drop-in js/fft_p_bn128.js over a Uint8Array, a chunked BigBuffer-shaped object and DevBuffers,
against bytes the Python checker (tests/bn128_fft_ref.py) wrote.  Node runs as a fresh child process."""
import json
import os
import random
import shutil
import subprocess

import pytest

import bn128_fft_ref as ref
from conftest import ROOT

NODE = shutil.which("node")


def _hex(words):
    return words.astype("<u8").tobytes().hex()


def _job():
    cases = []
    rng = random.Random(2024)
    for op, n_bits, n_pols, ext in (("fft", 5, 2, 0), ("ifft", 5, 2, 0), ("interpolate", 3, 1, 1), ("interpolate", 10, 3, 2)):
        cols = [[rng.randrange(ref.R) for _ in range(1 << n_bits)] for _ in range(n_pols)]
        case = {"op": op, "nBits": n_bits, "nPols": n_pols, "nBitsExt": n_bits + ext, "input": _hex(ref.matrix_words(cols))}
        if op == "interpolate":
            both = [ref.interpolate(c, n_bits + ext) for c in cols]
            case["coefs"] = _hex(ref.matrix_words([c for c, _ in both]))
            case["expected"] = _hex(ref.matrix_words([e for _, e in both]))
        else:
            case["expected"] = _hex(ref.matrix_words([(ref.ntt if op == "fft" else ref.intt)(c) for c in cols]))
        cases.append(case)
    return {"cases": cases}


@pytest.mark.gpu
@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_js_drop_in_matches_the_checker_three_ways(tmp_path):
    job = tmp_path / "fft_bn128_job.json"
    job.write_text(json.dumps(_job()))
    out = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "fft_bn128_parity.js"), str(job)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "fft bn128 parity OK" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
