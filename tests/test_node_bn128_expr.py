"""The BN254 Fr expression evaluator from Node: js/prover_helpers_bn128.js calculateExps / callCalculateExps over DevBuffer sections, on
domain n and on ext with ret, and the debug path's first failing row, against BigInt arithmetic the script computes itself.  Node runs
as a fresh child process."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

NODE = shutil.which("node")


@pytest.mark.gpu
@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_js_calculate_exps_over_fr_matches_bigint_arithmetic():
    out = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "expr_bn128_parity.js")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "expr bn128 parity OK" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
