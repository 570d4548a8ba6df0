"""The byte-staging scope the BN254 Node drop-ins share (js/bn128_stage.js), driven without a GPU: tests/js/bn128_stage_unit.js hands it
a stand-in for the addon's memory calls and a 64-byte piece size, and asserts on the call log and the bytes."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

NODE = shutil.which("node")


@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_staging_scope_pieces_roles_and_cleanup():
    out = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "bn128_stage_unit.js")], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "bn128 stage unit OK" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
