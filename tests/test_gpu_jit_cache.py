"""The evaluator's code objects on disk, where the kernels run: a process that finds its compiled kernel in the cache directory
compiles nothing and computes the same words (csrc/expr.hip; the host-only half is tests/test_jit_cache_cpu.py).  Every start is a
fresh child (tests/jit_cache_child.py) under its own time limit, one at a time.  Domains have 2^16 rows: the threshold from which the
evaluator chooses its compiled kernel unasked.  `no device` children run with every GPU hidden (HIP_VISIBLE_DEVICES empty)."""
import json
import os
import struct
import subprocess

import pytest

from test_jit_cache_cpu import ZERO, _cmd, counts, entries, files

pytestmark = pytest.mark.gpu
PROG = {"k": 50, "which": 0, "n_bits": 16, "prime_shift": 3, "seed": 5}
NO_GPU = {"HIP_VISIBLE_DEVICES": ""}
UNFORCED = {}


def _child(steps, env):
    """test_jit_cache_cpu.child forces PIL2GL_EXPR_JIT=1 for its small program; here the routing is the library's own unless a test says so"""
    e = {k: v for k, v in os.environ.items() if not k.startswith("PIL2GL_")}
    e.update(env)
    out = subprocess.run(_cmd(steps), capture_output=True, text=True, timeout=300, env=e)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    return json.loads(out.stdout.strip().splitlines()[-1])


@pytest.fixture(scope="module")
def restart(tmp_path_factory):
    """child A evaluates into an empty directory, child B starts again on the same directory -> (dir, A's results, B's results)"""
    d = tmp_path_factory.mktemp("restart")
    steps = [{"do": "set_dir", "dir": str(d)}, dict(PROG, do="eval"), {"do": "stats"}]
    return d, _child(steps, UNFORCED)[1:], _child(steps, UNFORCED)[1:]


def test_a_restarted_process_loads_the_kernel_instead_of_compiling_it(restart):
    """fibonacci_program(50, 0, 16, 3): both children bit-exact against the oracle on every row (evalpath.check_at_size, inside the child)
    through the compiled kernel; the first compiled and wrote, the second only read"""
    d, (ea, sa), (eb, sb) = restart
    assert ea["path"] == "jit" and eb["path"] == "jit" and ea["info"]["ops"] == eb["info"]["ops"]
    assert counts(sa) == dict(ZERO, compiles=1, diskWrites=1), sa
    assert counts(sb) == dict(ZERO, diskHits=1), sb
    assert len(entries(d)) == 1 and len(files(d)) == 1


def test_setup_on_a_host_without_a_device_then_prove(tmp_path):
    """child A only precompiles, with no GPU visible and no pil2gl_init; child B evaluates: one disk hit, no compile, bit-exact"""
    d = {"do": "set_dir", "dir": str(tmp_path)}
    ra = _child([d, dict(PROG, do="precompile")], NO_GPU)[1]
    assert ra["routed"] == "jit" and ra["origin"] == "compiled", ra
    eb, sb = _child([d, dict(PROG, do="eval"), {"do": "stats"}], UNFORCED)[1:]
    assert eb["path"] == "jit" and counts(sb) == dict(ZERO, diskHits=1), (eb, sb)


def test_a_damaged_entry_is_set_aside_on_the_device_path(restart, tmp_path):
    """one bit of the code object flipped: the checksum fails, the file is set aside before anything is loaded, the kernel compiled"""
    d = restart[0]
    blob = bytearray(open(entries(d)[0], "rb").read())
    hdr, = struct.unpack_from("<I", blob, 12); slen, clen = struct.unpack_from("<QQ", blob, 32)
    blob[hdr + slen + clen // 2] ^= 0x01
    f = tmp_path / os.path.basename(entries(d)[0])
    f.write_bytes(bytes(blob)); os.chmod(f, 0o600)
    e, s = _child([{"do": "set_dir", "dir": str(tmp_path)}, dict(PROG, do="eval"), {"do": "stats"}], UNFORCED)[1:]
    assert e["path"] == "jit" and counts(s) == dict(ZERO, rejected=1, compiles=1, diskWrites=1), (e, s)
    assert open(f, "rb").read() == open(entries(d)[0], "rb").read()


def test_a_whole_proof_after_stark_precompile_compiles_nothing(tmp_path):
    """fibonacci_air(50), nBits 13 / nBitsExt 16.  Child A: stark.precompile with no GPU visible.  Child B: stark.stark_gen on the GPU backend
    finds every compiled kernel on disk and its proof equals the oracle backend's field by field.  The program this AIR compiles is the
    constraint program, which the quotient stage evaluates on a sub-coset of 2^14 rows with section pitches x 4 and a smaller row shift:
    a precompile that encoded the full-domain context would leave B to compile.  2^14 rows are below the evaluator's own threshold for
    the compiled kernel, so both children run with PIL2GL_EXPR_JIT=1."""
    d = {"do": "set_dir", "dir": str(tmp_path)}
    job = {"k": 50, "n_bits": 13, "n_bits_ext": 16}
    pa = _child([d, dict(job, do="stark_precompile")], dict(NO_GPU, PIL2GL_EXPR_JIT="1"))[1]
    assert [p["origin"] for p in pa if p["routed"] == "jit"] == ["compiled"] and "sub-coset" in pa[-1]["program"], pa
    pb, sb = _child([d, dict(job, do="stark_prove"), {"do": "stats"}], {"PIL2GL_EXPR_JIT": "1"})[1:]
    assert pb["differing"] == [] and "evals" in pb["fields"] and "fri" in pb["fields"], pb
    assert sb["compiles"] == 0 and sb["diskHits"] >= 1 and sb["rejected"] == 0, sb
