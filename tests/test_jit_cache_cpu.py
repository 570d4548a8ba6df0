"""The evaluator's code objects on disk (csrc/expr.hip, `code objects kept on disk`; include/pil2gl.h pil2gl_jit_cache_set_dir,
pil2gl_jit_cache_stats, pil2gl_precompile_program), without a GPU: hiprtc compiles for gfx950 on any host.  The cache state lives as long
as a process, so every start is a fresh child (tests/jit_cache_child.py) under its own time limit; at most four run at once.
The program is evalpath.fibonacci_program(10, 0, 16, 3, seed) with PIL2GL_EXPR_JIT=1: about a second of compile.
A clean compile of it is made once (the `clean` fixture) and shared read-only by the tests that compare bytes against it."""
import glob
import json
import os
import struct
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CHILD = os.path.join(HERE, "jit_cache_child.py")
PROG = {"k": 10, "which": 0, "n_bits": 16, "prime_shift": 3, "seed": 1}
PRE = dict(PROG, do="precompile")
ZERO = {"memoryHits": 0, "diskHits": 0, "compiles": 0, "diskWrites": 0, "rejected": 0, "failedWrites": 0}


def _env(extra=None):
    env = {k: v for k, v in os.environ.items() if not k.startswith("PIL2GL_")}
    env["PIL2GL_EXPR_JIT"] = "1"
    env.update(extra or {})
    return env


def _cmd(steps):
    return [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [CHILD, json.dumps(steps)]


def child(steps, env=None):
    out = subprocess.run(_cmd(steps), capture_output=True, text=True, timeout=300, env=_env(env))
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    return json.loads(out.stdout.strip().splitlines()[-1])


def counts(st):
    return {k: st[k] for k in ZERO}


def files(d):
    return sorted(os.listdir(d))


def entries(d):
    return sorted(glob.glob(os.path.join(str(d), "*.p2gl")))


@pytest.fixture(scope="module")
def clean(tmp_path_factory):
    """(file name, bytes) of the program's entry as a first precompile into an empty directory writes it"""
    d = tmp_path_factory.mktemp("clean")
    res, st = child([{"do": "set_dir", "dir": str(d)}, PRE, {"do": "stats"}])[1:]
    assert res["routed"] == "jit" and res["origin"] == "compiled" and res["codeBytes"] > 1000, res
    assert counts(st) == dict(ZERO, compiles=1, diskWrites=1), st
    assert len(entries(d)) == 1 and files(d) == [os.path.basename(entries(d)[0])], files(d)       # one entry, no temporary file left
    return os.path.basename(entries(d)[0]), open(entries(d)[0], "rb").read()


def test_without_a_directory_nothing_is_cached():
    res, st = child([PRE, {"do": "stats"}])
    assert "error" in res and "no jit cache directory" in res["error"], res
    assert all(v == 0 for v in st.values()), st


def test_first_call_writes_one_private_file(clean, tmp_path):
    name, blob = clean
    d = tmp_path / "c"                                              # missing: set_dir creates it, mode 0700
    child([{"do": "set_dir", "dir": str(d)}, PRE])
    assert files(d) == [name] and open(d / name, "rb").read() == blob
    assert os.stat(d / name).st_mode & 0o7777 == 0o600 and os.stat(d).st_mode & 0o7777 == 0o700
    assert len(name) == 32 + len(".p2gl") and int(name[:32], 16) >= 0
    # the layout include/pil2gl.h documents
    magic, ver, hdr, major, minor, alen, olen, slen, clen = struct.unpack_from("<8sIIIIIIQQ", blob, 0)
    assert magic == b"P2GLJIT\0" and ver == 1 and hdr == 64 + alen + olen and hdr + slen + clen == len(blob)
    assert blob[64:64 + alen] == b"gfx950" and blob[64 + alen:hdr].split(b"\n") == [b"--offload-arch=gfx950", b"-O3", b"-ffp-contract=off"]
    assert b"jit_eval" in blob[hdr:hdr + slen] and blob[hdr + slen:hdr + slen + 4] == b"\x7fELF"


def test_a_second_process_finds_it(clean, tmp_path):
    name, blob = clean
    (tmp_path / name).write_bytes(blob); os.chmod(tmp_path / name, 0o600)
    res, st = child([PRE, {"do": "stats"}], env={"PIL2GL_JIT_CACHE_DIR": str(tmp_path)})          # the directory from the environment
    assert res["origin"] == "disk" and res["routed"] == "jit" and res["codeBytes"] == struct.unpack_from("<Q", blob, 40)[0]
    assert counts(st) == dict(ZERO, diskHits=1), st
    assert files(tmp_path) == [name] and open(tmp_path / name, "rb").read() == blob


def test_what_decides_the_kernel_moves_the_key_and_scalar_values_do_not(clean, tmp_path):
    name, blob = clean
    (tmp_path / name).write_bytes(blob); os.chmod(tmp_path / name, 0o600)
    d = {"do": "set_dir", "dir": str(tmp_path)}
    # other challenges / evaluations / publics: the same kernel, found on disk
    res, st = child([d, dict(PRE, scalar_seed=77), {"do": "stats"}])[1:]
    assert res["origin"] == "disk" and counts(st) == dict(ZERO, diskHits=1) and files(tmp_path) == [name]
    seen = {name}
    for change, env in ((dict(PRE, widen=1), None), (dict(PRE, ctx_prime_shift=2), None), (PRE, {"PIL2GL_EXPR_MULCALL": "1"})):
        res = child([d, change], env=env)[1]
        assert res["origin"] == "compiled", (change, env, res)
        new = set(files(tmp_path)) - seen
        assert len(new) == 1 and new.pop().endswith(".p2gl"), (change, env, files(tmp_path))
        seen = set(files(tmp_path))
    assert len(seen) == 4 and open(tmp_path / name, "rb").read() == blob


def _damage(case, blob):
    magic, ver, hdr, major, minor, alen, olen, slen, clen = struct.unpack_from("<8sIIIIIIQQ", blob, 0)
    b = bytearray(blob)
    if case == "truncated":
        return bytes(b[:-1])
    if case == "payload":
        b[hdr + slen + clen // 2] ^= 0x01
    elif case == "arch":
        assert b[64:70] == b"gfx950"; b[64:70] = b"gfx942"
    elif case == "hiprtc":
        struct.pack_into("<I", b, 20, minor + 1)
    elif case == "source":
        at = hdr + bytes(b[hdr:hdr + slen]).index(b"jit_eval")
        b[at] = ord("k")
    return bytes(b)


@pytest.mark.parametrize("case", ["truncated", "payload", "arch", "hiprtc", "source"])
def test_a_damaged_entry_is_set_aside_and_replaced(clean, tmp_path, case):
    name, blob = clean
    bad = _damage(case, blob)
    assert bad != blob
    (tmp_path / name).write_bytes(bad); os.chmod(tmp_path / name, 0o600)
    res, st = child([{"do": "set_dir", "dir": str(tmp_path)}, PRE, {"do": "stats"}])[1:]
    assert res["origin"] == "compiled" and counts(st) == dict(ZERO, rejected=1, compiles=1, diskWrites=1), (res, st)
    assert files(tmp_path) == [name] and open(tmp_path / name, "rb").read() == blob


def test_four_processes_fill_one_directory_at_once(clean, tmp_path):
    name, blob = clean
    steps = [{"do": "set_dir", "dir": str(tmp_path)}, PRE, {"do": "stats"}]
    procs = [subprocess.Popen(_cmd(steps), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=_env()) for _ in range(4)]
    outs = []
    try:
        for p in procs:
            outs.append(p.communicate(timeout=300) + (p.returncode,))
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    for so, se, rc in outs:
        assert rc == 0, so[-1000:] + se[-3000:]
        res, st = json.loads(so.strip().splitlines()[-1])[1:]
        assert res["routed"] == "jit" and res["origin"] in ("compiled", "disk") and st["failedWrites"] == 0 and st["rejected"] == 0, (res, st)
    assert files(tmp_path) == [name] and open(tmp_path / name, "rb").read() == blob


def test_a_program_for_the_interpreter_writes_nothing(tmp_path):
    """the reference's verifyEvals program: 331 slots after optimisation, over the compiled kernel's cap of 200 even when PIL2GL_EXPR_JIT=1 asks for it"""
    res, st = child([{"do": "set_dir", "dir": str(tmp_path)}, {"do": "precompile_verify_evals", "n_bits": 16}, {"do": "stats"}])[1:]
    assert res["ops"] == 3258 and res["routed"] == "interp" and res["origin"] == "none" and res["codeBytes"] == 0 and res["slots"] == 331, res
    assert counts(st) == ZERO and files(tmp_path) == []


def test_a_write_that_fails_is_counted_and_nothing_else(tmp_path):
    """the directory stops taking files after set_dir (mode 0500; for root, whom modes do not stop, it is removed): every call still
    succeeds, the failed writes are counted, and pil2gl_last_error says what it said before"""
    d = tmp_path / "c"
    out = child([{"do": "set_dir", "dir": str(d)}, {"do": "last_error"}, {"do": "lock_dir", "dir": str(d)}, PRE, PRE, {"do": "last_error"}, {"do": "stats"}])
    err0, r1, r2, err1, st = out[1], out[3], out[4], out[5], out[6]
    assert r1["origin"] == "compiled" and r2["origin"] == "compiled" and r1["codeBytes"] == r2["codeBytes"] > 1000, (r1, r2)
    assert err1 == err0
    assert counts(st) == dict(ZERO, compiles=2, failedWrites=2), st
    if os.path.isdir(d):
        os.chmod(d, 0o700)
        assert files(d) == []


def test_a_directory_that_cannot_serve_is_refused(tmp_path):
    f = tmp_path / "file"
    f.write_text("x")
    good = tmp_path / "good"
    r = child([{"do": "set_dir", "dir": str(good)}, {"do": "try_set_dir", "dir": str(f / "sub")}, {"do": "try_set_dir", "dir": str(f)}, PRE])
    assert "jit cache directory" in r[1] and "-1" in r[1] and "jit cache directory" in r[2], r
    assert r[3]["origin"] == "compiled" and len(entries(good)) == 1             # the earlier setting stayed
