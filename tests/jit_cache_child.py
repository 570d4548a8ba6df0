"""One fresh process of the code-object cache tests (tests/test_jit_cache_cpu.py, tests/test_gpu_jit_cache.py): the library's cache
state -- directory, counters, the in-memory map -- lives as long as the process, so every `start` of those tests is a child running this
file.  Usage: python jit_cache_child.py '<json list of steps>'; the steps run in order and the last line printed is the JSON list of
their results.  Steps ({"do": name, ...}):
  set_dir {dir}                  pil2gl.jit_cache_set_dir
  try_set_dir {dir}              the same -> None, or the error's text
  stats                          pil2gl.jit_cache_stats()
  precompile {k, which, n_bits, prime_shift, seed, widen?: section index, scalar_seed?}
                                 evalpath.fibonacci_program(k, which, n_bits, prime_shift, seed) through pil2gl.precompile_program; widen: that
                                 section one column wider; scalar_seed: the same program encoded with other challenges / evaluations / publics
  precompile_verify_evals {n_bits}   the reference's 3 257-op verifyEvals program (tests/test_ref_oplist.py)
  lock_dir {dir}                 make the directory refuse new files: mode 0500 -- and, for a user whom modes do not stop (root), removed
  last_error                     pil2gl_last_error()
  eval {k, which, n_bits, prime_shift, seed}     (GPU) evalpath.check_at_size on the whole domain -> the path taken
  stark_precompile {k, n_bits, n_bits_ext}       stark.precompile of fibonacci_air(k)
  stark_prove {k, n_bits, n_bits_ext}            (GPU) stark.stark_gen on the GPU backend and on the oracle backend -> equal proofs?
None of the steps before `eval` touches a device."""
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [HERE, ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "pil2-stark-js_amd", "python")]


class _Env:
    """what evalpath's helpers use of pytest's monkeypatch"""
    def setenv(self, k, v): os.environ[k] = v
    def delenv(self, k, raising=True): os.environ.pop(k, None)


class _Fd2:
    """what evalpath's helpers use of pytest's capfd: the text written to file descriptor 2 since the last readouterr()"""
    def __init__(self):
        self.f = tempfile.TemporaryFile()
        self.saved = os.dup(2)
        os.dup2(self.f.fileno(), 2)
        self.pos = 0

    def readouterr(self):
        sys.stderr.flush()
        self.f.seek(self.pos)
        text = self.f.read().decode(errors="replace")
        self.pos += len(text.encode())
        return "", text

    def close(self):
        os.dup2(self.saved, 2)


def _fib(st):
    import evalpath
    return evalpath.fibonacci_program(st["k"], st["which"], st["n_bits"], st["prime_shift"], st["seed"])


def _stark_struct(st):
    nbe = st["n_bits_ext"]
    return {"nBits": st["n_bits"], "nBitsExt": nbe, "nQueries": 8, "verificationHashType": "GL", "steps": [{"nBits": b} for b in (nbe, nbe - 5, nbe - 10)]}


def step(st):
    import numpy as np
    import pil2gl
    do = st["do"]
    if do == "set_dir":
        pil2gl.jit_cache_set_dir(st["dir"]); return None
    if do == "try_set_dir":
        try:
            pil2gl.jit_cache_set_dir(st["dir"]); return None
        except pil2gl.Pil2glError as e:
            return str(e)
    if do == "stats":
        return pil2gl.jit_cache_stats()
    if do == "last_error":
        return (pil2gl.load().pil2gl_last_error() or b"").decode()
    if do == "lock_dir":
        os.chmod(st["dir"], 0o500)
        if os.access(st["dir"], os.W_OK):
            for f in os.listdir(st["dir"]):
                os.remove(os.path.join(st["dir"], f))
            os.rmdir(st["dir"])
        return None
    if do == "precompile":
        from pil2gl import stark
        pr = _fib(st)
        ops, n_tmp, scalars = pr["ops"], pr["n_tmp"], pr["scalars"]
        if "scalar_seed" in st:
            rng = np.random.default_rng(st["scalar_seed"])
            r3 = lambda: [int(v) for v in rng.integers(0, pil2gl.P, 3, dtype=np.uint64)]
            ctx = dict(pr["ctx"], publics=[int(v) for v in rng.integers(0, pil2gl.P, 3, dtype=np.uint64)],
                       challenges=[[], [r3()], [r3()], [r3(), r3()]], evals=[r3() for _ in pr["ctx"]["evals"]])
            ops, n_tmp, names, scalars = stark.encode_code(pr["code"], "ext", ctx)
            assert names == pr["names"] and not (scalars == pr["scalars"]).all()
        widths = [s.shape[1] for s in pr["secs"]]
        if "widen" in st:
            widths[st["widen"]] += 1
        try:
            return pil2gl.precompile_program(ops, n_tmp, widths, scalars, pr["n_bits"], st.get("ctx_prime_shift", pr["prime_shift"]))
        except pil2gl.Pil2glError as e:
            return {"error": str(e)}
    if do == "precompile_verify_evals":
        from pil2gl import stark
        import test_ref_oplist
        inp = test_ref_oplist._inputs(4)
        ctx = {"pilInfo": {}, "publics": inp["publics"], "evals": inp["evals"], "challengesFlat": inp["challengesFlat"], "challenges": []}
        ops, n_tmp, secs, scalars = stark.encode_code(test_ref_oplist._load(), "ext", ctx)
        return dict(pil2gl.precompile_program(ops, n_tmp, [3] * len(secs), scalars, st["n_bits"], 0), ops=len(ops))
    if do == "eval":
        import evalpath
        import gl_oracle
        gl_oracle.build(); gl_oracle.set_threads(8)
        cap = _Fd2()
        try:
            path, info = evalpath.check_at_size(gl_oracle, cap, _Env(), _fib(st))
        finally:
            cap.close()
        return {"path": path, "info": info}
    if do == "stark_precompile":
        from pil2gl import stark
        info, exprs, _ = stark.fibonacci_air(st["k"], _stark_struct(st))
        return stark.precompile(info, exprs)
    if do == "stark_prove":
        import gl_oracle
        from pil2gl import stark
        from stark_backend import OracleBackend
        gl_oracle.build(); gl_oracle.set_threads(8)
        info, exprs, _ = stark.fibonacci_air(st["k"], _stark_struct(st))
        cm, consts, publics = stark.fibonacci_trace(st["n_bits"], st["k"])
        res = []
        for be in (stark.GpuBackend(0), OracleBackend()):
            setup = stark.build_const_tree(be, consts, info)
            res.append(stark.stark_gen(be, be.from_host(cm), setup, info, exprs, publics)["proof"])
        differing = sorted(k for k in set(res[0]) | set(res[1]) if res[0].get(k) != res[1].get(k))
        return {"fields": sorted(res[0]), "differing": differing}
    raise ValueError(do)


if __name__ == "__main__":
    out = [step(s) for s in json.loads(sys.argv[1])]
    print(json.dumps(out))
