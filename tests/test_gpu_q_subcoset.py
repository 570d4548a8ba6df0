"""pil2gl_compute_q_stark_dev (the constraint program on the extended rows k * 2^s that fix Q, then ifft, split, extension) against the
full-domain sequence it replaces (eval_program on every extended row -> ifft -> q_extend), on the buffers of a real proof: the argument
holds for a satisfied AIR, so the sections come from stark_gen itself.  The backend below takes stark_gen's one quotient call, runs both
forms on the same buffers and stops the proof there."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


class _Done(Exception):
    pass


def _case(air, n_bits, ext_bits, steps=None):
    from pil2gl import stark
    nbe = n_bits + ext_bits
    ss = {"nBits": n_bits, "nBitsExt": nbe, "nQueries": 8, "verificationHashType": "GL", "steps": [{"nBits": b} for b in (steps or [nbe])]}
    kind, k = air
    if kind == "perm":
        info, exprs, vinfo = stark.permutation_air(ss, copies=k)
        cm, consts, publics = stark.permutation_trace(n_bits, copies=k)
    else:
        info, exprs, vinfo = stark.fibonacci_air(k, ss, prev_row=kind == "fib_prev", im_pols=kind == "fib_im")
        cm, consts, publics = stark.fibonacci_trace(n_bits, k, im_pols=kind == "fib_im")
    return stark, info, exprs, vinfo, cm, consts, publics


def _both_forms(air, n_bits, ext_bits, capfd, monkeypatch):
    """the quotient stage of a proof of `air` both ways.  Returns a dict: new / old (the 2^nBitsExt x qDim*qDeg matrices, host), path
    (evalpath.eval_path of the new call: the kernel that ran on the sub-domain), old_jit (compiled launches of the full-domain program),
    n_ops, s, m"""
    import torch
    import evalpath
    stark, info, exprs, vinfo, cm, consts, publics = _case(air, n_bits, ext_bits)
    box = {}

    class Both(stark.GpuBackend):
        def q_stark(self, ops, n_tmp, sections, scalars, q_section, nb, nbe, qDim, qDeg, out):
            m = nb + (qDeg - 1).bit_length()
            s = nbe - m
            out.fill_(-1)                                  # all-ones words: no canonical value, a row left unwritten cannot pass
            sub_widths = [w if i == q_section else w << s for i, (_, w) in enumerate(sections)]
            new_call = lambda: stark.GpuBackend.q_stark(self, ops, n_tmp, sections, scalars, q_section, nb, nbe, qDim, qDeg, out)
            box["path"] = evalpath.eval_path(capfd, monkeypatch, new_call, ops, n_tmp, sub_widths, scalars, m, nbe - nb - s)
            q_ext = self.empty(qDim << nbe).fill_(-1)
            full = [(q_ext, w) if i == q_section else (t, w) for i, (t, w) in enumerate(sections)]
            box["old_jit"] = evalpath.jit_launches(capfd, monkeypatch, lambda: self.eval_program(ops, n_tmp, full, scalars, nbe, nbe - nb))
            qq1 = self.empty(qDim << nbe)
            self.ifft(q_ext, qDim, nbe, qq1)
            old = self.empty((qDim * qDeg) << nbe).fill_(-1)
            self.q_extend(qq1, nb, nbe, qDim, qDeg, old)
            torch.cuda.synchronize()
            box.update(new=self.to_host(out).copy(), old=self.to_host(old).copy(), s=s, m=m,
                       n_ops=evalpath.plan(ops, n_tmp, sub_widths, scalars, m, nbe - nb - s)[1], q_ptr=sections[q_section][0])
            raise _Done()

    be = Both(0)
    setup = stark.build_const_tree(be, consts, info)
    with pytest.raises(_Done):
        stark.stark_gen(be, be.from_host(cm), setup, info, exprs, publics)
    assert box["q_ptr"] is None                            # stark_gen allocates no q_ext on this path
    return box


def _assert_equal(box):
    from conftest import P
    assert box["new"].max() < P and box["new"].any()
    bad = np.nonzero(box["new"] != box["old"])[0]
    assert bad.size == 0, ("words differ", bad[:8].tolist())


@pytest.mark.parametrize("ext_bits", [1, 2, 3, 4])
def test_interpreter_path_on_every_sub_domain_step(ext_bits, capfd, monkeypatch):
    """Fibonacci K = 1 (qDeg 2), 2^5 rows: s = 0 (the full domain through the same entry), 1, 2, 3"""
    box = _both_forms(("fib", 1), 5, ext_bits, capfd, monkeypatch)
    assert box["s"] == ext_bits - 1 and box["path"][0] == "interp" and box["old_jit"] == []
    _assert_equal(box)


def test_compiled_path_on_the_sub_domain(capfd, monkeypatch):
    """>= 64 ops and 2^16 sub-domain rows: the run-time compiled kernel, with the row pitch in its source"""
    box = _both_forms(("fib", 6), 15, 3, capfd, monkeypatch)
    assert box["n_ops"] >= 64 and box["m"] == 16 and box["s"] == 2
    assert box["path"][0] == "jit", box["path"]
    assert len(box["old_jit"]) == 1
    _assert_equal(box)


def test_sub_domain_below_the_compile_threshold_takes_the_interpreter(capfd, monkeypatch):
    """the same program at 2^14: the sub-domain has 2^15 rows (interpreter) where the full domain of 2^17 compiles"""
    box = _both_forms(("fib", 6), 14, 3, capfd, monkeypatch)
    assert box["n_ops"] >= 64 and box["m"] == 15
    assert box["path"][0] == "interp", box["path"]
    assert len(box["old_jit"]) == 1
    _assert_equal(box)


@pytest.mark.parametrize("air", [("fib_prev", 1), ("perm", 1), ("fib_im", 1)])
def test_row_offsets_more_sections_and_an_odd_width(air, capfd, monkeypatch):
    """fib_prev: openings -1, 0, 1 -- a negative row offset wraps at the sub-domain's end; perm: two witness stages; fib_im: cm1 has
    three columns (an odd row pitch before the shift)"""
    box = _both_forms(air, 6, 3, capfd, monkeypatch)
    assert box["s"] == 2
    _assert_equal(box)


@pytest.mark.parametrize("air,n_bits,steps", [(("fib", 4), 10, [13, 9, 4]), (("perm", 1), 8, [11, 7, 3])])
def test_whole_proof_equals_the_oracle_proof(oracle, air, n_bits, steps):
    """OracleBackend has no q_stark: it evaluates every extended row.  The proofs are equal dictionaries."""
    import stark_ref
    stark, info, exprs, vinfo, cm, consts, publics = _case(air, n_bits, steps[0] - n_bits, steps)
    gpu, cpu = stark.GpuBackend(0), stark_ref.OracleBackend()
    assert hasattr(gpu, "q_stark") and not hasattr(cpu, "q_stark")
    res = []
    for be in (gpu, cpu):
        setup = stark.build_const_tree(be, consts, info)
        res.append(stark.stark_gen(be, be.from_host(cm), setup, info, exprs, publics))
    assert res[0]["proof"] == res[1]["proof"]
    assert res[0]["challenges"] == res[1]["challenges"] and res[0]["queries"] == res[1]["queries"]


def _tiny_call(n_bits, n_bits_ext, q_deg, op_src, prime_shift, dest_section=0):
    """one copy op into section `dest_section` of a two-section context (0: the quotient's, 1: one column); returns (rc, dst after)"""
    import torch
    from pil2gl import _lib, stark
    import pil2gl
    pil2gl.init(0)
    E = 1 << n_bits_ext
    x = torch.arange(E, dtype=torch.int64, device="cuda")
    dst = torch.full((3 * q_deg * E,), -1, dtype=torch.int64, device="cuda")
    prog = stark.make_c_program([(stark.OPC["copy"], (stark.SEC, 3 if dest_section == 0 else 1, dest_section, 0, 0), op_src, None)], 0)
    cs = (_lib.GlxSection * 2)()
    cs[0].ptr = None; cs[0].width = 3
    cs[1].ptr = x.data_ptr(); cs[1].width = 1
    scalars = np.array([5], dtype=np.uint64)
    ctx = _lib.GlxCtx(n_bits_ext, prime_shift, 2, 1, cs, scalars.ctypes.data_as(_lib.u64p))
    rc = _lib.load().pil2gl_compute_q_stark_dev(C.byref(prog), C.byref(ctx), 0, n_bits, n_bits_ext, 3, q_deg, C.c_void_p(dst.data_ptr()), None)
    torch.cuda.synchronize()
    return rc, dst.cpu().numpy()


def test_refusals_write_nothing():
    from pil2gl import stark
    scalar = (stark.SCALAR, 1, 0, 0, 0)
    rc, dst = _tiny_call(5, 5, 2, scalar, 0)                                   # qDeg * N > 2^nBitsExt
    assert rc == -1 and (dst == -1).all()
    rc, dst = _tiny_call(5, 8, 2, (stark.SEC, 1, 1, 1, 0), 0)                  # row offset 1 << 0 is not a row k * 2^2
    assert rc == -1 and (dst == -1).all()
    rc, dst = _tiny_call(5, 8, 2, scalar, 3, dest_section=1)                   # writes a section that is not the quotient's
    assert rc == -1 and (dst == -1).all()
    rc, dst = _tiny_call(5, 8, 2, (stark.SEC, 1, 1, 1, 0), 3)                  # the same read with primeShift = nBitsExt - nBits runs
    assert rc == 0 and not (dst == -1).any()
