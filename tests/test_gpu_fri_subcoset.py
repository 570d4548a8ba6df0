"""pil2gl_compute_fri_pol_dev (x / (x - xi), the row sums and the combination on the extended rows k << eb, then one unshifted extension)
against the full-domain chain it replaces (x_div_x_sub_xi -> rows_dot_ext_multi -> fri_combine_order on every extended row), word for
word, on the buffers of real proofs: the identity needs K built from the evaluations of the very columns, so matrices, evaluations and
challenges come from stark_gen itself.  The backend below takes stark_gen's one FRI-polynomial call, runs both forms on the same buffers
and stops the proof there.

Which row-sum kernels a case reaches follows from the widths of its matrices (dot.hip, rows_dot_mfma_plan: the matrix cores take side-by-side
matrices of 32..112 columns in all and one or two outputs per launch); each case states its widths and asserts them."""
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
        info, exprs, vinfo = stark.fibonacci_air(k, ss, prev_row=kind == "fib_prev")
        cm, consts, publics = stark.fibonacci_trace(n_bits, k)
    return stark, info, exprs, vinfo, cm, consts, publics


def _both_forms(air, n_bits, ext_bits):
    """the FRI polynomial of a proof of `air` both ways -> dict: new / old (2^nBitsExt x 3, host), widths (of the matrices summed), n_open"""
    import torch
    stark, info, exprs, vinfo, cm, consts, publics = _case(air, n_bits, ext_bits)
    box = {}

    class Both(stark.GpuBackend):
        def fri_polynomial(self, info, bufs, widths, evals, xis, vf1, vf2, nb, nbe, f_ext):
            f_ext.fill_(-1)                                # all-ones words: no canonical value, a row left unwritten cannot pass
            assert "xDivXSubXi_ext" not in bufs            # stark_gen builds no full-domain table on this path
            assert stark.GpuBackend.fri_polynomial(self, info, bufs, widths, evals, xis, vf1, vf2, nb, nbe, f_ext)
            full = dict(bufs, xDivXSubXi_ext=self.x_div_x_sub_xi(nbe, xis))
            old = self.empty(3 << nbe).fill_(-1)
            assert self.fri_polynomial_fast(info, full, widths, evals, vf1, vf2, nbe, old)
            torch.cuda.synchronize()
            names = list(stark.fri_polynomial_plan(info, evals, vf2)[0])
            box.update(new=self.to_host(f_ext).copy(), old=self.to_host(old).copy(), widths=sorted(widths[nm] for nm in names), n_open=len(xis))
            raise _Done()

    be = Both(0)
    setup = stark.build_const_tree(be, consts, info)
    with pytest.raises(_Done):
        stark.stark_gen(be, be.from_host(cm), setup, info, exprs, publics)
    return box


def _assert_equal(box):
    from conftest import P
    assert box["new"].max() < P and box["new"].any()
    bad = np.nonzero(box["new"] != box["old"])[0]
    assert bad.size == 0, ("words differ", bad.size, bad[:8].tolist())


@pytest.mark.parametrize("mfma", ["1", "0"])
def test_narrow_matrices_take_the_vector_kernels(mfma, monkeypatch):
    """2^10 x 2 (Fibonacci K = 1): cm1 2, cm2 6, constants 2 columns -- every matrix under 32 columns, no launch for the matrix cores;
    the same with PIL2GL_ROWS_DOT_MFMA=0"""
    monkeypatch.setenv("PIL2GL_ROWS_DOT_MFMA", mfma)
    box = _both_forms(("fib", 1), 10, 3)
    assert box["widths"] == [2, 2, 6] and box["n_open"] == 2
    _assert_equal(box)


@pytest.mark.parametrize("mfma", ["1", "0"])
def test_three_matrices_side_by_side_on_the_matrix_cores(mfma, monkeypatch):
    """2^10 x 100: 100 + 6 + 2 = 108 <= 112 columns, one launch of the matrix-core kernel with three segments; with
    PIL2GL_ROWS_DOT_MFMA=0 the 100 columns go through the streaming vector kernel (32 columns and more), the others through the column-tile one"""
    monkeypatch.setenv("PIL2GL_ROWS_DOT_MFMA", mfma)
    box = _both_forms(("fib", 50), 10, 3)
    assert box["widths"] == [2, 6, 100] and box["n_open"] == 2
    _assert_equal(box)


def test_column_windows():
    """2^8 x 120 (K = 60): wider than the staged row (112 columns) -- two windows of 60, packed with the narrow matrices into two
    accumulating launches"""
    box = _both_forms(("fib", 60), 8, 3)
    assert box["widths"] == [2, 6, 120]
    _assert_equal(box)


def test_odd_widths():
    """the permutation AIR with 9 copies: stages of 18 and 81 columns (81: an odd width, and an odd row pitch at step 0 only)"""
    box = _both_forms(("perm", 9), 8, 2)
    assert 18 in box["widths"] and 81 in box["widths"]
    _assert_equal(box)


def test_three_openings_take_two_sweeps_of_two():
    """openings -1, 0, 1 (the Horner order 0, 1, -1 is not that of openingPoints) on 32 + 6 + 2 columns: the matrix-core launch runs
    twice, outputs 0-1 then 2"""
    box = _both_forms(("fib_prev", 16), 8, 2)
    assert box["widths"] == [2, 6, 32] and box["n_open"] == 3
    _assert_equal(box)


@pytest.mark.parametrize("ext_bits", [1, 2, 3])
def test_every_extension(ext_bits):
    box = _both_forms(("fib", 3), 6, ext_bits)
    _assert_equal(box)


def test_multi_launch_transforms():
    """2^16 rows: the inverse side and the forward side of the extension both take several launches"""
    import transform_plan
    kinds = [l.kind for l in transform_plan.plan("interpolate", 16, 3, 1)]
    assert kinds.count("i") >= 2 and kinds.count("m") == 1 and kinds.count("d") >= 2, kinds
    _assert_equal(_both_forms(("fib", 1), 16, 1))


@pytest.mark.parametrize("air,n_bits,steps", [(("fib", 3), 10, [13, 9, 4]), (("perm", 1), 10, [12, 8, 3])])
def test_whole_proof_equals_the_oracle_proof(oracle, air, n_bits, steps):
    """OracleBackend has no fri_polynomial: it builds x / (x - xi) and interprets friExp on every extended row.  Equal dictionaries."""
    import stark_ref
    stark, info, exprs, vinfo, cm, consts, publics = _case(air, n_bits, steps[0] - n_bits, steps)
    gpu, cpu = stark.GpuBackend(0), stark_ref.OracleBackend()
    assert hasattr(gpu, "fri_polynomial") and not hasattr(cpu, "fri_polynomial")
    res = []
    for be in (gpu, cpu):
        setup = stark.build_const_tree(be, consts, info)
        res.append(stark.stark_gen(be, be.from_host(cm), setup, info, exprs, publics))
    assert res[0]["proof"] == res[1]["proof"]
    assert res[0]["challenges"] == res[1]["challenges"] and res[0]["queries"] == res[1]["queries"]


def _direct_call(n_bits, n_bits_ext, xis, n_open=None, order=None, chain=False):
    """the entry on one random 2^nBitsExt x 4 matrix (K random as well) -> (rc, fExt after); fExt starts as all-ones words.
    chain: the full-domain chain on the same inputs instead"""
    import torch
    import pil2gl
    from pil2gl import _lib
    from conftest import P
    pil2gl.init(0)
    n_open = len(xis) if n_open is None else n_open
    rows = 1 << max(n_bits, n_bits_ext)
    rng = np.random.default_rng(5)
    m = torch.from_numpy(rng.integers(0, P, size=rows * 4, dtype=np.uint64).view(np.int64)).cuda()
    f = torch.full((3 * rows,), -1, dtype=torch.int64, device="cuda")
    coef = rng.integers(0, P, size=(max(n_open, 1), 4, 3), dtype=np.uint64)
    K = rng.integers(0, P, size=(max(n_open, 1), 3), dtype=np.uint64)
    vf1 = np.array([3, 4, 5], dtype=np.uint64)
    od = np.array(list(range(n_open)) if order is None else order, dtype=np.uint32)
    xs = np.array(xis, dtype=np.uint64)
    ptrs = (C.c_void_p * 1)(m.data_ptr()); cps = (C.c_void_p * 1)(coef.ctypes.data)
    ws = np.array([4], dtype=np.uint64)
    if chain:
        E = 1 << n_bits_ext
        xd = torch.empty(3 * n_open * E, dtype=torch.int64, device="cuda"); acc = torch.empty_like(xd)
        for i in range(n_open):
            _lib.call("pil2gl_x_div_x_sub_xi_dev", n_bits_ext, C.c_void_p(xs[i].ctypes.data), n_open, i, C.c_void_p(xd.data_ptr()), None)
        _lib.call("pil2gl_rows_dot_ext_multi_dev", ptrs, C.c_void_p(ws.ctypes.data), 1, E, cps, n_open, C.c_void_p(acc.data_ptr()), 0, None)
        _lib.call("pil2gl_fri_combine_order_dev", C.c_void_p(acc.data_ptr()), C.c_void_p(K.ctypes.data), C.c_void_p(vf1.ctypes.data), C.c_void_p(xd.data_ptr()),
                  n_open, C.c_void_p(od.ctypes.data), E, C.c_void_p(f.data_ptr()), None)
        torch.cuda.synchronize()
        return 0, f.cpu().numpy()
    rc = _lib.load().pil2gl_compute_fri_pol_dev(ptrs, C.c_void_p(ws.ctypes.data), 1, cps, n_open, C.c_void_p(K.ctypes.data), C.c_void_p(vf1.ctypes.data),
                                                C.c_void_p(od.ctypes.data), C.c_void_p(xs.ctypes.data), n_bits, n_bits_ext, C.c_void_p(f.data_ptr()), None)
    torch.cuda.synchronize()
    return rc, f.cpu().numpy()


def test_without_an_extension_the_entry_is_the_full_domain_sequence():
    """nBitsExt == nBits (no proof has that shape: the quotient needs room): nothing to extend, and no condition on K"""
    from conftest import P
    xis = [[9, 8, 7], [1, 2, 3], [5, 0, 0]]
    rc, new = _direct_call(7, 7, xis, order=[1, 2, 0])
    _, old = _direct_call(7, 7, xis, order=[1, 2, 0], chain=True)
    assert rc == 0 and new.view(np.uint64).max() < P and np.array_equal(new, old)


def test_refusals_write_nothing():
    from pil2gl import stark
    from conftest import P
    nb, nbe = 5, 8
    wE = stark.root_of_unity(nbe)
    off = [9, 8, 7]                                                            # an extension element: never a row
    for k in (3, 6, 8):                                                        # rows not divisible by 2^eb = 8, and one that is
        rc, f = _direct_call(nb, nbe, [off, [7 * pow(wE, k, P) % P, 0, 0]])
        assert rc == -1 and (f == -1).all(), k
    rc, f = _direct_call(6, 5, [off])                                          # nBitsExt < nBits
    assert rc == -1 and (f == -1).all()
    for n_open in (0, 5):
        rc, f = _direct_call(nb, nbe, [off] * 5, n_open=n_open)
        assert rc == -1 and (f == -1).all()
    rc, f = _direct_call(nb, nbe, [off, [1, 2, 3]], order=[1, 1])              # no permutation
    assert rc == -1 and (f == -1).all()
    rc, f = _direct_call(nb, nbe, [off, [pow(wE, 3, P), 0, 0]])                # w_E^3 without the shift is no row of 7 <w_E>: runs
    assert rc == 0 and not (f == -1).any()


@pytest.mark.parametrize("widths,n_out", [([2, 6], 2), ([100, 6, 2], 2), ([120, 2], 1), ([81, 18], 2), ([33, 6], 3), ([40], 4)])
def test_stepped_row_sums_equal_the_dense_ones_on_gathered_rows(widths, n_out):
    """pil2gl_rows_dot_ext_multi_step_dev with step bits 0..3 against pil2gl_rows_dot_ext_multi_dev on a gathered copy of the rows it
    visits; 200 rows: four 64-row tiles, the last one ragged.  Widths: vector kernels; one matrix-core launch; column windows; odd
    widths; three and four outputs (two sweeps of two)"""
    import torch
    import pil2gl
    from pil2gl import _lib
    from conftest import P
    pil2gl.init(0)
    n_rows = 200
    rng = np.random.default_rng(11)
    coefs = [rng.integers(0, P, size=(n_out, w, 3), dtype=np.uint64) for w in widths]
    cps = (C.c_void_p * len(widths))(*[c.ctypes.data for c in coefs])
    ws = np.array(widths, dtype=np.uint64)
    lib = _lib.load()
    for step in range(4):
        mats = [torch.from_numpy(rng.integers(0, P, size=((n_rows << step), w), dtype=np.uint64).view(np.int64)).cuda() for w in widths]
        gathered = [m[::1 << step].contiguous() for m in mats]
        out = []
        for stepped in (True, False):
            acc = torch.full((n_rows * n_out * 3,), -1, dtype=torch.int64, device="cuda")
            src = mats if stepped else gathered
            ptrs = (C.c_void_p * len(widths))(*[m.data_ptr() for m in src])
            if stepped:
                rc = lib.pil2gl_rows_dot_ext_multi_step_dev(ptrs, C.c_void_p(ws.ctypes.data), len(widths), n_rows, step, cps, n_out, C.c_void_p(acc.data_ptr()), 0, None)
            else:
                rc = lib.pil2gl_rows_dot_ext_multi_dev(ptrs, C.c_void_p(ws.ctypes.data), len(widths), n_rows, cps, n_out, C.c_void_p(acc.data_ptr()), 0, None)
            assert rc == 0, lib.pil2gl_last_error()
            torch.cuda.synchronize()
            out.append(acc.cpu().numpy().view(np.uint64))
        assert out[0].max() < P and np.array_equal(out[0], out[1]), step
    # one value by hand: row 1 of the last step, output 0, component 0
    m0 = [m.cpu().numpy().view(np.uint64)[8] for m in mats]
    want = sum(int(v) * int(c) for m, cf in zip(m0, coefs) for v, c in zip(m, cf[0, :, 0])) % P
    assert int(out[0][n_out * 3]) == want
