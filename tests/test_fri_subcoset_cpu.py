"""The argument pil2gl_compute_fri_pol_dev rests on, stated with the oracle alone (no GPU).

F(x) = sum_o (sum_c coef_{o,c} col_c(x) - K_o) x / (x - xi_o).  Every column has degree < N and K_o is built from the evaluations the
prover took from those same columns, so each bracket vanishes at xi_o and deg F < N -- for any witness, since nothing here asks the AIR
to hold.  The extended rows k * 2^eb are the coset 7 <w_N>: the size-N inverse transform of F's values there gives the coefficients of
F(7x), and the plain transform of those coefficients, zero-padded to 2^nBitsExt rows, gives F on every extended row.

The oracle's full-domain f_ext is taken from a proof on OracleBackend (it has no fri_polynomial method: x / (x - xi) on every extended
row, friExp interpreted on every extended row): the backend below stops the proof where FRI first reads the polynomial."""
import numpy as np
import pytest

from conftest import P


class _Captured(Exception):
    pass


_cache = {}


def _oracle_f_ext(oracle, air, n_bits, ext_bits, corrupt=None, bend_eval=None):
    """f_ext (2^nBitsExt x 3) of the oracle's proof of `air` at these sizes.  corrupt: a witness cell to move by one; bend_eval: the index
    of an evaluation to move by one before the FRI polynomial is built from it.  Computed once per case."""
    key = (air, n_bits, ext_bits, corrupt, bend_eval)
    if key in _cache:
        return _cache[key]
    import stark_ref
    from pil2gl import stark
    nbe = n_bits + ext_bits
    ss = {"nBits": n_bits, "nBitsExt": nbe, "nQueries": 8, "verificationHashType": "GL", "steps": [{"nBits": nbe}, {"nBits": 2}]}
    if air[0] == "fib":
        info, exprs, _ = stark.fibonacci_air(air[1], ss)
        cm, consts, publics = stark.fibonacci_trace(n_bits, air[1])
    else:
        info, exprs, _ = stark.permutation_air(ss, copies=air[1])
        cm, consts, publics = stark.permutation_trace(n_bits, copies=air[1])
    if corrupt is not None:
        cm = cm.copy(); cm[corrupt] = (int(cm[corrupt]) + 1) % P
    box = {}

    class Capture(stark_ref.OracleBackend):
        def compute_evals(self, descs, nb, eb, levs):
            evals = stark_ref.OracleBackend.compute_evals(self, descs, nb, eb, levs)
            if bend_eval is not None:
                evals[bend_eval][0] = (evals[bend_eval][0] + 1) % P
            return evals

        def fri_transpose(self, pol, pol_bits, t_bits):        # step 0 of the commit phase: pol is f_ext
            box["f"] = np.array(pol, dtype=np.uint64).reshape(-1, 3).copy()
            raise _Captured()

    be = Capture()
    assert not hasattr(be, "fri_polynomial") and not hasattr(be, "evals_fast")
    setup = stark.build_const_tree(be, consts, info)
    with pytest.raises(_Captured):
        stark.stark_gen(be, be.from_host(cm), setup, info, exprs, publics)
    assert box["f"].shape == (1 << nbe, 3)
    _cache[key] = box["f"]
    return box["f"]


def _from_the_sub_coset(oracle, f_ext, n_bits, ext_bits):
    """inverse transform of the rows k * 2^eb, zero-padded, transformed to 2^nBitsExt rows"""
    nbe = n_bits + ext_bits
    coef = oracle.ifft_cols(np.ascontiguousarray(f_ext[::1 << ext_bits]), n_bits)
    padded = np.zeros((1 << nbe, 3), np.uint64)
    padded[:1 << n_bits] = coef
    return oracle.fft_cols(padded, nbe)


@pytest.mark.parametrize("ext_bits", [1, 2, 3])
@pytest.mark.parametrize("n_bits", [5, 8])
@pytest.mark.parametrize("air", [("fib", 1), ("fib", 3), ("perm", 1)])
def test_extension_of_the_sub_coset_values_equals_f_ext(oracle, air, n_bits, ext_bits):
    f_ext = _oracle_f_ext(oracle, air, n_bits, ext_bits)
    again = _from_the_sub_coset(oracle, f_ext, n_bits, ext_bits)
    assert f_ext.any() and f_ext.max() < P
    assert np.array_equal(again, f_ext)
    # and the statement itself: no coefficient of F(7x) at or above N
    assert not oracle.ifft_cols(f_ext, n_bits + ext_bits)[1 << n_bits:].any()


@pytest.mark.parametrize("ext_bits", [1, 3])
@pytest.mark.parametrize("air,cell", [(("fib", 1), (5, 0)), (("fib", 3), (9, 4)), (("perm", 1), (7, 1))])
def test_the_identity_does_not_need_a_satisfied_air(oracle, air, cell, ext_bits):
    """one witness cell off by one (the quotient's sub-coset identity fails for these very witnesses, test_q_subcoset_cpu.py): the
    evaluations are still those of the committed columns, so F is still a polynomial of degree < N"""
    f_ext = _oracle_f_ext(oracle, air, 5, ext_bits, corrupt=cell)
    assert not np.array_equal(f_ext, _oracle_f_ext(oracle, air, 5, ext_bits))
    assert np.array_equal(_from_the_sub_coset(oracle, f_ext, 5, ext_bits), f_ext)


@pytest.mark.parametrize("air", [("fib", 1), ("perm", 1)])
def test_an_altered_evaluation_gives_two_different_polynomials(oracle, air):
    """the precondition: K must hold the true evaluations.  With one of them moved by one a bracket no longer vanishes at its xi, F has a
    pole there, and the values on the sub-coset no longer determine the others."""
    f_ext = _oracle_f_ext(oracle, air, 5, 2, bend_eval=0)
    assert oracle.ifft_cols(f_ext, 7)[1 << 5:].any()
    assert not np.array_equal(_from_the_sub_coset(oracle, f_ext, 5, 2), f_ext)
