"""The argument pil2gl_compute_q_stark_dev rests on, stated with the oracle alone (no GPU).

For a satisfied AIR deg Q < qDeg * N <= M = 2^m, m = nBits + ceil(log2 qDeg).  The extended rows k * 2^s, s = nBitsExt - m, are the
coset 7 <w_M>, so the size-M inverse transform of Q's values there gives c_j 7^j for j < M: the same words as the first M rows of the
size-2^nBitsExt inverse transform of Q's values on the whole extended domain.  computeQStark keeps only rows below qDeg * N.

The oracle's full-domain q_ext is taken from a proof on OracleBackend (it has no q_stark method and evaluates every extended row): the
backend below stops the proof at the quotient's inverse transform and hands over its input."""
import numpy as np
import pytest

from conftest import P


class _Captured(Exception):
    pass


def _oracle_q_ext(oracle, air, n_bits, ext_bits, corrupt=None):
    """(q_ext as a 2^nBitsExt x qDim matrix, info) of the oracle's proof of `air` at these sizes"""
    import stark_ref
    from pil2gl import stark
    nbe = n_bits + ext_bits
    ss = {"nBits": n_bits, "nBitsExt": nbe, "nQueries": 8, "verificationHashType": "GL", "steps": [{"nBits": nbe}]}
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
        def ifft(self, src, C, nb, dst):
            box["q"] = src.reshape(-1, C).copy()
            raise _Captured()

    be = Capture()
    setup = stark.build_const_tree(be, consts, info)
    with pytest.raises(_Captured):
        stark.stark_gen(be, be.from_host(cm), setup, info, exprs, publics)
    assert box["q"].shape == (1 << nbe, info["qDim"])
    return box["q"], info


def _both_ways(oracle, q_ext, info, n_bits, ext_bits):
    """(first qDeg * N coefficient rows of the full-domain inverse transform, the same rows from the rows k * 2^s alone, the full one's rest)"""
    nbe, qDeg = n_bits + ext_bits, info["qDeg"]
    m = n_bits + (qDeg - 1).bit_length()
    s = nbe - m
    assert s >= 0
    keep = qDeg << n_bits
    full = oracle.ifft_cols(q_ext, nbe)
    sub = oracle.ifft_cols(np.ascontiguousarray(q_ext[::1 << s]), m)
    return full[:keep], sub[:keep], full[keep:]


@pytest.mark.parametrize("ext_bits", [1, 2, 3, 4])
@pytest.mark.parametrize("n_bits", [5, 8])
@pytest.mark.parametrize("air", [("fib", 1), ("fib", 3), ("perm", 1)])
def test_sub_coset_inverse_transform_equals_the_full_one_on_the_kept_rows(oracle, air, n_bits, ext_bits):
    q_ext, info = _oracle_q_ext(oracle, air, n_bits, ext_bits)
    full, sub, rest = _both_ways(oracle, q_ext, info, n_bits, ext_bits)
    assert not rest.any()                       # deg Q < qDeg * N: what computeQStark drops is zero
    assert full.any() and np.array_equal(full, sub)


@pytest.mark.parametrize("n_bits_ext", range(2, 33))
def test_root_of_unity_convention(oracle, n_bits_ext):
    """root_of_unity(nBitsExt)^(2^s) == root_of_unity(nBitsExt - s): the rows k * 2^s of the extended domain are the coset 7 <w_M>"""
    from pil2gl import stark
    for s in range(1, min(n_bits_ext, 6) + 1):
        assert pow(stark.root_of_unity(n_bits_ext), 1 << s, P) == stark.root_of_unity(n_bits_ext - s)
        assert pow(int(oracle.root(n_bits_ext)), 1 << s, P) == int(oracle.root(n_bits_ext - s))
    assert int(oracle.root(n_bits_ext)) == stark.root_of_unity(n_bits_ext)


@pytest.mark.parametrize("air,cell", [(("fib", 1), (5, 0)), (("perm", 1), (7, 1))])
def test_a_broken_witness_gives_two_different_coefficient_matrices(oracle, air, cell):
    """one witness cell off by one: Q is no longer a polynomial of degree < qDeg * N, the full-domain transform drops its high
    coefficients and the sub-coset transform folds them onto the low ones.  Proof identity is claimed for satisfied AIRs only."""
    q_ext, info = _oracle_q_ext(oracle, air, 5, 3, corrupt=cell)
    full, sub, rest = _both_ways(oracle, q_ext, info, 5, 3)
    assert rest.any()
    assert not np.array_equal(full, sub)
