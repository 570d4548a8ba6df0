"""The host-pointer forms that go through the staging helper (csrc/common.h Stage), against the oracles, on both sides of its threshold:
up to 2^21 words a call is staged in the persistent slot, above it in a buffer allocated for the call.  Small shapes are a few dozen
words; the large ones pass 2^21 words in total by a few per cent.  (pil2gl_bn128_linear_hash_rows has its small shapes in
test_gpu_bn128.py::test_linear_hash_rows; a large one would cost the oracle 44 000 width-17 permutations, and the allocate-per-call branch
is the helper's own, taken by the three forms here.)"""
import numpy as np
import pytest

from conftest import rand_field

pytestmark = pytest.mark.gpu

STAGE_WORDS = 2 << 20


@pytest.fixture(scope="module")
def gl():
    import pil2gl
    pil2gl.init(0)
    return pil2gl


@pytest.mark.parametrize("pol_bits,t_bits", [(3, 1), (20, 7)])          # 48 words; 6 * 2^20
def test_fri_transpose_host(gl, oracle, pol_bits, t_bits):
    assert (6 << pol_bits > STAGE_WORDS) == (pol_bits == 20)
    pol = rand_field(np.random.default_rng(pol_bits), (1 << pol_bits, 3))
    out = np.zeros_like(pol)
    gl.call("pil2gl_fri_transpose", gl._ptr(pol), pol_bits, t_bits, gl._ptr(out))
    assert (out == oracle.fri_transpose(pol, t_bits)).all()


@pytest.mark.parametrize("fold_bits,nq", [(2, 3), (10, 700)])           # 48 words; (3 * 2^10 + 4) * 700
def test_fri_verify_fold_host(gl, oracle, fold_bits, nq):
    assert (((3 << fold_bits) + 4) * nq > STAGE_WORDS) == (nq == 700)
    rng = np.random.default_rng(fold_bits)
    G = rand_field(rng, (nq, 1 << fold_bits, 3)); sinv = rand_field(rng, nq); ch = rand_field(rng, 3)
    Gt = np.ascontiguousarray(G.transpose(1, 0, 2))
    out = np.zeros((nq, 3), np.uint64)
    gl.call("pil2gl_fri_verify_fold", gl._ptr(Gt), fold_bits, nq, gl._ptr(sinv), gl._ptr(ch), gl._ptr(out))
    want = np.array([oracle.fri_fold(G[q], 0, int(sinv[q]), ch)[0] for q in range(nq)])
    assert (out == want).all()


@pytest.mark.parametrize("n_ops", [5, 175001])                          # 60 words; 12 * 175001
def test_merkelize_level_host(gl, oracle, n_ops):
    """a row of up to four words is its own leaf digest (merklehash_p.js: linearHash returns short rows as they are), so the first level the
    oracle builds over 2 n_ops rows of four words is merkelizeLevel of those words"""
    assert (12 * n_ops > STAGE_WORDS) == (n_ops > 5)
    a = rand_field(np.random.default_rng(n_ops), (2 * n_ops, 4))
    out = np.zeros(n_ops * 4, np.uint64)
    gl.call("pil2gl_merkelize_level", gl._ptr(a), n_ops, gl._ptr(out))
    nodes = oracle.merkelize(a, False)
    assert (nodes[:8 * n_ops] == a.reshape(-1)).all()
    assert (out == nodes[8 * n_ops:12 * n_ops]).all()
