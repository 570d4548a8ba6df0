"""Chosen outputs: inputs built so that the device's RESULT is small, zero or a magnitude edge.

csrc/gl_field.cuh's invariant is that kernels may carry lazy values (any representative in [0, 2^64)) while everything stored to
memory is canonical, [0, p).  A value has a second 64-bit representative only when it is below 2^32 - 1, which a uniformly random
result is with probability 2^-32: a store that forgets its canon() is invisible to every test that feeds random data and compares
with the oracle.  Here the expected output is chosen first (every word below 2^32 - 1, a fifth of them zero) and the input is the
oracle's inverse image of it, so a lazy product that reaches memory shows as a word >= p.

The transforms keep their tiles lazy through every stage and canonicalise at separate store sites (ntt_pass_kernel's three forms,
lde_mid_kernel's, the fixed-geometry instances of both, fft_block_stage_kernel); the parametrisation walks all of them: single-kernel,
two- and three-pass sizes, the fixed-geometry kernels and their any-geometry twins, every pass split the planner can take, the
wide-forward-pass switch, extBits = 0, columns 1 / 3 / 15 / 16 / 17 / 100, every coset-slice and coefficient-input entry point.
Inputs that cancel to exact zeros inside the tiles or sit at the magnitude edges are compared with the oracle on all rows.

Poseidon: the permutation is inverted in Python integers, so the chosen twelve-word final state is reached through
pil2gl_selftest_poseidon (all three statements) and pil2gl_poseidon with a capacity.  The leaf, split-leaf and tree-level kernels
start their first block from capacity zero: a preimage of a chosen digest has a non-zero capacity in general, so no chosen digest
can be reached through them and they are NOT covered here.

Degenerate opening points: xi on the evaluation coset (x / (x - xi) divides by zero: refused, as the reference throws) and xi a
root of unity of the trace domain (LEv is a unit vector: the closed form is 0 / 0 there)."""
import os
import re

import numpy as np
import pytest

from conftest import P, ROOT, rand_field

pytestmark = pytest.mark.gpu

SMALL = (1 << 32) - 1               # values below it have a second representative v + p < 2^64
EDGES = [P - 1, P - 2, (1 << 32) - 1, 1 << 32, 1 << 63, 0xFFFFFFFF00000000]
_P = np.uint64(P)
_M32 = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


@pytest.fixture(scope="module")
def gl():
    import pil2gl
    pil2gl.init(0)
    return pil2gl


# ------------------------------------------------------------------ helpers
def _targets(n, C, seed):
    """(n, C) words, all below 2^32 - 1: about a fifth exactly 0, and 1, 2^32 - 2, 2^31 sprinkled in"""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, SMALL, size=(n, C), dtype=np.uint64)
    r = rng.random(size=(n, C))
    a[r < 0.2] = 0
    for k, v in enumerate((1, SMALL - 1, 1 << 31)):
        a[(r >= 0.2 + 0.02 * k) & (r < 0.22 + 0.02 * k)] = v
    return a


def _edge_matrix(n, C, seed):
    """(n, C) words drawn from the magnitude edges only"""
    rng = np.random.default_rng(seed)
    return np.array(EDGES, dtype=np.uint64)[rng.integers(0, len(EDGES), size=(n, C))]


def _addmod(a, b):
    s = a + b
    return np.where((s < a) | (s >= _P), s - _P, s)


def _submod(a, b):
    d = a - b
    return np.where(a < b, d + _P, d)


def _mulmod(a, b):
    """canonical * canonical -> canonical on uint64 arrays (host helper of the constructions; every construction is checked against the
    oracle before the device sees it)"""
    a, b = np.broadcast_arrays(np.asarray(a, dtype=np.uint64), np.asarray(b, dtype=np.uint64))
    a0, a1, b0, b1 = a & _M32, a >> _S32, b & _M32, b >> _S32
    t = a0 * b0
    u = a0 * b1 + (t >> _S32)
    v = a1 * b0 + (u & _M32)
    hi = a1 * b1 + (u >> _S32) + (v >> _S32)
    lo = (v << _S32) | (t & _M32)
    r = np.where(lo >= _P, lo - _P, lo)
    r = _submod(r, hi >> _S32)                      # 2^96 = -1
    return _addmod(r, (hi & _M32) * _M32)           # 2^64 = 2^32 - 1; (2^32 - 1)^2 < p


def _powers(g, n):
    """g^k for k < n (n a power of two)"""
    pw = np.array([1], dtype=np.uint64)
    while pw.size < n:
        pw = np.concatenate([pw, _mulmod(pw, np.uint64(pow(g, pw.size, P)))])
    return pw


def _brev(nb):
    i = np.arange(1 << nb, dtype=np.uint64)
    r = np.zeros_like(i)
    for b in range(nb):
        r |= ((i >> np.uint64(b)) & np.uint64(1)) << np.uint64(nb - 1 - b)
    return r.astype(np.int64)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64).reshape(-1)).cuda()


def _host(t, shape):
    return t.cpu().numpy().view(np.uint64).reshape(shape)


def _enough_small(expected, count):
    """the condition that keeps a chosen-output test from passing vacuously, on the EXPECTED array alone"""
    assert int((expected < np.uint64(SMALL)).sum()) >= count


def _same(got, want, what):
    assert (got < _P).all(), ("stored word >= p", what, int((got >= _P).sum()))
    assert np.array_equal(got, want), what


def test_host_helpers(oracle):
    """the numpy products the constructions use, against Python integers on edge and random operands"""
    rng = np.random.default_rng(1)
    a = np.concatenate([np.array(EDGES + [0, 1, SMALL - 1, 1 << 31], dtype=np.uint64) % _P, rand_field(rng, 4000)])
    b = np.concatenate([rand_field(rng, 4000), np.array(EDGES + [0, 1, SMALL - 1, 1 << 31], dtype=np.uint64) % _P])
    assert [int(v) for v in _mulmod(a, b)] == [int(x) * int(y) % P for x, y in zip(a, b)]
    assert [int(v) for v in _mulmod(a, a)] == [int(x) * int(x) % P for x in a]
    assert [int(v) for v in _powers(12345, 64)] == [pow(12345, k, P) for k in range(64)]
    t = _targets(1 << 12, 7, 3)
    assert (t < np.uint64(SMALL)).all() and 0.15 < (t == 0).mean() < 0.25
    for v in (1, SMALL - 1, 1 << 31):
        assert (t == v).any()
    assert np.array_equal(t, _targets(1 << 12, 7, 3))
    assert set(int(v) for v in _edge_matrix(64, 8, 0).reshape(-1)) == set(EDGES)


# ------------------------------------------------------------------ fft / ifft with chosen outputs
# (nBits, columns, switches): single-pass sizes (n <= 8, or 7 for rows under 128 bytes), two passes, three passes (2^21 x 1); the
# fixed-geometry shapes of test_ntt_fixed_geometry_kernels with both kernel families; PIL2GL_NTT_KMAX as
# test_ntt_random_shapes_and_pass_splits forces it
_NTT_CASES = [(1, 3, {}), (4, 100, {}), (7, 1, {}), (7, 15, {}), (8, 16, {}), (8, 17, {}),
              (9, 1, {}), (10, 15, {}), (12, 3, {}), (13, 17, {}), (14, 100, {}), (16, 16, {}),
              (21, 1, {})]
_GENERIC = {"GENERIC": [{"PIL2GL_NTT_GENERIC": g} for g in ("0", "1")]}
_KMAX = {"KMAX": [{}] + [{"PIL2GL_NTT_KMAX": k} for k in ("4", "6", "9", "10")]}
_WIDEFWD = {"WIDEFWD": [{"PIL2GL_LDE_WIDEFWD": w} for w in ("1", "0")]}
_NTT_CASES += [(nb, C, _GENERIC) for nb, C in ((16, 30), (16, 32), (17, 100))]
# (9, 3): PIL2GL_NTT_KMAX=9 reaches a 9-stage tile exactly; (8, 15) and (16, 15): with 9 or 10 a 15-column matrix takes 8-stage passes, the
# only way to the 15-slot fixed-geometry pass instances (rows of 15 columns are under 128 bytes: 7-stage passes by default)
_NTT_CASES += [(nb, C, _KMAX) for nb, C in ((10, 3), (12, 17), (13, 100), (9, 3), (8, 15), (16, 15))]


def _case_id(c):
    return "-".join(str(x) for x in c[:-1]) + "".join("-" + k for k in c[-1])


def _envs(monkeypatch, switch, ops=(), shape=()):
    """the settings a case runs under, one after the other on the same host-side construction: {} = the defaults, else the values of
    one switch.  What the switch is there to reach -- a kernel family, a pass size -- is asserted on the host-only plan of `ops` at
    `shape` (transform_plan.check_hooks) before the case runs under it."""
    import transform_plan as tp
    for env in (next(iter(switch.values())) if switch else [{}]):
        for k in ("PIL2GL_NTT_KMAX", "PIL2GL_NTT_GENERIC", "PIL2GL_LDE_WIDEFWD"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        tp.check_hooks(env, ops, *shape)
        yield tuple(env.items())


def test_the_kmax_cases_reach_every_forced_pass_size(monkeypatch):
    """the planner balances its passes, so PIL2GL_NTT_KMAX=K yields a K-stage tile only where K divides the index bits (or covers them): for
    each K the cases force, some fft case and some interpolate case plans exactly K stages; and the 15-column cases reach the 15-slot
    fixed-geometry pass kernels, forward DIF, inverse DIF and DIT"""
    import transform_plan as tp
    monkeypatch.delenv("PIL2GL_NTT_GENERIC", raising=False)
    inst = set()
    for env in _KMAX["KMAX"][1:]:
        K = int(env["PIL2GL_NTT_KMAX"])
        monkeypatch.setenv("PIL2GL_NTT_KMAX", str(K))
        assert any(max(l.k for l in tp.plan("fft", nb, C)) == K for nb, C, e in _NTT_CASES if e is _KMAX), K
        assert any(max(l.k for l in tp.plan("interpolate", nb, C, eb)) == K for nb, C, eb, e in _LDE_CASES if e is _KMAX), K
        for op, shape in [(op, (nb, C)) for nb, C, e in _NTT_CASES if e is _KMAX for op in ("fft", "ifft")] + \
                         [("interpolate", (nb, C, eb)) for nb, C, eb, e in _LDE_CASES if e is _KMAX]:
            inst |= {l.kind for l in tp.plan(op, *shape) if l.fixed == 15 and l.kind != "m"}
    assert inst == {"f", "i", "d"}


@pytest.mark.parametrize("nBits,C,env", _NTT_CASES, ids=[_case_id(c) for c in _NTT_CASES])
def test_fft_ifft_chosen_outputs(gl, oracle, monkeypatch, nBits, C, env):
    """fft of oracle.ifft(Y) and ifft of oracle.fft(Y) must be Y word for word, out of place (host buffers) and in place (device)"""
    n = 1 << nBits
    Y = _targets(n, C, nBits * 1000 + C)
    _enough_small(Y, n * C)
    for name, fn, inverse_image in (("fft", gl.fft, oracle.ifft_cols), ("ifft", gl.ifft, oracle.fft_cols)):
        src = inverse_image(Y, nBits)
        assert (src < _P).all()                     # every kernel relies on canonical inputs
        for e in _envs(monkeypatch, env, (name,), (nBits, C)):
            out = np.full_like(Y, 0xDEADBEEF)
            fn(src, C, nBits, out)
            _same(out, Y, (name, "out of place", e))
            d = _dev(src)
            fn(d, C, nBits, d)
            _same(_host(d, Y.shape), Y, (name, "in place", e))


# ------------------------------------------------------------------ extensions with a chosen coset
def _chosen_coset(oracle, nb, C, eb, j, shift, seed):
    """values V chosen on coset j of the extension: the polynomial with p(g w_N^pos) = V[pos], g = shift * w_E^j, has the coefficients
    ifft(V)_k g^-k.  -> (V, c = those coefficients, trace = their values on the trace domain)"""
    n = 1 << nb
    V = _targets(n, C, seed)
    g = shift * pow(int(oracle.root(nb + eb)), j, P) % P
    c = np.ascontiguousarray(_mulmod(oracle.ifft_cols(V, nb), _powers(pow(g, P - 2, P), n)[:, None]))
    trace = oracle.fft_cols(c, nb)
    assert (c < _P).all() and (trace < _P).all()
    return V, c, trace


def _cosets_of(eb):
    last = (1 << eb) - 1
    return sorted({0, last // 2 + (1 if last > 1 else 0), last} if eb else {0})


# (nBits, columns, extBits, switches): single-kernel sizes (lde_mid_kernel stores the result itself), two passes, three passes,
# extBits = 0, the fixed-geometry mid / pass kernels and their any-geometry twins, every pass split, wide forward passes on and off
_LDE_CASES = [(1, 1, 1, {}), (3, 3, 2, {}), (7, 1, 3, {}), (7, 15, 3, {}), (8, 16, 1, {}), (8, 100, 2, {}), (7, 33, 0, {}), (8, 17, 0, {}),
              (10, 3, 3, {}), (12, 17, 2, {}), (13, 16, 0, {}), (14, 100, 1, {}), (14, 15, 3, {}),
              (21, 1, 1, {})]
_LDE_CASES += [(nb, C, eb, _GENERIC) for nb, C, eb in ((16, 30, 3), (16, 32, 1), (17, 100, 1))]
_LDE_CASES += [(nb, C, eb, _KMAX) for nb, C, eb in ((10, 3, 1), (12, 17, 2), (13, 100, 1), (9, 3, 1), (16, 15, 0))]
_LDE_CASES += [(nb, C, eb, _WIDEFWD) for nb, C, eb in ((15, 2, 3), (16, 8, 2), (16, 1, 3))]


@pytest.mark.parametrize("nb,C,eb,env", _LDE_CASES, ids=[_case_id(c) for c in _LDE_CASES])
def test_interpolate_chosen_coset(gl, oracle, monkeypatch, nb, C, eb, env):
    """interpolate and its coset-slice forms: rows (pos << eb) + j of the extension are the chosen V, for j = 0, a middle coset and the
    last one; the whole extension is the oracle's"""
    import torch
    n, E, nc = 1 << nb, 1 << (nb + eb), 1 << eb
    for j in _cosets_of(eb):
        V, _, trace = _chosen_coset(oracle, nb, C, eb, j, 7, nb * 1000 + C * 10 + j)
        whole = oracle.interpolate(trace, nb, nb + eb)
        assert np.array_equal(whole.reshape(n, nc, C)[:, j], V)
        _enough_small(whole, n * C)
        slices = {(j, 1), (0, nc)}
        if nc >= 2:
            slices |= {((j & ~1), 2), ((j + 1) % nc, 1)}                            # a slice that holds j beside another coset, one that does not
        for e in _envs(monkeypatch, env, ("interpolate",), (nb, C, eb)):
            out = np.full((E, C), 0xDEADBEEF, np.uint64)
            gl.interpolate(trace, C, nb, out, nb + eb)
            assert np.array_equal(out.reshape(n, nc, C)[:, j], V), ("interpolate", j, e)
            _same(out, whole, ("interpolate", j, e))
            if nb == 21:
                continue                            # (the slice forms run the same kernels: kept to the sizes where the host work is small)
            src = _dev(trace)
            for cb, cc in sorted(slices):
                want = np.ascontiguousarray(whole.reshape(n, nc, C)[:, cb:cb + cc]).reshape(-1)
                dst = torch.full(((C * cc) << nb,), 0xDEADBEEF, dtype=torch.int64, device="cuda")
                gl.interpolateCosets(src, C, nb, dst, nb + eb, cb, cc)
                _same(_host(dst, want.shape), want, ("interpolateCosets", j, cb, cc, e))
            # the trace itself as workspace (overwritten): last
            dst = torch.full((C << nb,), 0xDEADBEEF, dtype=torch.int64, device="cuda")
            gl.interpolateCosets(src, C, nb, dst, nb + eb, j, 1, workspace=src)
            _same(_host(dst, V.shape), V, ("interpolate_cosets_ws, workspace == src", j, e))


_COEF_CASES = [(1, 3, 1, {}), (6, 6, 2, {}), (8, 16, 3, {}), (8, 6, 0, {}), (10, 6, 3, {}), (12, 17, 2, {}), (14, 100, 1, {}), (16, 6, 3, {}),
               (16, 32, 1, _GENERIC), (17, 100, 1, _GENERIC), (20, 6, 1, {}), (12, 6, 2, _KMAX)]


@pytest.mark.parametrize("nb,C,eb,env", _COEF_CASES, ids=[_case_id(c) for c in _COEF_CASES])
def test_unshifted_and_coefficient_extensions_chosen_coset(gl, oracle, monkeypatch, nb, C, eb, env):
    """the plain extension (no coset shift: evaluation points w_E^j <w_N>) from a trace (pil2gl_extend_cosets_unshifted_dev) and from
    coefficients in bit-reversed row order (pil2gl_extend_coefs_brev_dev, _cosets_dev), against fft of the zero-padded coefficients;
    rows (pos << eb) + j are the chosen V"""
    import torch
    from pil2gl import _lib
    n, E, nc = 1 << nb, 1 << (nb + eb), 1 << eb
    br = _brev(nb)
    for j in _cosets_of(eb):
        V, c, trace = _chosen_coset(oracle, nb, C, eb, j, 1, nb * 999 + C * 10 + j)
        padded = np.zeros((E, C), np.uint64); padded[:n] = c
        whole = oracle.fft_cols(padded, nb + eb)
        assert np.array_equal(whole.reshape(n, nc, C)[:, j], V)
        _enough_small(whole, n * C)
        slices = {(j, 1), (0, nc)}
        if nc >= 2:
            slices |= {((j & ~1), 2), ((j + 1) % nc, 1)}
        for e in _envs(monkeypatch, env, ("interpolate", "extend_coefs"), (nb, C, eb)):
            cb_ = _dev(c[br])                       # row bitrev(m) = coefficient m
            out = torch.full((C << (nb + eb),), 0xDEADBEEF, dtype=torch.int64, device="cuda")
            _lib.call("pil2gl_extend_coefs_brev_dev", gl._ptr(cb_), C, nb, gl._ptr(out), nb + eb, None)
            _same(_host(out, whole.shape), whole, ("extend_coefs_brev", j, e))
            src = _dev(trace)
            for cb, cc in sorted(slices):
                want = np.ascontiguousarray(whole.reshape(n, nc, C)[:, cb:cb + cc]).reshape(-1)
                for entry, buf in (("pil2gl_extend_cosets_unshifted_dev", src), ("pil2gl_extend_coefs_brev_cosets_dev", cb_)):
                    dst = torch.full(((C * cc) << nb,), 0xDEADBEEF, dtype=torch.int64, device="cuda")
                    _lib.call(entry, gl._ptr(buf), C, nb, gl._ptr(dst), nb + eb, cb, cc, None)
                    _same(_host(dst, want.shape), want, (entry, j, cb, cc, e))


# ------------------------------------------------------------------ the worker-level operators
def _fft_block_inverse(buff, rel_pos, start_pos, nPols, nBits, s, blockBits, layers):
    """undoes oracle/fft_worker_ref.py:_fft_block (fft_worker.js:21-60): the butterflies of the last stage first, a = (a' + b') / 2,
    b = (a' - b') / (2 w), then the two half blocks"""
    import fft_worker_ref as R
    m = 1 << blockBits
    md2 = m >> 1
    if layers < blockBits:
        _fft_block_inverse(buff, rel_pos, start_pos, nPols, nBits, s, blockBits - 1, layers)
        _fft_block_inverse(buff, rel_pos, start_pos + md2, nPols, nBits, s, blockBits - 1, layers)
        return
    if s > blockBits:
        width = 1 << (s - layers)
        heigth = (1 << nBits) // width
        w = pow(R.root(s), (start_pos % heigth) * width + start_pos // heigth, P)
    else:
        w = 1
    wl, half = R.root(layers), pow(2, P - 2, P)
    for i in range(md2):
        wi = pow(w, P - 2, P)
        for j in range(nPols):
            a, b = (start_pos - rel_pos + i) * nPols + j, (start_pos - rel_pos + md2 + i) * nPols + j
            x, y = buff[a], buff[b]
            buff[a] = (x + y) * half % P
            buff[b] = (x - y) * half % P * wi % P
        w = w * wl % P
    if layers > 1:
        _fft_block_inverse(buff, rel_pos, start_pos, nPols, nBits, s - 1, blockBits - 1, layers - 1)
        _fft_block_inverse(buff, rel_pos, start_pos + md2, nPols, nBits, s - 1, blockBits - 1, layers - 1)


@pytest.mark.parametrize("nBits,s,blockBits,nPols,start_pos", [(6, 6, 6, 3, 0), (3, 3, 3, 1, 0), (14, 12, 8, 5, 3 << 8), (32, 32, 6, 2, 5 << 6), (10, 4, 4, 17, 16)])
def test_fft_block_chosen_outputs(gl, nBits, s, blockBits, nPols, start_pos):
    """one block with layers = blockBits whose outputs are the target (w0 = 1 and w0 != 1 alike); then the same block with some input
    words handed over as their second representative v + p, which F.add / F.mul of the reference reduce: the stage kernel must too"""
    import fft_worker_ref as R
    Y = _targets(1 << blockBits, nPols, nBits * 100 + s)
    _enough_small(Y, Y.size)
    pre = [int(v) for v in Y.reshape(-1)]
    _fft_block_inverse(pre, start_pos, start_pos, nPols, nBits, s, blockBits, blockBits)
    assert all(0 <= v < P for v in pre)
    assert R.fft_block(list(pre), start_pos, nPols, nBits, s, blockBits, blockBits) == [int(v) for v in Y.reshape(-1)]
    buf = np.array(pre, dtype=np.uint64)
    gl.fft_block(buf, start_pos, nPols, nBits, s, blockBits, blockBits)
    _same(buf.reshape(Y.shape), Y, "canonical input")
    rng = np.random.default_rng(s)
    # inputs that are themselves small, lifted to v + p: one stage, so that the lifted words are the block's inputs
    X = _targets(1 << blockBits, nPols, 77 + s)
    want = R.fft_block([int(v) for v in X.reshape(-1)], start_pos, nPols, nBits, s, blockBits, 1)
    lifted = X.copy()
    lift = rng.random(size=X.shape) < 0.5
    lifted[lift] += _P
    assert (lifted[lift] >= _P).all() and lift.sum() > 0
    got = lifted.reshape(-1).copy()
    gl.fft_block(got, start_pos, nPols, nBits, s, blockBits, 1)
    _same(got, np.array(want, dtype=np.uint64), "inputs lifted by p")


def test_interpolate_prepare_block_chosen_outputs(gl):
    """row_i = target_i / (start * inc^i): the products must be the target"""
    rng = np.random.default_rng(9)
    for width, height in ((1, 1), (3, 64), (100, 256), (8, 4096)):
        Y = _targets(height, width, width + height)
        _enough_small(Y, Y.size)
        start, inc = int(rand_field(rng, 1)[0]) or 1, int(rand_field(rng, 1)[0]) or 1
        f = np.array([pow(start * pow(inc, i, P) % P, P - 2, P) for i in range(height)], dtype=np.uint64)
        src = np.ascontiguousarray(_mulmod(Y, f[:, None]))
        assert (src < _P).all()
        got = src.reshape(-1).copy()
        gl.interpolatePrepareBlock(got, width, start, inc)
        _same(got.reshape(Y.shape), Y, (width, height))


# ------------------------------------------------------------------ cancellation and magnitude
def _structured(nb, seed, ks=None, bits=None):
    """columns that cancel to exact zeros inside the transform or sit at the magnitude edges (canonical: the edges taken mod p):
    constants; period 2^k for every k in ks (exact zeros from stage k on); one non-zero row; all p - 1; for every bit b in bits of
    the row index a two-valued column (A if bit b of the row else B) with (A, B) from the edges; columns drawn from the edges only"""
    n = 1 << nb
    rng = np.random.default_rng(seed)
    edges = [v % P for v in EDGES]
    r = np.arange(n, dtype=np.uint64)
    cols = [np.full(n, v, np.uint64) for v in (1, edges[0], edges[4])]
    for k in (range(nb + 1) if ks is None else ks):
        per = rand_field(rng, 1 << k) if k % 2 else np.array(edges, dtype=np.uint64)[rng.integers(0, len(edges), 1 << k)]
        cols.append(per[r & np.uint64((1 << k) - 1)])
    for row, v in ((0, 1), (n - 1, edges[0]), (n // 2, edges[3]), (int(rng.integers(0, n)), edges[5] % P)):
        c = np.zeros(n, np.uint64); c[row] = v; cols.append(c)
    cols.append(np.full(n, P - 1, np.uint64))
    for b in (range(nb) if bits is None else bits):
        A, B = (edges[int(x)] for x in rng.choice(len(edges), 2, replace=False))
        cols.append(np.where((r >> np.uint64(b)) & np.uint64(1), np.uint64(A), np.uint64(B)).astype(np.uint64))
    e = _edge_matrix(n, 3, seed + 1) % _P
    cols += [e[:, 0], e[:, 1], e[:, 2]]
    a = np.ascontiguousarray(np.stack(cols, axis=1))
    assert (a < _P).all()
    return a


_STRUCT_CASES = [(nb, eb, _KMAX) for nb, eb in ((3, 2), (8, 1), (10, 2), (12, 2), (13, 1))] + [(16, 1, _GENERIC), (7, 0, {}), (14, 0, {})]


@pytest.mark.parametrize("nb,eb,env", _STRUCT_CASES, ids=[_case_id(c) for c in _STRUCT_CASES])
def test_cancellation_and_magnitude_columns(gl, oracle, monkeypatch, nb, eb, env):
    """fft, ifft and interpolate of the structured columns against the oracle on all rows, in every pass split"""
    a = _structured(nb, nb * 7 + eb)
    C = a.shape[1]
    wf, wi, we = oracle.fft_cols(a, nb), oracle.ifft_cols(a, nb), oracle.interpolate(a, nb, nb + eb)
    for e in _envs(monkeypatch, env, ("fft", "ifft", "interpolate"), (nb, C, eb)):
        out = np.zeros_like(a)
        gl.fft(a, C, nb, out); _same(out, wf, ("fft", e))
        gl.ifft(a, C, nb, out); _same(out, wi, ("ifft", e))
        ext = np.zeros((1 << (nb + eb), C), np.uint64)
        gl.interpolate(a, C, nb, ext, nb + eb); _same(ext, we, ("interpolate", e))


def test_cancellation_and_magnitude_columns_three_passes(gl, oracle):
    """the same at 2^21 rows (three passes in every direction), with the periods and bits that fall in each of the three passes"""
    nb = 21
    a = _structured(nb, 21, ks=(0, 3, 7, 8, 14, 15, 21), bits=(0, 6, 7, 13, 14, 20))
    C = a.shape[1]
    out = np.zeros_like(a)
    gl.fft(a, C, nb, out); _same(out, oracle.fft_cols(a, nb), "fft")
    gl.ifft(a, C, nb, out); _same(out, oracle.ifft_cols(a, nb), "ifft")
    ext = np.zeros((1 << (nb + 1), C), np.uint64)
    gl.interpolate(a, C, nb, ext, nb + 1); _same(ext, oracle.interpolate(a, nb, nb + 1), "interpolate")


# ------------------------------------------------------------------ degenerate opening points
@pytest.mark.parametrize("nBits", [1, 4, 9, 13])
def test_lev_at_roots_of_unity_and_other_base_field_points(gl, oracle, nBits):
    """LEv = ifft of xi^k.  xi = (w_N^j, 0, 0): the unit vector at row j (the closed form the library otherwise uses is 0 / 0 there);
    base-field points that are no root of unity, and xi = 0 (xi^0 = 1: the constant 1 / N)"""
    import torch
    from pil2gl import _lib
    N = 1 << nBits
    w = int(oracle.root(nBits))
    lev = torch.zeros(3 * N, dtype=torch.int64, device="cuda")
    for j in sorted({0, 1, N // 2 + (1 if N > 4 else 0), N - 1}):
        xi = np.array([pow(w, j, P), 0, 0], dtype=np.uint64)
        want = oracle.lev(nBits, xi)
        unit = np.zeros((N, 3), np.uint64); unit[j, 0] = 1
        assert np.array_equal(want, unit)
        lev.fill_(0xDEADBEEF)
        _lib.call("pil2gl_build_lev_dev", nBits, gl._ptr(xi), gl._ptr(lev), None)
        _same(_host(lev, (N, 3)), want, ("root of unity", j))
    xi = np.array([1 + P, P, 0], dtype=np.uint64)                  # w^0 with words that are not reduced
    unit = np.zeros((N, 3), np.uint64); unit[0, 0] = 1
    lev.fill_(0xDEADBEEF)
    _lib.call("pil2gl_build_lev_dev", nBits, gl._ptr(xi), gl._ptr(lev), None)
    _same(_host(lev, (N, 3)), unit, "root of unity, unreduced words")
    for x0 in (0, 7, 2, P - 1 if nBits > 1 else 3, 7 * w % P, pow(int(oracle.root(nBits + 1)), 1, P), 0x123456789ABCDEF):
        if pow(x0, N, P) == 1:
            continue
        xi = np.array([x0, 0, 0], dtype=np.uint64)
        lev.fill_(0xDEADBEEF)
        _lib.call("pil2gl_build_lev_dev", nBits, gl._ptr(xi), gl._ptr(lev), None)
        _same(_host(lev, (N, 3)), oracle.lev(nBits, xi), ("base field", x0))


@pytest.mark.parametrize("nbe,eb", [(1, 0), (4, 1), (9, 3), (12, 3)])
def test_x_div_x_sub_xi_refuses_a_point_of_its_own_coset(gl, oracle, nbe, eb):
    """xi = (7 w_E^k, 0, 0): row k of x / (x - xi) divides by zero, the reference throws (F.batchInverse): PIL2GL_EINVAL and nothing
    written, from both forms and whichever cosets are asked for; a base-field xi outside the coset is the oracle's table"""
    import torch
    from pil2gl import _lib
    E = 1 << nbe
    wE = int(oracle.root(nbe))
    d = torch.full((E * 6,), 0x5EED, dtype=torch.int64, device="cuda")
    for k in sorted({0, 1, E // 2, E - 1}):
        for zero in (0, P):                         # (P: the same point, words not reduced)
            xi = np.array([7 * pow(wE, k, P) % P, zero, zero], dtype=np.uint64)
            with pytest.raises(gl.Pil2glError):
                _lib.call("pil2gl_x_div_x_sub_xi_dev", nbe, gl._ptr(xi), 2, 1, gl._ptr(d), None)
            for cb, cc in {(0, 1), ((1 << eb) - 1, 1), (0, 1 << eb)}:
                with pytest.raises(gl.Pil2glError):
                    _lib.call("pil2gl_x_div_x_sub_xi_cosets_dev", nbe, eb, gl._ptr(xi), 2, 0, cb, cc, gl._ptr(d), None)
    torch.cuda.synchronize()
    assert bool((d == 0x5EED).all())
    xis = np.array([[3, 0, 0], [7 * pow(int(oracle.root(nbe + 1)), 1, P) % P, 0, 0]], dtype=np.uint64)      # off the coset: 3 / 7 and w_2E have no order dividing E
    assert all(pow(int(x) * pow(7, P - 2, P) % P, E, P) != 1 for x in xis[:, 0])
    for i in range(2):
        _lib.call("pil2gl_x_div_x_sub_xi_dev", nbe, gl._ptr(np.ascontiguousarray(xis[i])), 2, i, gl._ptr(d), None)
    full = oracle.x_div_x_sub_xi(nbe, xis)
    _same(_host(d, (E, 6)), full, "base-field xi outside the coset")
    if eb:
        nb = nbe - eb
        cb, cc = (1 << eb) - 2, 2
        ds = torch.zeros((cc << nb) * 6, dtype=torch.int64, device="cuda")
        for i in range(2):
            _lib.call("pil2gl_x_div_x_sub_xi_cosets_dev", nbe, eb, gl._ptr(np.ascontiguousarray(xis[i])), 2, i, cb, cc, gl._ptr(ds), None)
        _same(_host(ds, (cc << nb, 6)), full.reshape(1 << nb, 1 << eb, 6)[:, cb:cb + cc].reshape(-1, 6), "coset slice")


# ------------------------------------------------------------------ Poseidon with chosen final states
_MC = [17, 15, 41, 16, 2, 28, 13, 13, 39, 18, 34, 20]
_MDS = [[_MC[(j - i) % 12] + (8 if i == 0 and j == 0 else 0) for j in range(12)] for i in range(12)]


def _round_constants():
    with open(os.path.join(ROOT, "oracle", "poseidon_gl_constants.h")) as f:
        rc = [int(x, 16) for x in re.findall(r"0x([0-9a-f]{16})ull", f.read())]
    assert len(rc) == 360
    return rc


def _mat_inverse(M):
    """Gaussian elimination mod p"""
    n = len(M)
    A = [[v % P for v in row] + [int(i == k) for k in range(n)] for i, row in enumerate(M)]
    for c in range(n):
        piv = next(r for r in range(c, n) if A[r][c])
        A[c], A[piv] = A[piv], A[c]
        iv = pow(A[c][c], P - 2, P)
        A[c] = [v * iv % P for v in A[c]]
        for r in range(n):
            if r != c and A[r][c]:
                f = A[r][c]
                A[r] = [(x - f * y) % P for x, y in zip(A[r], A[c])]
    return [row[n:] for row in A]


def _perm(st, rc):
    """glwasm.js:216-426, the 30-round form: constants, x^7 (all lanes in rounds 0-3 and 26-29, lane 0 otherwise), MDS"""
    st = [v % P for v in st]
    for r in range(30):
        st = [(v + rc[12 * r + i]) % P for i, v in enumerate(st)]
        if r < 4 or r >= 26:
            st = [pow(v, 7, P) for v in st]
        else:
            st[0] = pow(st[0], 7, P)
        st = [sum(_MDS[i][j] * st[j] for j in range(12)) % P for i in range(12)]
    return st


def _perm_inverse(st, rc, Minv, d):
    for r in reversed(range(30)):
        st = [sum(Minv[i][j] * st[j] for j in range(12)) % P for i in range(12)]
        if r < 4 or r >= 26:
            st = [pow(v, d, P) for v in st]
        else:
            st[0] = pow(st[0], d, P)
        st = [(v - rc[12 * r + i]) % P for i, v in enumerate(st)]
    return st


def test_poseidon_chosen_final_states(gl, oracle):
    """preimages, computed in Python integers, of final states whose twelve words are all below 2^32 - 1 (some exactly 0): the three
    statements of the permutation and pil2gl_poseidon with the capacity given must return the chosen state, canonical"""
    from pil2gl import _lib
    rc = _round_constants()
    Minv = _mat_inverse(_MDS)
    assert all(sum(_MDS[i][k] * Minv[k][j] for k in range(12)) % P == int(i == j) for i in range(12) for j in range(12))
    d = pow(7, -1, P - 1)
    rng = np.random.default_rng(12)
    for s in rand_field(rng, (20, 12)):             # the forward restatement against the oracle, and the inverse against it
        s = [int(v) for v in s]
        f = _perm(s, rc)
        assert f == [int(v) for v in oracle.poseidon(s[:8], s[8:], 12)]
        assert _perm_inverse(f, rc, Minv, d) == s
    Y = _targets(300, 12, 5)
    Y[0] = 0; Y[1] = SMALL - 1; Y[2] = 1
    _enough_small(Y, Y.size)
    pre = np.array([_perm_inverse([int(v) for v in y], rc, Minv, d) for y in Y], dtype=np.uint64)
    assert (pre < _P).all()
    assert _perm([int(v) for v in pre[7]], rc) == [int(v) for v in Y[7]]
    for what in (0, 1, 2):
        o = np.full_like(pre, 0xDEADBEEF)
        _lib.call("pil2gl_selftest_poseidon", gl._ptr(pre), pre.shape[0], what, gl._ptr(o))
        _same(o, Y, ("selftest_poseidon", what))
    got = gl.poseidon_batch(np.ascontiguousarray(pre[:, :8]), np.ascontiguousarray(pre[:, 8:]), 12)
    _same(got, Y, "poseidon_batch with capacity")
    got4 = gl.poseidon_batch(np.ascontiguousarray(pre[:, :8]), np.ascontiguousarray(pre[:, 8:]), 4)
    _same(got4, Y[:, :4], "poseidon_batch, four outputs")
