"""The chunk walk on the device: transforms whose 16-slot pass kernels walk several column chunks per workgroup (csrc/ntt.hip, walk_at),
word for word against gl_oracle.  Each case first reads from the host-only plan how its launches walk -- more than one chunk, or exactly
one where that is the point -- so none of them passes on one chunk per workgroup.  The mid kernel keeps one tile per workgroup; its
cases check the walking passes around it (and the 2^17-row ones the mapping it shares with them)."""
import numpy as np
import pytest

from conftest import rand_field

import transform_plan as tp
import transform_walk as tw

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gl():
    import pil2gl
    pil2gl.init(0)
    return pil2gl


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64).reshape(-1)).cuda()


def _out(words):
    import torch
    return torch.full((words,), 0xDEADBEEF, dtype=torch.int64, device="cuda")


def _host(t, shape):
    return t.cpu().numpy().view(np.uint64).reshape(shape)


def _walks(op, nb, C, eb=0, cosets=0):
    """[(kind, fixed slots, column chunks, W, grid)] of the call's launches"""
    return [(l.kind, l.fixed, l.chunks, g.walk, g.grid) for l, g in zip(tp.plan(op, nb, C, eb, cosets), tw.grids(op, nb, C, eb, cosets))]


_TRACES = {}


def _trace(nb, C):
    if (nb, C) not in _TRACES:
        _TRACES[nb, C] = rand_field(np.random.default_rng(nb * 1000 + C), (1 << nb, C))
    return _TRACES[nb, C]


# (rows, columns): (chunks, W) of every pass of fft and ifft
_NTT = {(8, 16): (1, 1),       # one chunk, no inter-pass table
        (8, 17): (2, 2),       # two chunks in one workgroup, the second a single ragged column
        (16, 31): (2, 2),      # 16 + 15, two passes with the inter-pass table, scatter store; W divides the chunks
        (16, 33): (3, 2),      # 2 + 1: a remainder run
        (16, 100): (7, 2),     # 2 + 2 + 2 + 1, ragged last chunk of 4 columns
        (16, 112): (7, 2)}     # seven full chunks


@pytest.mark.parametrize("nb,C", sorted(_NTT))
def test_fft_and_ifft_walk_their_chunks(gl, oracle, nb, C):
    """forward DIF and inverse DIF instances, with and without the inter-pass table, last pass scattering"""
    chunks, walk = _NTT[nb, C]
    a = _trace(nb, C)
    for op, fn, ref in (("fft", gl.fft, oracle.fft_cols), ("ifft", gl.ifft, oracle.ifft_cols)):
        w = _walks(op, nb, C)
        assert len(w) == nb // 8 and all(l[1:4] == (16, chunks, walk) for l in w), w
        dst = _out(a.size)
        fn(_dev(a), C, nb, dst)
        assert np.array_equal(_host(dst, a.shape), ref(a, nb)), (op, nb, C)


@pytest.fixture(scope="module")
def lde16(oracle):
    """2^16 x 100 onto 2^19: the whole extension, once for the tests below"""
    return oracle.interpolate(_trace(16, 100), 16, 19)


@pytest.mark.parametrize("eb", [1, 2, 3])
def test_interpolate_walks_on_both_sides_of_the_mid_kernel(gl, oracle, lde16, eb):
    """inverse DIF pass on 100 columns (7 chunks), mid kernel, DIT pass on 200 / 400 / 800 columns (13 / 25 / 50 chunks in runs of
    3 / 6 / 12 and a remainder): with fft and ifft above, every walking instance on one shape"""
    a = _trace(16, 100)
    w = _walks("interpolate", 16, 100, eb)
    nc = -(-(100 << eb) // 16)
    assert w == [("i", 16, 7, 2, 1024), ("m", 16, 7, 1, 1792), ("d", 16, nc, nc // 4, 256 * -(-nc // (nc // 4)))], w
    assert nc % (nc // 4)
    dst = _out(a.size << eb)
    gl.interpolate(_dev(a), 100, 16, dst, 16 + eb)
    want = lde16 if eb == 3 else oracle.interpolate(a, 16, 16 + eb)
    assert np.array_equal(_host(dst, want.shape), want)


def test_a_coset_slice_walks(gl, lde16):
    """cosets [3, 5) of 8: the DIT pass runs on 200 columns, 13 chunks in runs of 3"""
    a = _trace(16, 100)
    w = _walks("interpolate", 16, 100, 3, 2)
    assert w == [("i", 16, 7, 2, 1024), ("m", 16, 7, 1, 1792), ("d", 16, 13, 3, 1280)], w
    dst = _out(a.size * 2)
    gl.interpolateCosets(_dev(a), 100, 16, dst, 19, 3, 2)
    want = np.ascontiguousarray(lde16.reshape(1 << 16, 8, 100)[:, 3:5])
    assert np.array_equal(_host(dst, want.shape), want)


def test_extension_from_coefficients_2_17_x_20(gl, oracle):
    """2^17 x 20 by 3 bits from coefficients in bit-reversed rows: the 16-slot mid kernel (16 + 4 columns) between any-geometry passes --
    exactly one tile per workgroup, through the same mapping"""
    from pil2gl import _lib
    nb, C, eb = 17, 20, 3
    w = _walks("extend_coefs", nb, C, eb)
    assert w[0] == ("m", 16, 2, 1, 1024) and all(l[1] == 0 and l[3] == 1 for l in w[1:]), w
    c = _trace(nb, C)
    i = np.arange(1 << nb, dtype=np.uint64)
    br = np.zeros_like(i)
    for b in range(nb):
        br |= ((i >> np.uint64(b)) & np.uint64(1)) << np.uint64(nb - 1 - b)
    padded = np.zeros((1 << (nb + eb), C), np.uint64)
    padded[:1 << nb] = c
    want = oracle.fft_cols(padded, nb + eb)
    dst = _out(C << (nb + eb))
    _lib.call("pil2gl_extend_coefs_brev_dev", gl._ptr(_dev(c[br])), C, nb, gl._ptr(dst), nb + eb, None)
    assert np.array_equal(_host(dst, want.shape), want)
