"""The 16-slot fixed-geometry tile kernels (ntt_pass_kernel<.., 8, 16>, lde_mid_kernel<16, 16>) move a tile between HBM and LDS in
pairs of column slots: a lane owns two adjacent slots of eight rows, and the ragged last lane of a chunk with an odd column count owns
one.  Every shape here is the smallest that runs those instances -- the plan is asserted, so no case can pass on the any-geometry
kernels -- and every result is compared bit for bit with the CPU oracle.

Widths: 16 (one full chunk), 20 (16 + a ragged 4, config 3's pattern), 31 (16 + 15: the one-column lane, and rows that start on 8
bytes), 100 (6 x 16 + 4).  2^16 rows select the fixed mid kernel for all four widths (asserted).  The row count of a transform is a
power of two and a tile takes 2^8 of them, so no workgroup is ever short of ROWS; the partly empty workgroups that exist are the
ragged last column chunks (4, 15 and 8 of 16 slots), which widths 20, 31 and 100 reach on every launch.

Inputs: uniform canonical elements; every word p - 1; all zeros (the canonical store); and columns that are each one distinct nonzero
coefficient, so a wrong twiddle, slot or row index shows as a wrong column."""
import numpy as np
import pytest

from conftest import P, rand_field

pytestmark = pytest.mark.gpu

N_BITS, EXT = 16, 3
WIDTHS = (16, 20, 31, 100)
INPUTS = ("uniform", "p_minus_1", "zeros", "single_coefficient")


@pytest.fixture(scope="module")
def gl():
    import pil2gl
    pil2gl.init(0)
    return pil2gl


def _coefficients(kind, n_bits, C):
    """(2^n_bits, C) coefficient matrix of the `single_coefficient` input: column c holds value c + 2 at a row of its own"""
    n = 1 << n_bits
    a = np.zeros((n, C), dtype=np.uint64)
    rows = (np.arange(C, dtype=np.uint64) * np.uint64(2654435761) + np.uint64(7)) % np.uint64(n)
    rows = (rows + np.arange(C, dtype=np.uint64) * np.uint64(n // 128 + 1)) % np.uint64(n)
    a[rows.astype(np.int64), np.arange(C)] = np.arange(C, dtype=np.uint64) + np.uint64(2)
    return a


_cache = {}


def _input(oracle, kind, n_bits, C, evaluations):
    """the input matrix; evaluations: the transform takes values on the domain (ifft, interpolate), so the single coefficients are
    handed over as their evaluations"""
    key = (kind, n_bits, C, evaluations)
    if key not in _cache:
        n = 1 << n_bits
        if kind == "uniform":
            a = rand_field(np.random.default_rng(1000 * n_bits + C), (n, C))
        elif kind == "p_minus_1":
            a = np.full((n, C), P - 1, dtype=np.uint64)
        elif kind == "zeros":
            a = np.zeros((n, C), dtype=np.uint64)
        else:
            a = _coefficients(kind, n_bits, C)
            if evaluations:
                a = oracle.fft_cols(a, n_bits)
        a.setflags(write=False)
        _cache[key] = a
    return _cache[key]


def _run(gl, op, a, n_bits, n_bits_out):
    import torch
    C = a.shape[1]
    src = torch.from_numpy(a.view(np.int64).copy()).cuda()
    dst = torch.empty((1 << n_bits_out) * C, dtype=torch.int64, device="cuda")
    if op == "interpolate":
        gl.interpolate(src, C, n_bits, dst, n_bits_out)
    else:
        getattr(gl, op)(src, C, n_bits, dst)
    torch.cuda.synchronize()
    return dst.cpu().numpy().view(np.uint64).reshape(1 << n_bits_out, C)


def _same(got, want, what):
    bad = np.argwhere(got != want)
    assert bad.size == 0, "%s: %d words differ, columns %s, first at row %d column %d" % (
        what, len(bad), sorted(set(bad[:, 1].tolist()))[:8], bad[0][0], bad[0][1])


def _kernels(launches):
    return [(l.kind, l.k, l.fixed) for l in launches]


def test_the_shapes_run_the_sixteen_slot_instances():
    """what the cases below claim, read from the planner: three 8-stage launches per interpolate, two per transform, all on the
    16-slot fixed-geometry instances"""
    import transform_plan as tp
    for C in WIDTHS:
        assert _kernels(tp.plan("interpolate", N_BITS, C, EXT)) == [("i", 8, 16), ("m", 8, 16), ("d", 8, 16)], C
        assert _kernels(tp.plan("interpolate", 8, C, EXT)) == [("m", 8, 16)], C
    for C in (16, 20):
        for op, kind in (("fft", "f"), ("ifft", "i")):
            assert _kernels(tp.plan(op, N_BITS, C)) == [(kind, 8, 16), (kind, 8, 16)], (op, C)
            assert _kernels(tp.plan(op, 8, C)) == [(kind, 8, 16)], (op, C)


@pytest.mark.parametrize("kind", INPUTS)
@pytest.mark.parametrize("C", WIDTHS)
def test_interpolate_three_passes(gl, oracle, C, kind):
    """2^16 -> 2^19 rows: inverse pass, fixed mid kernel, forward pass on the 8 C columns of the extension"""
    import transform_plan as tp
    p = tp.plan("interpolate", N_BITS, C, EXT)
    assert _kernels(p) == [("i", 8, 16), ("m", 8, 16), ("d", 8, 16)], p
    assert p[1].ept == 16 and p[2].canon == 1
    a = _input(oracle, kind, N_BITS, C, True)
    _same(_run(gl, "interpolate", a, N_BITS, N_BITS + EXT), oracle.interpolate(a, N_BITS, N_BITS + EXT), "interpolate 2^16 x %d %s" % (C, kind))


@pytest.mark.parametrize("kind", INPUTS)
@pytest.mark.parametrize("C", (16, 31))
def test_interpolate_mid_kernel_alone(gl, oracle, C, kind):
    """2^8 -> 2^11 rows: the mid kernel is the whole transform and stores the canonical result itself"""
    import transform_plan as tp
    p = tp.plan("interpolate", 8, C, EXT)
    assert _kernels(p) == [("m", 8, 16)] and p[0].canon == 1, p
    a = _input(oracle, kind, 8, C, True)
    _same(_run(gl, "interpolate", a, 8, 8 + EXT), oracle.interpolate(a, 8, 8 + EXT), "interpolate 2^8 x %d %s" % (C, kind))


@pytest.mark.parametrize("kind", INPUTS)
@pytest.mark.parametrize("C", (16, 20))
@pytest.mark.parametrize("op", ("fft", "ifft"))
def test_transform_two_passes(gl, oracle, op, C, kind):
    """2^16 rows: a pass with inter-pass twiddles (and the 1/N of an inverse folded into them), then the scattering pass that
    stores canonical values at bit-reversed rows"""
    import transform_plan as tp
    p = tp.plan(op, N_BITS, C)
    assert _kernels(p) == [("fi"[op == "ifft"], 8, 16)] * 2 and p[1].scatter == 1 and p[1].canon == 1, p
    a = _input(oracle, kind, N_BITS, C, op == "ifft")
    want = oracle.fft_cols(a, N_BITS) if op == "fft" else oracle.ifft_cols(a, N_BITS)
    _same(_run(gl, op, a, N_BITS, N_BITS), want, "%s 2^16 x %d %s" % (op, C, kind))


@pytest.mark.parametrize("kind", ("uniform", "single_coefficient"))
@pytest.mark.parametrize("C", (16, 31))
@pytest.mark.parametrize("op", ("fft", "ifft"))
def test_transform_one_pass(gl, oracle, op, C, kind):
    """2^8 rows: one scattering pass without inter-pass twiddles; the inverse multiplies by 1/N on the way out"""
    import transform_plan as tp
    p = tp.plan(op, 8, C)
    assert _kernels(p) == [("fi"[op == "ifft"], 8, 16)] and p[0].scatter == 1, p
    a = _input(oracle, kind, 8, C, op == "ifft")
    want = oracle.fft_cols(a, 8) if op == "fft" else oracle.ifft_cols(a, 8)
    _same(_run(gl, op, a, 8, 8), want, "%s 2^8 x %d %s" % (op, C, kind))
