"""pil2gl.bn128's wrappers share one kind check: a call that names a host array next to a device buffer is refused with one message before
the library is reached.  No device: a marker class stands for the device tensor, and `call` is replaced by a recorder.
Every wrapper that takes two or more buffers is here, once per position a foreign buffer can take; interpolate, poly_eval and poly_degree
take one buffer (their points are host words by contract) and have nothing to mix."""
import numpy as np
import pytest


class Dev:
    """stands for a device tensor: the kind check looks at nothing else"""
    shape = (8, 4)


A = np.ones((8, 4), np.uint64)
E = np.ones(4, np.uint64)
D = Dev()
ONE_POLY = [(0, 2, [0])]

CASES = {
    "fft out": lambda bn: bn.fft(A, 1, 3, out=D),
    "fft words": lambda bn: bn.fft(D, 1, 3, out=A),
    "ifft out": lambda bn: bn.ifft(A, 1, 3, out=D),
    "ifft words": lambda bn: bn.ifft(D, 1, 3, out=A),
    "g1_msm scalars": lambda bn: bn.g1_msm(A, D),
    "g1_msm bases": lambda bn: bn.g1_msm(D, A),
    "g1_msm out": lambda bn: bn.g1_msm(A, A, out=D),
    "g1_commit scalars": lambda bn: bn.g1_commit(A, D, ONE_POLY, 1),
    "g1_commit bases": lambda bn: bn.g1_commit(D, A, ONE_POLY, 1),
    "g1_commit out": lambda bn: bn.g1_commit(A, A, ONE_POLY, 1, out=D),
    "eval_program": lambda bn: bn.eval_program([], [A.reshape(8, 1, 4), None, D], None, 3),
    "poly_div out": lambda bn: bn.poly_div(A, 1, E, out=D),
    "poly_div words": lambda bn: bn.poly_div(D, 1, E, out=A),
    "poly_fma src": lambda bn: bn.poly_fma(A, D, E, [0], n_acc=8, n_src=8),
    "poly_fma acc": lambda bn: bn.poly_fma(D, A, E, [0], n_acc=8, n_src=8),
    "batch_inverse out": lambda bn: bn.batch_inverse(A, out=D),
    "batch_inverse words": lambda bn: bn.batch_inverse(D, out=A),
    "gprod num": lambda bn: bn.gprod(D, A),
    "gprod den": lambda bn: bn.gprod(A, D),
    "gprod out": lambda bn: bn.gprod(A, A, out=D),
    "gsum out": lambda bn: bn.gsum(E, A, out=D),
    "gsum den": lambda bn: bn.gsum(E, D, out=A),
    "h1h2 f": lambda bn: bn.h1h2(D, A),
    "h1h2 t": lambda bn: bn.h1h2(A, D),
    "h1h2 h1": lambda bn: bn.h1h2(A, A, h1=D),
    "h1h2 h2": lambda bn: bn.h1h2(A, A, h2=D),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_a_host_array_next_to_a_device_buffer_is_refused_before_the_library(monkeypatch, case):
    import pil2gl
    from pil2gl import bn128
    reached = []
    is_dev = lambda b: isinstance(b, Dev)
    monkeypatch.setattr(pil2gl, "_is_dev", is_dev)
    monkeypatch.setattr(bn128, "_is_dev", is_dev)
    monkeypatch.setattr(bn128, "call", lambda name, *args: reached.append(name))
    with pytest.raises(pil2gl.Pil2glError) as err:
        CASES[case](bn128)
    assert str(err.value) == "mixing host and device buffers in one call"
    assert reached == []
