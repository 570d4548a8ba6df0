"""BN254 Fr transforms on the device (pil2gl.bn128.fft / ifft / interpolate over csrc/bn_ntt.hip) against the Python checker
(tests/bn128_fft_ref.py).  Every comparison is exact equality of the Montgomery words."""
import ctypes as C
import random

import numpy as np
import pytest

import bn128_fft_ref as ref
from bn128_fft_ref import R

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def bn():
    import pil2gl
    from pil2gl import bn128
    pil2gl.init(0)
    return bn128


def dev(words):
    return torch.from_numpy(np.ascontiguousarray(words).view(np.int64)).cuda()


def host(t):
    return t.cpu().numpy().view(np.uint64)


def rand_cols(n_bits, n_pols, seed):
    rng = random.Random(seed)
    return [[rng.randrange(R) for _ in range(1 << n_bits)] for _ in range(n_pols)]


def same(got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape
    bad = np.argwhere((got != want).any(axis=-1))
    assert bad.size == 0, "first difference at (row, pol) %s of %d" % (bad[0].tolist(), len(bad))


def max_single_sweep(lib):
    """K: the largest transform the plan does in one sweep"""
    k = 0
    while True:
        layers = (C.c_uint32 * 8)(); n = C.c_uint32()
        assert lib.pil2gl_debug_bn128_fft_plan(k + 1, layers, 8, C.byref(n)) == 0
        if n.value > 1:
            return k
        k += 1


def last_sweep_layers(lib, n_bits):
    layers = (C.c_uint32 * 8)(); n = C.c_uint32()
    assert lib.pil2gl_debug_bn128_fft_plan(n_bits, layers, 8, C.byref(n)) == 0
    return layers[n.value - 1]


# ---- small shapes against the checker ------------------------------------------------------------------------------------------------
SMALL = [(b, p) for b in (0, 1, 2, 3, 5) for p in (1, 2, 5)] + [(12, 3)]


@pytest.mark.parametrize("n_bits,n_pols", SMALL)
def test_fft_and_ifft_match_the_checker(bn, n_bits, n_pols):
    x = ref.matrix_words(rand_cols(n_bits, n_pols, 1000 * n_bits + n_pols))
    same(host(bn.fft(dev(x), n_pols, n_bits)), ref.apply_cols(ref.ntt, x))
    same(host(bn.ifft(dev(x), n_pols, n_bits)), ref.apply_cols(ref.intt, x))


def test_reference_fill_host_and_device_and_in_place(bn):
    """test/fft_p.bn128.test.js:21-33: polynomial i at row j = i*degree + j, at (nBits, nPols) = (5, 2); through the host-pointer
    entries, the device entries, and with dst == src"""
    n_bits, n_pols, degree = 5, 2, 32
    x = ref.matrix_words([[i * degree + j for j in range(degree)] for i in range(n_pols)])
    f, fi = ref.apply_cols(ref.ntt, x), ref.apply_cols(ref.intt, x)
    same(bn.fft(x.copy(), n_pols, n_bits), f)
    same(bn.ifft(x.copy(), n_pols, n_bits), fi)
    same(host(bn.fft(dev(x), n_pols, n_bits)), f)
    d = dev(x); r = bn.fft(d, n_pols, n_bits, out=d)
    assert r.data_ptr() == d.data_ptr()
    same(host(d), f)
    d = dev(x); bn.ifft(d, n_pols, n_bits, out=d)
    same(host(d), fi)
    h = x.copy(); bn.fft(h, n_pols, n_bits, out=h)
    same(h, f)


# ---- interpolate ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_bits,n_pols,ext_bits", [(3, 1, 1), (0, 2, 3), (5, 5, 0), (10, 3, 2)])
def test_interpolate_matches_the_checker(bn, n_bits, n_pols, ext_bits):
    cols = rand_cols(n_bits, n_pols, 77 + n_bits)
    x = ref.matrix_words(cols)
    want = [ref.interpolate(c, n_bits + ext_bits) for c in cols]
    w_coefs, w_ext = ref.matrix_words([c for c, _ in want]), ref.matrix_words([e for _, e in want])
    coefs, ext = bn.interpolate(dev(x), n_pols, n_bits, n_bits + ext_bits)
    same(host(coefs), w_coefs); same(host(ext), w_ext)
    if n_bits == 3:                                                   # the host-pointer entry, and dstCoefs = NULL on both
        coefs, ext = bn.interpolate(x, n_pols, n_bits, n_bits + ext_bits)
        same(coefs, w_coefs); same(ext, w_ext)
        none, ext = bn.interpolate(dev(x), n_pols, n_bits, n_bits + ext_bits, coefs=False)
        assert none is None
        same(host(ext), w_ext)
        none, ext = bn.interpolate(x, n_pols, n_bits, n_bits + ext_bits, coefs=False)
        assert none is None
        same(ext, w_ext)


# ---- chosen operands ---------------------------------------------------------------------------------------------------------------
def chosen_pairs():
    """(A, B): Montgomery WORDS of the two rows of a 2-point transform, whose butterfly is A + B, A - B mod r"""
    ones = (0x30644e71 << 224) | ((1 << 224) - 1)                    # seven low 32-bit limbs all ones under a top limb of 0x30644e71
    p255 = (1 << 255) % R
    pats = [ones, R - 1, p255, 1, 1 << 31, 1 << 32, 1 << 63, 1 << 64, 1 << 127, 1 << 128, 1 << 191, 1 << 192, 1 << 223, 1 << 224, 1 << 253]
    assert all(0 <= v < R for v in pats)
    pairs = [(5, R - 5), (ones, R - ones), (p255, R - p255), (1 << 253, R - (1 << 253)),        # A + B = r exactly
             (7, 7), (ones, ones), (p255, p255),                                                # A = B
             (0, 12345), (0, ones), (0, R - 1), (0, 0),                                         # A = 0
             (12345, 0), (ones, 0), (R - 1, 0),                                                 # B = 0
             (R - 1, R - 1),
             (6, R - 5), (ones + 1, R - ones), (R - 1, 2)]                                      # A + B = r + 1
    pairs += [(a, b) for a in pats for b in (pats[0], pats[1], pats[2], 1)]
    pairs += [(b, a) for a in pats[3:] for b in (pats[0], pats[1])]
    return pairs


def test_two_point_butterfly_on_chosen_words(bn):
    pairs = chosen_pairs()
    while len(pairs) % 8:
        pairs.append((0, 0))
    inv2 = pow(2, -1, R)
    for o in range(0, len(pairs), 8):                                 # nPols 8: a row fills the lanes of the column group
        grp = pairs[o:o + 8]
        x = np.stack([ref.words_of([a for a, _ in grp]), ref.words_of([b for _, b in grp])])
        assert x.shape == (2, 8, 4)
        want = np.stack([ref.words_of([(a + b) % R for a, b in grp]), ref.words_of([(a - b) % R for a, b in grp])])
        same(host(bn.fft(dev(x), 8, 1)), want)
        want = np.stack([ref.words_of([(a + b) * inv2 % R for a, b in grp]), ref.words_of([(a - b) * inv2 % R for a, b in grp])])
        same(host(bn.ifft(dev(x), 8, 1)), want)


@pytest.mark.parametrize("n_bits", (3, 5))
def test_one_hot_and_constant_inputs(bn, n_bits):
    """a single non-zero row (output: a column of twiddle powers; t = 0 in all butterflies but one per layer) and a constant column
    (output: n c at row 0 and zeros; u = t in every layer)"""
    n = 1 << n_bits
    g = ref.w(n_bits)
    c = [0x1234567890abcdef1234567890abcdef % R, R - 1]
    for hot in (0, 1, n - 1, n // 2 + 1):
        cols = [[c[i] if j == hot else 0 for j in range(n)] for i in range(2)]
        want = [[c[i] * pow(g, hot * j, R) % R for j in range(n)] for i in range(2)]
        assert want == [ref.ntt(col) for col in cols]
        same(host(bn.fft(dev(ref.matrix_words(cols)), 2, n_bits)), ref.matrix_words(want))
        same(host(bn.ifft(dev(ref.matrix_words(want)), 2, n_bits)), ref.matrix_words(cols))
    cols = [[c[i]] * n for i in range(2)]
    want = [[c[i] * n % R] + [0] * (n - 1) for i in range(2)]
    same(host(bn.fft(dev(ref.matrix_words(cols)), 2, n_bits)), ref.matrix_words(want))
    same(host(bn.ifft(dev(ref.matrix_words(cols)), 2, n_bits)), ref.matrix_words([[c[i]] + [0] * (n - 1) for i in range(2)]))


# ---- sweep boundaries: sizes the checker is too slow for ------------------------------------------------------------------------------
def boundary_shapes():
    import pil2gl
    k = max_single_sweep(pil2gl.load())
    return k, [(k, 3), (k + 1, 3), (min(2 * k + 1, 22), 3), (k + 1, 1), (k + 1, 17)]


def device_words(n_bits, n_pols, seed):
    """canonical words made on the device: every 64-bit limb below 2^62 and the top one below 2^58, so that the limb-wise sum of two
    such matrices has no carry and stays below 2^251 < r (linearity needs x + y without field arithmetic of the test's own)"""
    gen = torch.Generator(device="cuda"); gen.manual_seed(seed)
    t = torch.randint(0, 1 << 62, (1 << n_bits, n_pols, 4), dtype=torch.int64, device="cuda", generator=gen)
    t[:, :, 3] >>= 4
    return t


def sample_rows(lib, n_bits, count, seed):
    """`count` random rows plus 0, 1, n/2, n-1 and the first and last output row of EVERY tile of the last sweep: that sweep's tile b
    stores its 2^k rows at brev(q) * 2^(nBits-k) + brev(b), so the first rows are 0 .. 2^(nBits-k) - 1 and the last are the top as many"""
    n = 1 << n_bits
    tiles = n >> last_sweep_layers(lib, n_bits)
    rows = {0, 1, n // 2, n - 1} | set(range(tiles)) | set(range(n - tiles, n))
    rng = random.Random(seed)
    while len(rows) < min(n, tiles * 2 + count):
        rows.add(rng.randrange(n))
    return sorted(rows)


def test_plan_puts_these_sizes_on_the_boundaries():
    import pil2gl
    lib = pil2gl.load()
    k, shapes = boundary_shapes()
    assert k >= 5 and (32 << k) <= lib.pil2gl_debug_bn128_fft_tile_bytes()
    n = C.c_uint32(); layers = (C.c_uint32 * 8)()
    for bits, want in ((k, 1), (k + 1, 2), (min(2 * k + 1, 22), 3 if 2 * k + 1 <= 22 else None)):
        assert lib.pil2gl_debug_bn128_fft_plan(bits, layers, 8, C.byref(n)) == 0
        assert want is None or n.value == want


@pytest.mark.parametrize("which", range(5))
def test_round_trip_on_the_sweep_boundaries(bn, which):
    n_bits, n_pols = boundary_shapes()[1][which]
    x = device_words(n_bits, n_pols, 5 + which)
    y = bn.ifft(bn.fft(x, n_pols, n_bits), n_pols, n_bits)
    assert torch.equal(x, y)
    y = bn.fft(bn.ifft(x, n_pols, n_bits), n_pols, n_bits)
    assert torch.equal(x, y)


@pytest.mark.parametrize("which", range(5))
def test_closed_form_on_the_sweep_boundaries(bn, which):
    """coefficients zero but for indices 1, n/2+1 and n-1: row j of the transform is c1 w^j + c2 w^(j(n/2+1)) + c3 w^(j(n-1))
    = w^j (c1 + (-1)^j c2) + c3 w^(-j)"""
    import pil2gl
    n_bits, n_pols = boundary_shapes()[1][which]
    n = 1 << n_bits
    rng = random.Random(40 + which)
    c = [[rng.randrange(R) for _ in range(3)] for _ in range(n_pols)]
    x = torch.zeros((n, n_pols, 4), dtype=torch.int64, device="cuda")
    for i, k in enumerate((1, n // 2 + 1, n - 1)):
        x[k] = dev(ref.words_of([ref.to_mont(c[p][i]) for p in range(n_pols)]))
    rows = sample_rows(pil2gl.load(), n_bits, 2048, which)
    got = host(bn.fft(x, n_pols, n_bits)[torch.tensor(rows, device="cuda")])
    g = ref.w(n_bits)
    gi = pow(g, -1, R)
    want = []
    for j in rows:
        wj, wij = pow(g, j, R), pow(gi, j, R)
        want += [ref.to_mont(wj * (c[p][0] + (-1) ** j * c[p][1]) + c[p][2] * wij) for p in range(n_pols)]
    same(got, ref.words_of(want).reshape(len(rows), n_pols, 4))


@pytest.mark.parametrize("which", range(5))
def test_linearity_on_the_sweep_boundaries(bn, which):
    n_bits, n_pols = boundary_shapes()[1][which]
    x, y = device_words(n_bits, n_pols, 60 + which), device_words(n_bits, n_pols, 80 + which)
    n = 1 << n_bits
    rows = torch.tensor(sorted({0, 1, n // 2, n - 1} | set(random.Random(9 + which).sample(range(n), min(n, 2048)))), device="cuda")
    fx, fy, fs = (host(bn.fft(t, n_pols, n_bits)[rows]) for t in (x, y, x + y))
    want = [(a + b) % R for a, b in zip(ref.ints_of(fx), ref.ints_of(fy))]
    same(fs, ref.words_of(want).reshape(fs.shape))


# ---- stream order -------------------------------------------------------------------------------------------------------------------
def test_fft_dev_runs_in_stream_order(bn):
    """the transform enqueued behind a device-side fill on a non-default stream, no synchronise between the two"""
    n_bits, n_pols = 12, 3
    x = ref.matrix_words(rand_cols(n_bits, n_pols, 4242))
    want = ref.apply_cols(ref.ntt, x)
    xd = dev(x)
    d = torch.zeros_like(xd); out = torch.zeros_like(xd)
    ballast = torch.empty(1 << 25, dtype=torch.int64, device="cuda")
    bn.fft(xd, n_pols, n_bits)                                         # tables and scratch exist before the ordered part
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        for v in range(8):
            ballast.fill_(v)                                          # work ahead of the fill on the same stream
        d.copy_(xd)
        bn.fft(d, n_pols, n_bits, out=out)
    s.synchronize()
    same(host(out), want)
