"""Decimation-in-frequency layers of a BN254 Fr transform, in Python integers, with a record of what enters every twiddle product; and the
columns that steer chosen words into those products (tests/test_gpu_bn128_fft_shapes.py part C, checked without a device in
tests/test_bn128_fft_cpu.py).  Not a test.

Everything here works on Montgomery WORDS taken as integers below r: sums and differences of words are the words of the sums and
differences, and a word times a normal-form twiddle is the word of the product.  The layer of distance 2^t maps the pair (a, b) at
positions (q0, q0 + 2^t), q0 = (pi >> t << (t + 1)) | j, j < 2^t, to (a + b, (a - b) w_{2^(t+1)}^j); the distance-1 layer has no product.
After the layers position p holds the output of index brev(p)."""
import bn128_fft_ref as ref
from bn128_fft_ref import R


def dif(col, inverse=False):
    """col: the words of one column, length 2^k -> (the transform's words in natural order, the set of (d, t, j): the difference word d
    met the twiddle w_{2^(t+1)}^j, or its inverse, in the layer of distance 2^t >= 2)"""
    n = len(col)
    k = n.bit_length() - 1
    assert n == 1 << k
    a = [v % R for v in col]
    met = set()
    for t in range(k - 1, -1, -1):
        g = ref.w(t + 1)
        if inverse:
            g = pow(g, -1, R)
        for pi in range(n // 2):
            j = pi & ((1 << t) - 1)
            q0 = ((pi >> t) << (t + 1)) | j
            u, v = a[q0], a[q0 + (1 << t)]
            d = (u - v) % R
            if t > 0:
                met.add((d, t, j))
                d = d * pow(g, j, R) % R
            a[q0], a[q0 + (1 << t)] = (u + v) % R, d
    scale = pow(n, -1, R) if inverse else 1
    return [a[ref._brev(p, k)] * scale % R for p in range(n)], met


def chosen_words(pairs):
    """the distinct non-zero words of chosen_pairs() (tests/test_gpu_bn128_fft.py), in their order of appearance"""
    seen = []
    for p in pairs:
        for v in p:
            if v and v not in seen:
                seen.append(v)
    return seen


def twiddle_cases(n_bits, x):
    """columns of 2^n_bits words (n_bits 2 or 3) that present the word x to every twiddle of a transform of that size.
    4 rows: (0, x, 0, 0) has x meet w_4; (0, x, 0, r - x) has 2x meet it while the sum above it is r exactly; (x, 0, x, 0) has a zero
    difference meet 1 under the sum 2x; (x, 0, 0, 0) has x meet 1.  8 rows: x alone at each position in turn -- at position p < 4 it
    meets w_8^p and then w_4^(p mod 2), at p >= 4 its negative does."""
    assert 0 < x < R
    if n_bits == 2:
        return [[0, x, 0, 0], [0, x, 0, R - x], [x, 0, x, 0], [x, 0, 0, 0]]
    assert n_bits == 3
    return [[x if j == p else 0 for j in range(8)] for p in range(8)]


def twiddles_of(n_bits):
    """(t, j) of every twiddle product of a transform of 2^n_bits rows"""
    return {(t, j) for t in range(1, n_bits) for j in range(1 << t)}
