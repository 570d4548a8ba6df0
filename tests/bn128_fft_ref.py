"""Checker for the BN254 Fr transforms (pil2gl_bn128_fft / _ifft / _interpolate), in Python integers, written from the definitions:

  r      = the BN254 scalar field's modulus
  w(k)   = ffjavascript's Fr.w[k]: w(28) = 5^((r-1)/2^28) mod r (5 is the smallest quadratic non-residue), w(k) = w(k+1)^2
  fft    : dst[j] = sum_k src[k] w(nBits)^(jk), natural order in and out
  ifft   : its inverse, dst[k] = 1/n sum_j src[j] w(nBits)^(-jk)
  interpolate(x, nBitsExt) = (coefs, fft of coefs padded with zeros to 2^nBitsExt): no coset shift (fft_worker.bn128.js:15-22)

Vectors are lists of ints in normal form, one polynomial at a time; the matrix helpers at the end go column by column and convert to and
from the library's words (four little-endian u64 of a * 2^256 mod r).  Not a test, and nothing here knows how the device computes.
"""
import numpy as np

R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
W28 = 19103219067921713944291392827692070036145651957329286315305642004821462161904
S = 28
MONT = (1 << 256) % R
MONT_INV = pow(MONT, -1, R)


def w(k):
    assert 0 <= k <= S
    return pow(pow(5, (R - 1) >> S, R), 1 << (S - k), R)


def dft_naive(x, root=None):
    """straight from the definition, O(n^2)"""
    n = len(x)
    g = w(n.bit_length() - 1) if root is None else root
    return [sum(x[k] * pow(g, j * k % n, R) for k in range(n)) % R for j in range(n)]


def _brev(i, bits):
    return int(format(i, "0%db" % bits)[::-1], 2) if bits else 0


def _radix2(x, g):
    """iterative radix-2, decimation in time: bit-reversed copy, then layers of growing span"""
    n = len(x)
    bits = n.bit_length() - 1
    assert n == 1 << bits
    a = [x[_brev(i, bits)] % R for i in range(n)]
    span = 1
    while span < n:
        step = pow(g, n // (2 * span), R)
        for base in range(0, n, 2 * span):
            t = 1
            for j in range(span):
                u, v = a[base + j], a[base + j + span] * t % R
                a[base + j], a[base + j + span] = (u + v) % R, (u - v) % R
                t = t * step % R
        span *= 2
    return a


def ntt(x):
    return _radix2(x, w(len(x).bit_length() - 1))


def intt(x):
    n = len(x)
    ninv = pow(n, -1, R)
    return [v * ninv % R for v in _radix2(x, pow(w(n.bit_length() - 1), -1, R))]


def interpolate(x, n_bits_ext):
    coefs = intt(x)
    return coefs, ntt(coefs + [0] * ((1 << n_bits_ext) - len(x)))


def batch_inverse(vals):
    """Montgomery's trick: the inverses of non-zero vals with one modular inversion"""
    prefix, acc = [], 1
    for v in vals:
        assert v % R, "zero in a batch inversion"
        prefix.append(acc)
        acc = acc * v % R
    inv = pow(acc, -1, R)
    out = [0] * len(vals)
    for i in range(len(vals) - 1, -1, -1):
        out[i] = inv * prefix[i] % R
        inv = inv * vals[i] % R
    return out


def geometric_ntt_rows(c, a, n_bits, rows, inverse=False):
    """rows `rows` of the transform of the geometric column x_j = c a^j, j < n = 2^n_bits, without the transform: with g = w(n_bits),
    or its inverse for the inverse transform, sum_j c a^j g^(jk) = c ((a g^k)^n - 1) / (a g^k - 1) = c (a^n - 1) / (a g^k - 1),
    and the inverse transform divides by n.  Needs a^n != 1 (a = 1 and every n-th root of unity are refused): then a g^k != 1 for
    every k and no denominator is zero."""
    n = 1 << n_bits
    c, a = c % R, a % R
    an = pow(a, n, R)
    if an == 1:
        raise ValueError("geometric_ntt_rows: a^n = 1, the closed form has a zero denominator")
    g = w(n_bits)
    if inverse:
        g = pow(g, -1, R)
    num = c * (an - 1) % R
    if inverse:
        num = num * pow(n, -1, R) % R
    inv = batch_inverse([(a * pow(g, k % n, R) - 1) % R for k in rows])
    return [num * d % R for d in inv]


# ---- the library's words -----------------------------------------------------------------------------------------------------
def to_mont(v):
    return v % R * MONT % R


def from_mont(v):
    return v * MONT_INV % R


def words_of(vals):
    """ints (< 2^256, taken as they are) -> (len, 4) uint64 little-endian words"""
    a = np.zeros((len(vals), 4), np.uint64)
    for i, v in enumerate(vals):
        for k in range(4):
            a[i, k] = (v >> (64 * k)) & 0xFFFFFFFFFFFFFFFF
    return a


def pack_words(vals):
    """words_of for long lists: through int.to_bytes and one np.frombuffer"""
    return np.frombuffer(b"".join(v.to_bytes(32, "little") for v in vals), dtype="<u8").reshape(len(vals), 4)


def geometric_words(c, a, n_bits):
    """(2^n_bits, 4) Montgomery words of the column x_j = c a^j: one product per element, starting from the Montgomery form of c"""
    vals, v = [], to_mont(c)
    for _ in range(1 << n_bits):
        vals.append(v)
        v = v * a % R
    return pack_words(vals)


def ints_of(words):
    wd = np.asarray(words, dtype=np.uint64).reshape(-1, 4)
    return [sum(int(x) << (64 * k) for k, x in enumerate(row)) for row in wd]


def matrix_words(cols):
    """cols[i][j] = normal-form value of polynomial i at row j -> (rows, nPols, 4) Montgomery words"""
    n_pols, rows = len(cols), len(cols[0])
    return words_of([to_mont(cols[i][j]) for j in range(rows) for i in range(n_pols)]).reshape(rows, n_pols, 4)


def matrix_cols(words):
    """(rows, nPols, 4) Montgomery words -> cols[i][j] normal form"""
    wd = np.asarray(words, dtype=np.uint64)
    rows, n_pols = wd.shape[0], wd.shape[1]
    flat = [from_mont(v) for v in ints_of(wd)]
    return [[flat[j * n_pols + i] for j in range(rows)] for i in range(n_pols)]


def apply_cols(fn, words):
    """the transform fn (list -> list) applied to every column of a Montgomery-word matrix"""
    return matrix_words([fn(c) for c in matrix_cols(words)])
