"""The checker of the BN254 Fr polynomial division / evaluation (a plain module: tests/test_bn128_poly_cpu.py, tests/test_gpu_bn128_poly.py
and the Node test's expectations build on it), in Python integers from the definition

    d[i] = (c[i] + beta * d[i + k]) mod r,  d[j] = 0 for j >= n          (from the top)

d[k..n) is the quotient of c by x^k - beta (coefficient m at position m + k), d[0..k) the remainder; eval is Horner.  The recurrence is
linear in c, so it holds unchanged on Montgomery representations c * 2^256 with beta as a plain integer: the tests run it on the very
integers the device words spell.  mul_back multiplies quotient * (x^k - beta) + remainder out again, which checks the checker."""
import random

import numpy as np

R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
MONT = (1 << 256) % R
MONT_INV = pow(MONT, -1, R)


def scan(c, k, beta):
    d = list(c)
    for i in range(len(d) - k - 1, -1, -1):
        d[i] = (d[i] + beta * d[i + k]) % R
    return d


def evaluate(c, z):
    acc = 0
    for v in reversed(c):
        acc = (acc * z + v) % R
    return acc


def divmod_xk(c, k, beta):
    """(quotient, remainder) of c by x^k - beta"""
    d = scan(c, k, beta)
    return d[k:], d[:k]


def mul_back(q, rem, k, beta):
    """q * (x^k - beta) + rem, schoolbook, len(q) + k coefficients (len(rem) if q is empty)"""
    out = [0] * max(len(q) + k if q else 0, len(rem))
    for i, v in enumerate(rem):
        out[i] = v % R
    for m, v in enumerate(q):
        out[m + k] = (out[m + k] + v) % R
        out[m] = (out[m] - beta * v) % R
    return out


def divzh_low_to_high(c, N):
    """the reference's divZh recurrence, from the low end: q[i] = -c[i] for i < N, then q[i] = q[i - N] - c[i]; the top N it leaves
    must be zero ("Polynomial is not divisible" otherwise) -> (quotient of len(c) - N coefficients, divisible)"""
    q = [0] * len(c)
    for i in range(len(c)):
        q[i] = ((q[i - N] if i >= N else 0) - c[i]) % R
    return q[:len(c) - N], not any(q[len(c) - N:])


def mont(v):
    return v * MONT % R


def words(vals):
    """integers below 2^256 -> (n, 4) uint64, little-endian words, as they are"""
    raw = b"".join(int(v).to_bytes(32, "little") for v in vals)
    return np.frombuffer(raw, dtype=np.uint64).reshape(-1, 4).copy()


def ints(w):
    raw = np.ascontiguousarray(w, dtype=np.uint64).reshape(-1, 4).tobytes()
    return [int.from_bytes(raw[o:o + 32], "little") for o in range(0, len(raw), 32)]


def rand_elems(n, seed):
    """n canonical values over the whole range: 254 random bits, less r where that is not below r (fast enough for millions)"""
    raw = np.random.default_rng(seed).bytes(32 * n)
    mask = (1 << 254) - 1
    vals = (int.from_bytes(raw[o:o + 32], "little") & mask for o in range(0, 32 * n, 32))
    return [v - R if v >= R else v for v in vals]


def limb_pattern_elems(n, seed):
    """canonical values whose 32-bit limbs are 0 or 2^32 - 1 (the top limb 0 so that the value stays below r), cycled with 0 and r - 1"""
    rng = random.Random(seed)
    out = []
    for i in range(n):
        if i % 7 == 5:
            out.append(0)
        elif i % 7 == 6:
            out.append(R - 1)
        else:
            out.append(sum((0xFFFFFFFF if rng.getrandbits(1) else 0) << (32 * j) for j in range(7)))
    return out
