"""Chosen Fq coordinates for the G1 MSM tests.  The xyzz formulas of bn_g1.cuh (madd, add, dbl with a = 0) never use the curve constant
b and the MSM never checks that a base is on the curve, so any canonical pair (x, y) != (0, 0) is a point of y^2 = x^3 + b' with
b' = y^2 - x^3, on which the kernels compute the true group law: the stored (Montgomery) bytes of a base can be chosen freely, and
bn128_g1_ref's add / mul, equally b-free, check the result.  The order of such a curve is not r: a scalar acts as the integer it is.
(x, 0) has order 2 and (0, y) has order 3 on their curves."""
import random

import numpy as np

import bn128_g1_ref as ref
from bn128_g1_ref import MONT, Q

MONT_INV = pow(MONT, -1, Q)
Q_TOP = Q >> 224                                     # q's top 32-bit limb
ONES7 = ((Q_TOP - 1) << 224) | ((1 << 224) - 1)      # seven limbs of ones under q's top limb minus one
X = random.Random(0xF9).randrange(1 << 200, Q - 1)

NAMED = [
    ("1", 1), ("2", 2), ("q-1", Q - 1), ("q-2", Q - 2),
    ("(q-1)/2", (Q - 1) // 2), ("(q+1)/2", (Q + 1) // 2),
    ("2^256 mod q", MONT % Q), ("2^512 mod q", MONT * MONT % Q),
    ("ones7", ONES7), ("q-ones7", Q - ONES7),
    ("2^224", 1 << 224), ("2^224-1", (1 << 224) - 1), ("2^32", 1 << 32), ("2^32-1", (1 << 32) - 1),
    ("X", X), ("X+1", X + 1),
]
NAMES = [name for name, _ in NAMED]
STORED = [v for _, v in NAMED]
BY_NAME = dict(NAMED)
Y_SUBSET = [BY_NAME[k] for k in ("1", "q-1", "(q+1)/2", "2^256 mod q", "ones7", "2^224", "X")]     # section a's stored y


def limbs(v):
    return [(v >> (32 * i)) & 0xffffffff for i in range(8)]


def value_of(stored):
    """the field element whose Montgomery form is `stored`"""
    return stored * MONT_INV % Q


def point_of_stored(sx, sy):
    """the checker's point (values) of a stored pair; (0, 0) is infinity"""
    return None if sx == 0 and sy == 0 else (value_of(sx), value_of(sy))


def stored_point_words(pairs):
    """(n, 8) uint64: the stored integers (sx, sy) written as they are, no conversion; None is infinity (all zero)"""
    flat = []
    for p in pairs:
        flat += [0, 0] if p is None else [p[0], p[1]]
    assert all(0 <= v < Q for v in flat), "a stored coordinate must be canonical"
    return ref._words(flat, 8) if pairs else np.zeros((0, 8), np.uint64)


def stored_of(point):
    """the stored pair of a checker point"""
    return None if point is None else (point[0] * MONT % Q, point[1] * MONT % Q)


def chord_pairs():
    """section b: ((sx1, sy1), (sx2, sy2)) for every ordered pair x1 != x2 of STORED, y cycling through STORED with two strides"""
    n, out = len(STORED), []
    for i in range(n):
        for j in range(n):
            if i != j:
                out.append(((STORED[i], STORED[(3 * i + j) % n]), (STORED[j], STORED[(i + 5 * j + 7) % n])))
    return out


def curve_b(p):
    """b' of the curve y^2 = x^3 + b' through p"""
    return (p[1] * p[1] - p[0] * p[0] * p[0]) % Q


def independent_point(p, seed=1):
    """another point of p's curve, found by a square root (q = 3 mod 4), not a multiple of p in general"""
    b, x = curve_b(p), seed
    while True:
        rhs = (x * x * x + b) % Q
        y = pow(rhs, (Q + 1) // 4, Q)
        if y and y * y % Q == rhs and x != p[0]:
            return (x, y)
        x += 1
