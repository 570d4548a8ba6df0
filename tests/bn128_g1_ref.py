"""Checker for the BN254 G1 multi-scalar multiplication (pil2gl_bn128_g1_msm), in Python integers, written from the definitions: the
curve y^2 = x^3 + 3 over Fq, generator (1, 2) of prime order r, ffjavascript's byte formats (affine points of 2 x 32 little-endian bytes
in Fq Montgomery form, infinity all zero; scalars of 32 bytes, Fr Montgomery or normal form).  No reference-written fixture exists for
this operation; what pins it is the group law itself.  A point is None (infinity) or (x, y); a Jacobian point is (X, Y, Z)."""
import random

import numpy as np

Q = 21888242871839275222246405745257275088696311157297823662689037894645226208583
R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
G = (1, 2)
MONT = 1 << 256


def on_curve(p):
    return p is None or (p[1] * p[1] - p[0] * p[0] * p[0] - 3) % Q == 0


def neg(p):
    return None if p is None else (p[0], (Q - p[1]) % Q)


def add(p, q):
    if p is None:
        return q
    if q is None:
        return p
    if p[0] == q[0]:
        if (p[1] + q[1]) % Q == 0:
            return None
        lam = 3 * p[0] * p[0] * pow(2 * p[1], -1, Q) % Q
    else:
        lam = (q[1] - p[1]) * pow(q[0] - p[0], -1, Q) % Q
    x = (lam * lam - p[0] - q[0]) % Q
    return (x, (lam * (p[0] - x) - p[1]) % Q)


def jac_double(p):
    X, Y, Z = p
    if Z == 0 or Y == 0:
        return (1, 1, 0)
    a, b = X * X % Q, Y * Y % Q
    c = b * b % Q
    d = 2 * ((X + b) * (X + b) - a - c) % Q
    e = 3 * a % Q
    x3 = (e * e - 2 * d) % Q
    return (x3, (e * (d - x3) - 8 * c) % Q, 2 * Y * Z % Q)


def jac_add(p, q):
    if p[2] == 0:
        return q
    if q[2] == 0:
        return p
    z1z1, z2z2 = p[2] * p[2] % Q, q[2] * q[2] % Q
    u1, u2 = p[0] * z2z2 % Q, q[0] * z1z1 % Q
    s1, s2 = p[1] * q[2] * z2z2 % Q, q[1] * p[2] * z1z1 % Q
    if u1 == u2:
        return jac_double(p) if s1 == s2 else (1, 1, 0)
    h, r = (u2 - u1) % Q, (s2 - s1) % Q
    hh = h * h % Q
    hhh, v = h * hh % Q, u1 * hh % Q
    x3 = (r * r - hhh - 2 * v) % Q
    return (x3, (r * (v - x3) - s1 * hhh) % Q, p[2] * q[2] * h % Q)


def to_jac(p):
    return (1, 1, 0) if p is None else (p[0], p[1], 1)


def to_affine(p):
    if p[2] == 0:
        return None
    zi = pow(p[2], -1, Q)
    return (p[0] * zi * zi % Q, p[1] * zi * zi * zi % Q)


def batch_to_affine(ps):
    """Jacobian points -> affine, with one inversion for the whole list"""
    pref, acc = [], 1
    for p in ps:
        pref.append(acc)
        if p[2]:
            acc = acc * p[2] % Q
    inv, out = pow(acc, -1, Q), [None] * len(ps)
    for i in range(len(ps) - 1, -1, -1):
        X, Y, Z = ps[i]
        if Z:
            zi = inv * pref[i] % Q
            inv = inv * Z % Q
            out[i] = (X * zi * zi % Q, Y * zi * zi * zi % Q)
    return out


def mul(k, p):
    """k p by double-and-add (k any non-negative integer)"""
    acc, base = (1, 1, 0), to_jac(p)
    while k:
        if k & 1:
            acc = jac_add(acc, base)
        base = jac_double(base)
        k >>= 1
    return to_affine(acc)


def msm(scalars, points):
    """sum s_i P_i, one double-and-add per point"""
    acc = None
    for s, p in zip(scalars, points):
        acc = add(acc, mul(s, p))
    return acc


def known_log_bases(n, seed, a=None, d=None):
    """-> (points, logs): P_i = k_i G with k_i = a + j d for a seeded permutation j of 0..n-1 (repeated addition of d G in Jacobian form,
    one batch inversion), so that sum s_i P_i = (sum s_i k_i mod r) G"""
    rng = random.Random(seed)
    a = rng.randrange(1, R) if a is None else a
    d = rng.randrange(1, R) if d is None else d
    step, cur, jac = to_jac(mul(d, G)), to_jac(mul(a, G)), []
    for _ in range(n):
        jac.append(cur)
        cur = jac_add(cur, step)
    pts = batch_to_affine(jac)
    order = list(range(n))
    rng.shuffle(order)
    return [pts[j] for j in order], [(a + j * d) % R for j in order]


def expected_from_logs(scalars, logs):
    return mul(sum(s * k for s, k in zip(scalars, logs)) % R, G)


# ---- byte formats --------------------------------------------------------------------------------------------------------------------
def _words(vals, width):
    raw = b"".join(int(v).to_bytes(32, "little") for v in vals)
    return np.frombuffer(raw, dtype="<u8").reshape(-1, width).copy()


def point_words(points):
    """(n, 8) uint64: x then y in Fq Montgomery form; infinity is all zero"""
    flat = []
    for p in points:
        flat += [0, 0] if p is None else [p[0] * MONT % Q, p[1] * MONT % Q]
    return _words(flat, 8) if points else np.zeros((0, 8), np.uint64)


def point_of(words):
    b = np.ascontiguousarray(words, dtype="<u8").reshape(8).tobytes()
    x, y = int.from_bytes(b[:32], "little"), int.from_bytes(b[32:], "little")
    assert x < Q and y < Q, "coordinate not canonical"
    minv = pow(MONT, -1, Q)
    return None if x == 0 and y == 0 else (x * minv % Q, y * minv % Q)


def scalar_words(scalars, montgomery=True):
    """(n, 4) uint64: Fr Montgomery words, or the scalars as they are"""
    return _words([s * MONT % R if montgomery else s for s in scalars], 4) if scalars else np.zeros((0, 4), np.uint64)


# ---- the signed digits and the plan, from their definitions --------------------------------------------------------------------------
def digits(s, c):
    """windows of c bits from the least significant; a window's value above 2^(c-1) becomes value - 2^c and carries one"""
    out, carry = [], 0
    for _ in range(-(-255 // c)):
        v = (s & ((1 << c) - 1)) + carry
        s >>= c
        carry = 1 if v > (1 << (c - 1)) else 0
        out.append(v - (carry << c))
    assert s == 0 and carry == 0
    return out


def edge_scalars(c):
    """the recoding's edges for windows of c bits, each below 2^254: 0, 1, r-1, the three values around the sign switch in every window
    position, every window at 2^(c-1) and at 2^(c-1)+1 (the carry ripples to the top), 2^253"""
    n_w, half = -(-255 // c), 1 << (c - 1)
    out = [0, 1, R - 1, 1 << 253]
    for w in range(n_w):
        out += [v << (c * w) for v in (half - 1, half, (1 << c) - 1)]
    out += [sum(v << (c * w) for w in range(n_w)) for v in (half, half + 1)]
    return sorted({s & ((1 << 254) - 1) for s in out})


def plan(n):
    n = max(n, 1)
    c = min(max(n.bit_length() - 1 - 3, 4), 16)
    n_w = -(-255 // c)
    g = 1
    while 2 * g <= min(max(8 * n, 1 << 19), 1 << 30) // n and 2 * g <= 64:
        g *= 2
    return c, n_w, 1 << (c - 1), min(g, n_w)


def scratch_bound(n):
    return 4 * min(max(8 * n, 1 << 19), 1 << 30) + (96 << 20)
