"""Checker for the BN254 G1 stage commit (pil2gl_bn128_g1_commit): the packed polynomials of a batch, the batch planner and the lane
mapping, in Python integers, written from their definitions.  A packed polynomial is fflonk's CPolynomial as the fflonk paper and snarkjs
state it, f(X) = sum_j X^j p_j(X^m): coefficient i sits in slot j = i mod m and row t = i div m of a row-major matrix.  A polynomial is
(first, rows, slots) with None for an empty slot; a matrix is a flat list of scalars (Python ints), row_stride per row."""
import bn128_g1_ref as ref
from bn128_g1_ref import R

EMPTY = 0xFFFFFFFF


def elements(poly, row_stride):
    """the element offset of every coefficient, None where the slot is empty"""
    first, rows, slots = poly
    m = len(slots)
    return [None if slots[i % m] is None else first + (i // m) * row_stride + slots[i % m] for i in range(m * rows)]


def coefficients(matrix, poly, row_stride):
    return [0 if e is None else matrix[e] for e in elements(poly, row_stride)]


def expected(matrix, poly, row_stride, logs, points=None):
    """the commitment of one packed polynomial over known-log bases; a base given as None in `points` is the point at infinity"""
    coefs = coefficients(matrix, poly, row_stride)
    if points is not None:
        coefs = [0 if points[i] is None else c for i, c in enumerate(coefs)]
    return ref.expected_from_logs(coefs, logs[:len(coefs)])


def locate(polys, lane):
    """lane of the whole batch -> (k, i): the polynomials' coefficients one polynomial after the other"""
    for k, (first, rows, slots) in enumerate(polys):
        n = rows * len(slots)
        if lane < n:
            return k, lane
        lane -= n
    return None


# ---- the batch plan, from its definition ---------------------------------------------------------------------------------------------
BUCKET_BUDGET, PASS_CELLS = 9 << 19, 1 << 18


def batch_plan(counts):
    K, total, n_max = len(counts), max(sum(counts), 1), max(max(counts), 1)
    c = min(max(n_max.bit_length() - 1 - 3, 4), 16)
    while c > 4 and K * -(-255 // c) * (1 << (c - 1)) > BUCKET_BUDGET:
        c -= 1
    n_w, nbw = -(-255 // c), 1 << (c - 1)
    g = 1
    while 2 * g <= min(max(8 * total, 1 << 19), 1 << 30) // total and 2 * g <= 64 and K * min(2 * g, n_w) * nbw <= PASS_CELLS:
        g *= 2
    return c, n_w, nbw, min(g, n_w)


def batch_scratch_bound(K, total):
    return 4 * min(max(8 * total, 1 << 19), 1 << 30) + (96 << 20) * min(K, 9)
