"""The checker of the BN254 Fr sparse products, scaled sums and degree (a plain module: tests/test_bn128_polymul_cpu.py,
tests/test_gpu_bn128_polymul.py and the Node test's expectations build on it), in Python integers from the definition

    acc[i] <- (s * acc[i] + sum_j m[j] * src[i - e[j]]) mod r      0 <= i < nAcc,   src[x] = 0 for x < 0 or x >= nSrc

with s = None meaning "acc is not read".  The form is linear in acc and src, so it holds unchanged on Montgomery representations
x * 2^256 with s and m as plain integers: the tests run it on the very integers the device words spell.  Nothing reference-written
exists for these operations (the reference tree vendors neither shplonkjs nor ffjavascript), so the checker is checked by evaluating both
sides of acc' = s acc + M src at points, and zerofier_terms by its roots (tests/test_bn128_polymul_cpu.py)."""
from bn128_poly_ref import R, MONT, MONT_INV, mont, words, ints, rand_elems, evaluate       # noqa: F401  (one set of helpers for both checkers)

NONE = (1 << 64) - 1
POISON = (1 << 256) - 1                              # 32 bytes of 0xFF: not canonical


def fma(acc, src, terms, s=None, n_acc=None, n_src=None):
    """terms = [(m, e)], plain integers; acc, src lists of integers -> the new acc[0..n_acc) (a new list)"""
    n_acc = len(acc) if n_acc is None else n_acc
    n_src = len(src) if n_src is None else n_src
    out = []
    for i in range(n_acc):
        v = 0 if s is None else s * acc[i]
        for m, e in terms:
            if 0 <= i - e < n_src:
                v += m * src[i - e]
        out.append(v % R)
    return out


def fma_column(buf, col_a, stride_a, n_acc, src_buf, col_s, stride_s, n_src, terms, s=None):
    """the same on columns: element i of acc is buf[col_a + i * stride_a], of src src_buf[col_s + i * stride_s] -> the whole new buf"""
    acc = [buf[col_a + i * stride_a] for i in range(n_acc)]
    src = [src_buf[col_s + i * stride_s] for i in range(n_src)]
    new = fma(acc, src, terms, s)
    out = list(buf)
    for i, v in enumerate(new):
        out[col_a + i * stride_a] = v
    return out


def degree(c):
    """the largest i with c[i] != 0, NONE (2^64 - 1) for the zero polynomial"""
    for i in range(len(c) - 1, -1, -1):
        if c[i]:
            return i
    return NONE


def zerofier_terms(factors):
    """prod_j (x^k_j - beta_j), factors = [(k, beta)] plain integers -> [(coef, exp)] ascending, zero coefficients dropped"""
    poly = {0: 1}
    for k, beta in factors:
        nxt = {}
        for e, c in poly.items():
            nxt[e + k] = (nxt.get(e + k, 0) + c) % R
            nxt[e] = (nxt.get(e, 0) - beta * c) % R
        poly = {e: c for e, c in nxt.items() if c}
    return [(poly[e], e) for e in sorted(poly)]


def eval_terms(terms, z):
    return sum(m * pow(z, e, R) for m, e in terms) % R


def dense(terms):
    out = [0] * (terms[-1][1] + 1 if terms else 0)
    for m, e in terms:
        out[e] = m
    return out


def poly_mul(a, b):
    """schoolbook, for the composition test's small factors"""
    out = [0] * (len(a) + len(b) - 1 if a and b else 0)
    for i, x in enumerate(a):
        if x:
            for j, y in enumerate(b):
                out[i + j] = (out[i + j] + x * y) % R
    return out


def interpolate(points, values):
    """the coefficients (plain integers) of the polynomial of degree < len(points) through (points[i], values[i]): Lagrange"""
    n = len(points)
    out = [0] * n
    for i in range(n):
        num, den = [1], 1
        for j in range(n):
            if j != i:
                num = poly_mul(num, [-points[j] % R, 1])
                den = den * (points[i] - points[j]) % R
        c = values[i] * pow(den, -1, R) % R
        for d, v in enumerate(num):
            out[d] = (out[d] + c * v) % R
    return out
