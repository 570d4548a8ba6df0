"""The lookup grand sum of include/pil2gl.h over Python integers, from the statement and sharing no code with the library:

    s[i] = s[i-1] + sum_{u < nTerms} coef_u w_u[i] / D_u[i]            s[-1] = 0
    D_u[i] = ((..((v_0 alpha + v_1) alpha + v_2).. + v_{k-1}) alpha + busId_u) + beta

A zero D_u[i] adds 0.  Over Goldilocks alpha, beta and s are elements of the cubic extension (hints_ref.mul3 / inv3), everything else is in
the base field; over Fr everything is a PLAIN integer mod r (the tests convert Montgomery patterns with bn128_hints_ref.mont / unmont: the
statement is algebra over field values, so it commutes with that bijection).  A term is (tuples, w, coef, bus_id): tuples n rows of k
integers, w n integers or None (then 1).  Every integer is taken mod the base modulus first.  `period`: the inputs repeat with that period, so
only `period` rows are inverted and the rest only added (the deep-scan tests).  gsum_col is the same sum for one ready fraction a row."""
from hints_ref import P, add3, mul3, inv3
from bn128_hints_ref import R


class Gl3:
    """the cubic extension of Goldilocks; base-field values come in as integers"""
    q = P
    zero, one = (0, 0, 0), (1, 0, 0)
    add = staticmethod(add3)
    mul = staticmethod(mul3)
    inv = staticmethod(inv3)

    @staticmethod
    def base(v):
        return (v % P, 0, 0)

    @staticmethod
    def ext(v):
        return tuple(int(x) % P for x in v)


class Fr:
    q = R
    zero, one = 0, 1
    add = staticmethod(lambda a, b: (a + b) % R)
    mul = staticmethod(lambda a, b: a * b % R)
    inv = staticmethod(lambda a: pow(a, R - 2, R))
    base = staticmethod(lambda v: v % R)
    ext = staticmethod(lambda v: int(v) % R)


FIELDS = {"gl": Gl3, "bn128": Fr}


def denominator(F, row, alpha, beta, bus_id):
    """D of one term at one row: the tuple Horner-compressed with alpha, first column highest, the bus id the last Horner term, + beta"""
    acc = F.zero
    for v in row:
        acc = F.add(F.mul(acc, alpha), F.base(v))
    return F.add(F.add(F.mul(acc, alpha), F.base(bus_id)), beta)


def row_fraction(F, terms, alpha, beta, i):
    """row i as (N, D, ratio): D = the product of the non-zero D_u, N = sum coef_u w_u prod_{v != u} D_v over them, ratio = sum of the terms"""
    ds, cs = [], []
    for tuples, w, coef, bus in terms:
        d = denominator(F, tuples[i], alpha, beta, bus)
        if d != F.zero:
            ds.append(d)
            cs.append(F.base(coef * (1 if w is None else w[i])))
    N, D, ratio = F.zero, F.one, F.zero
    for u, (d, c) in enumerate(zip(ds, cs)):
        others = F.one
        for v, dv in enumerate(ds):
            if v != u:
                others = F.mul(others, dv)
        N = F.add(N, F.mul(c, others))
        D = F.mul(D, d)
        ratio = F.add(ratio, F.mul(c, F.inv(d)))
    return N, D, ratio


def logup_sum(field, terms, alpha, beta, n, period=None):
    """-> s as n field elements (triples over Goldilocks, plain integers over Fr)"""
    F = FIELDS[field]
    alpha, beta = F.ext(alpha), F.ext(beta)
    per = n if period is None else min(period, n)
    ratios = [row_fraction(F, terms, alpha, beta, i)[2] for i in range(per)]
    s, acc = [], F.zero
    for i in range(n):
        acc = F.add(acc, ratios[i % per])
        s.append(acc)
    return s


def gsum_col(field, num, den, period=None):
    """num, den: n field elements each (triples / plain integers) -> s[i] = s[i-1] + num[i] / den[i], a zero denominator adding 0"""
    F = FIELDS[field]
    n = len(den)
    per = n if period is None else min(period, n)
    ratios = [F.mul(F.ext(num[i]), F.inv(F.ext(den[i]))) if F.ext(den[i]) != F.zero else F.zero for i in range(per)]
    s, acc = [], F.zero
    for i in range(n):
        acc = F.add(acc, ratios[i % per])
        s.append(acc)
    return s


def plan(n, n_terms, field):
    """the numbers of pil2gl_logup_sum_plan, restated: (threads, items, blocks, launches, depth, width), working bytes"""
    if field == "gl":
        nb = -(-n // 2048)
        return (256, 8, nb, 3 if n else 0, -(-nb // 256), 3), 24 * n + 24 * nb
    levels, cur, elems = 0, n, 0
    while True:                                       # csrc/bn_scan_plan.h: segments of >= 16 rows, at most 2^17, until <= 64 are left
        if levels:
            elems += 2 * cur
        levels += 1
        if cur <= 64:
            break
        want = min(1 << 17, -(-cur // 16))
        L = -(-cur // want)
        cur = -(-cur // L)
    blocks = min(2048, max(1, -(-n // 256))) if n else 0
    return (256, 1, blocks, 4 * levels - 1 if n else 0, levels, 1), (32 * elems + 64 * n) if n else 0
