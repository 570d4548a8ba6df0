"""The range-check grand sum of include/pil2gl.h over Python integers, from the statement and sharing no code with the library:

    s[i] = s[i-1] + sum_{u < nF} coef_u w_u[i] / D_u[i]  +  sum_{r < nR} coefR_r [row0_r <= i < row0_r + size_r] m_r[i] / E_r[i]      s[-1] = 0
    D_u[i]  logup_sum_ref.denominator
    E_r[i] = field(lo_r + (i - row0_r)) alpha + busId_r + beta

A zero D_u[i] or E_r[i] adds 0.  Fields, f terms (tuples, w, coef, bus_id) and challenges are logup_sum_ref's: over Goldilocks alpha, beta and
s are elements of the cubic extension, over Fr everything is a PLAIN integer mod r.  A range is (m, lo, size, row0, coef, bus_id): m a
sequence of n integers, or a function of the row, consulted ONLY inside the window (the tests put None outside to prove it); lo a signed
integer.  `period`: the f terms repeat with that period, so only `period` of their rows are inverted; a range is inverted at every row of its
window (its denominator is never periodic), so the deep tests keep the windows short.
materialise() turns ranges into logup_sum_ref terms: the statement's promise."""
import logup_sum_ref as lref

FIELDS = lref.FIELDS


def in_window(rng, i):
    return rng[3] <= i < rng[3] + rng[2]


def m_at(m, i):
    return m(i) if callable(m) else m[i]


def range_denominator(F, rng, alpha, beta, i):
    """E of one range at a row of its window"""
    _, lo, _, row0, _, bus = rng
    return F.add(F.add(F.mul(alpha, F.base(lo + (i - row0))), F.base(bus)), beta)


def row_parts(F, terms, ranges, alpha, beta, i):
    """the non-zero denominators of row i and their numerators, f terms first"""
    ds, cs = [], []
    for tuples, w, coef, bus in terms:
        d = lref.denominator(F, tuples[i], alpha, beta, bus)
        if d != F.zero:
            ds.append(d)
            cs.append(F.base(coef * (1 if w is None else w[i])))
    for rng in ranges:
        if not in_window(rng, i):
            continue
        d = range_denominator(F, rng, alpha, beta, i)
        if d != F.zero:
            ds.append(d)
            cs.append(F.base(rng[4] * m_at(rng[0], i)))
    return ds, cs


def row_fraction(F, terms, ranges, alpha, beta, i):
    """row i as (N, D, ratio): D = the product of the non-zero denominators, N = sum c_u prod_{v != u} d_v over them, ratio = the row's sum"""
    ds, cs = row_parts(F, terms, ranges, alpha, beta, i)
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


def range_sum(field, terms, ranges, alpha, beta, n, period=None):
    """-> s as n field elements (triples over Goldilocks, plain integers over Fr)"""
    F = FIELDS[field]
    alpha, beta = F.ext(alpha), F.ext(beta)
    per = n if period is None else min(period, n)
    f_ratio = [row_fraction(F, terms, [], alpha, beta, i)[2] for i in range(per)] if terms else None
    extra = {}
    for rng in ranges:
        for i in range(rng[3], rng[3] + rng[2]):
            extra[i] = F.add(extra.get(i, F.zero), row_fraction(F, [], [rng], alpha, beta, i)[2])
    s, acc = [], F.zero
    for i in range(n):
        if f_ratio is not None:
            acc = F.add(acc, f_ratio[i % per])
        if i in extra:
            acc = F.add(acc, extra[i])
        s.append(acc)
    return s


def materialise(field, ranges, n):
    """each range as the k = 1 term of logup_sum_ref that the statement promises it equals: the tuple column
    t[i] = field(lo + clamp(i - row0, 0, size - 1)), the numerator column m zeroed outside the window, the same coef and bus id"""
    q = FIELDS[field].q
    terms = []
    for rng in ranges:
        m, lo, size, row0, coef, bus = rng
        t = [[(lo + min(max(i - row0, 0), size - 1)) % q] for i in range(n)]
        w = [m_at(m, i) if in_window(rng, i) else 0 for i in range(n)]
        terms.append((t, w, coef, bus))
    return terms


def plan(n, n_f, n_r, field):
    """the numbers of pil2gl_range_sum_plan, restated: logup_sum's for the same n, whatever n_f and n_r"""
    return lref.plan(n, n_f + n_r, field)
