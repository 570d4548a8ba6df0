"""The grand product of a permutation or a connection of include/pil2gl.h over Python integers, from the statement and sharing no code with
the library:

    z[0] = 1,   z[i] = z[i-1] R[i-1]
    R[i]   = prod_{u: den_u = 0} D_u[i]  /  prod_{u: den_u = 1} D_u[i]
    D_u[i] = B_u[i] + idCoef_u id_u[i] + gamma
    B_u[i] = H_u[i]   or   (H_u[i] - beta) sel_u[i] + beta   when the term has a selector
    H_u[i] = (..(v_0 alpha + v_1) alpha .. ) alpha + v_{k-1}

A zero denominator product makes R[i] = 0 (gprod's convention).  The fields are logup_sum_ref's: over Goldilocks alpha, beta, gamma, idCoef
and z are elements of the cubic extension and everything else is in the base field; over Fr everything is a PLAIN integer mod r.  A term
is (tuples, sel, den, ids, id_coef): tuples n rows of k integers, sel n integers or None, den 0 / 1, ids n integers or None, id_coef an
extension element (ignored without ids).  `period`: the inputs repeat with that period, so only `period` rows are computed and inverted."""
from logup_sum_ref import FIELDS
from logup_sum_ref import plan as _logup_plan


def _neg(F, a):
    return tuple((F.q - x) % F.q for x in a) if isinstance(a, tuple) else (F.q - a) % F.q


def factor(F, term, alpha, beta, gamma, i):
    """D_u[i] of one term"""
    tuples, sel, _, ids, id_coef = term
    h = F.zero
    for v in tuples[i]:
        h = F.add(F.mul(h, alpha), F.base(v))
    if sel is not None:
        h = F.add(F.mul(F.add(h, _neg(F, beta)), F.base(sel[i])), beta)
    if ids is not None:
        h = F.add(h, F.mul(F.ext(id_coef), F.base(ids[i])))
    return F.add(h, gamma)


def num_den(field, terms, alpha, beta, gamma, n, period=None):
    """-> the two materialised product columns (num, den), `period` rows at most"""
    F = FIELDS[field]
    alpha, beta, gamma = F.ext(alpha), F.ext(beta), F.ext(gamma)
    per = n if period is None else min(period, n)
    num, den = [], []
    for i in range(per):
        N, D = F.one, F.one
        for term in terms:
            d = factor(F, term, alpha, beta, gamma, i)
            if term[2]:
                D = F.mul(D, d)
            else:
                N = F.mul(N, d)
        num.append(N)
        den.append(D)
    return num, den


def ratios(field, terms, alpha, beta, gamma, n, period=None):
    F = FIELDS[field]
    num, den = num_den(field, terms, alpha, beta, gamma, n, period)
    return [F.zero if d == F.zero else F.mul(N, F.inv(d)) for N, d in zip(num, den)]


def grand_prod(field, terms, alpha, beta, gamma, n, period=None):
    """-> z as n field elements (triples over Goldilocks, plain integers over Fr)"""
    F = FIELDS[field]
    r = ratios(field, terms, alpha, beta, gamma, n, period)
    z, acc = [], F.one
    for i in range(n):
        z.append(acc)
        acc = F.mul(acc, r[i % len(r)])
    return z


def closing(field, terms, alpha, beta, gamma, n):
    """z[n-1] R[n-1]: 1 exactly when the whole product closes"""
    F = FIELDS[field]
    z = grand_prod(field, terms, alpha, beta, gamma, n)
    return F.mul(z[n - 1], ratios(field, terms, alpha, beta, gamma, n)[n - 1])


def plan(n, field):
    """the numbers of pil2gl_grand_prod_plan, restated: logup_sum's geometry and bytes (the same passes with a product in them)"""
    return _logup_plan(n, 1, field)
