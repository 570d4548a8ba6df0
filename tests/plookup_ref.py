"""The plookup argument of include/pil2gl.h (pil1's grandProductPlookup.js) over Python integers, from the statement and sharing no code with
the library:

    H_t[i] = (..(t_0 alpha + t_1) alpha ..) alpha + t_{kT-1}
    T[i]   = H_t[i]   or   (H_t[i] - beta) selT[i] + beta        with a selector: its field value
    F[i]   = H_f[i]   or   (H_f[i] - T[i]) selF[i] + T[i]        blended towards T of the same row
    g      = gamma (1 + delta)
    num[i] = (F[i] + gamma) (T[i] + delta T[(i+1) mod n] + g) (1 + delta)
    den[i] = (h1[i] + delta h2[i] + g) (h2[i] + delta h1[(i+1) mod n] + g)
    z[0] = 1,  z[i] = z[i-1] num[i-1] / den[i-1]                  a zero den[i-1] makes the ratio 0 (gprod's convention)

The fields are logup_sum_ref's: over Goldilocks the challenges, F, T (and h when it is an extension column) and z are elements of the cubic
extension x^3 = x + 1 and the trace is in the base field; over Fr everything is a PLAIN integer mod r (the tests convert Montgomery
patterns at the edge).  A side is (tuples, sel): tuples n rows of k integers, sel n integers or None.  h1 and h2 are n field elements as
elem() makes them.  valid_lookup() builds sides whose selected f tuples are all taken from selected t rows, and h1, h2 by the h1h2
checkers of the field on the folded F and T."""
from logup_sum_ref import FIELDS
import hints_ref
import bn128_h1h2_ref


def _neg(F, a):
    return tuple((F.q - x) % F.q for x in a) if isinstance(a, tuple) else (F.q - a) % F.q


def elem(field, v):
    """an h element as the checker's value: an integer (a base column) or a triple over Goldilocks, an integer over Fr"""
    F = FIELDS[field]
    return F.ext(v) if field == "bn128" or isinstance(v, (tuple, list)) else F.base(v)


def horner(F, row, alpha):
    h = F.zero
    for v in row:
        h = F.add(F.mul(h, alpha), F.base(v))
    return h


def fold(field, f, t, alpha, beta):
    """-> (F, T), n field elements each"""
    Fd = FIELDS[field]
    alpha, beta = Fd.ext(alpha), Fd.ext(beta)

    def blend(h, s, to):
        return Fd.add(Fd.mul(Fd.add(h, _neg(Fd, to)), Fd.base(s)), to)

    n = len(t[0])
    T = [horner(Fd, t[0][i], alpha) for i in range(n)]
    if t[1] is not None:
        T = [blend(T[i], t[1][i], beta) for i in range(n)]
    Fx = [horner(Fd, f[0][i], alpha) for i in range(n)]
    if f[1] is not None:
        Fx = [blend(Fx[i], f[1][i], T[i]) for i in range(n)]
    return Fx, T


def num_den(field, f, t, h1, h2, alpha, beta, gamma, delta):
    """-> the two materialised columns (num, den) of n field elements"""
    Fd = FIELDS[field]
    Fx, T = fold(field, f, t, alpha, beta)
    gamma, delta = Fd.ext(gamma), Fd.ext(delta)
    opd = Fd.add(Fd.one, delta)
    g = Fd.mul(gamma, opd)
    n = len(T)
    h1 = [elem(field, v) for v in h1]
    h2 = [elem(field, v) for v in h2]
    num, den = [], []
    for i in range(n):
        nx = (i + 1) % n
        a = Fd.add(Fx[i], gamma)
        b = Fd.add(Fd.add(T[i], Fd.mul(delta, T[nx])), g)
        num.append(Fd.mul(Fd.mul(a, b), opd))
        c = Fd.add(Fd.add(h1[i], Fd.mul(delta, h2[i])), g)
        d = Fd.add(Fd.add(h2[i], Fd.mul(delta, h1[nx])), g)
        den.append(Fd.mul(c, d))
    return num, den


def ratios(field, num, den):
    Fd = FIELDS[field]
    return [Fd.zero if d == Fd.zero else Fd.mul(N, Fd.inv(d)) for N, d in zip(num, den)]


def z_of(field, num, den):
    """calculateZ on the two columns -> z, n field elements"""
    Fd = FIELDS[field]
    z, acc = [], Fd.one
    for r in ratios(field, num, den):
        z.append(acc)
        acc = Fd.mul(acc, r)
    return z


def plookup_z(field, f, t, h1, h2, alpha, beta, gamma, delta):
    return z_of(field, *num_den(field, f, t, h1, h2, alpha, beta, gamma, delta))


def closing(field, f, t, h1, h2, alpha, beta, gamma, delta):
    """z[n-1] num[n-1] / den[n-1]: 1 exactly when the whole product closes"""
    Fd = FIELDS[field]
    num, den = num_den(field, f, t, h1, h2, alpha, beta, gamma, delta)
    return Fd.mul(z_of(field, num, den)[-1], ratios(field, num, den)[-1])


def h1h2(field, Fx, T):
    """the field's own checker of calculateH1H2 on the folded columns"""
    if field == "gl":
        return hints_ref.h1h2(Fx, T)
    return bn128_h1h2_ref.h1h2(Fx, T)


def valid_lookup(rng, field, n, k_f, k_t, sel_f=False, sel_t=False, alpha=None, beta=None, distinct=4):
    """-> (f, t, h1, h2): a lookup that HOLDS.  t's rows are drawn from `distinct` tuples; every selected f tuple is the tuple of a selected
    t row (a longer side carries leading zero columns, so that the two compressions agree); selectors are 0 / 1, row 0 of t always
    selected; an unselected f row may hold anything.  h1, h2: the field's h1h2 checker on the folded F and T."""
    q = FIELDS[field].q
    k = min(k_f, k_t)
    pool = [[rng.randrange(q) for _ in range(k)] for _ in range(distinct)]
    pad = lambda row, kk: [0] * (kk - k) + list(row)                                 # noqa: E731
    t_rows = [pad(rng.choice(pool), k_t) for _ in range(n)]
    st = [1 if i == 0 or rng.random() < 0.7 else 0 for i in range(n)] if sel_t else None
    live = [t_rows[i][k_t - k:] for i in range(n) if st is None or st[i]]
    sf = [1 if rng.random() < 0.6 else 0 for _ in range(n)] if sel_f else None
    f_rows = [pad(rng.choice(live), k_f) if sf is None or sf[i] else [rng.randrange(q) for _ in range(k_f)] for i in range(n)]
    if alpha is None:
        alpha = tuple(rng.randrange(q) for _ in range(3)) if field == "gl" else rng.randrange(q)
    if beta is None:
        beta = tuple(rng.randrange(q) for _ in range(3)) if field == "gl" else rng.randrange(q)
    f, t = (f_rows, sf), (t_rows, st)
    Fx, T = fold(field, f, t, alpha, beta)
    a, b = h1h2(field, Fx, T)
    return f, t, a, b, alpha, beta


def plan(n, field):
    """the numbers of pil2gl_plookup_plan, restated: logup_sum's geometry and bytes (the same passes with a product in them)"""
    from logup_sum_ref import plan as _logup_plan
    return _logup_plan(n, 1, field)
