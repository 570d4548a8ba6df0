"""The clustered logUp sum of include/pil2gl.h over Python integers, from the statement and sharing no code with the library:

    frac_u[i] = coef_u w_u[i] / D_u[i]  (an f term)   |   [in window] coefR m_r[i] / E_r[i]  (a range)   |   0 at a zero denominator
    im_c[i]   = sum_{cluster[u] = c} frac_u[i]                                           c < n_im
    s[i]      = s[i-1] + sum_c im_c[i] + sum_{cluster[u] = DIRECT} frac_u[i]             s[-1] = 0

Fields, f terms, ranges and challenges are logup_sum_ref's and range_sum_ref's (a range's m is consulted ONLY inside its window).  cluster
holds one entry a term, the f terms first, then the ranges: a cluster id, or DIRECT."""
import logup_sum_ref as lref
import range_sum_ref as rref

FIELDS = lref.FIELDS
DIRECT = (1 << 64) - 1


def fractions(F, terms, ranges, alpha, beta, i):
    """frac_u[i] for every term, f terms first; a range outside its window and a zero denominator give 0"""
    out = []
    for tuples, w, coef, bus in terms:
        d = lref.denominator(F, tuples[i], alpha, beta, bus)
        out.append(F.zero if d == F.zero else F.mul(F.base(coef * (1 if w is None else w[i])), F.inv(d)))
    for rng in ranges:
        if not rref.in_window(rng, i):
            out.append(F.zero)
            continue
        d = rref.range_denominator(F, rng, alpha, beta, i)
        out.append(F.zero if d == F.zero else F.mul(F.base(rng[4] * rref.m_at(rng[0], i)), F.inv(d)))
    return out


def cluster_sum(field, terms, ranges, cluster, n_im, alpha, beta, n):
    """-> (s, im): s as n field elements, im[c] as n field elements for every cluster (triples over Goldilocks, integers over Fr)"""
    F = FIELDS[field]
    alpha, beta = F.ext(alpha), F.ext(beta)
    assert len(cluster) == len(terms) + len(ranges)
    s, im, acc = [], [[] for _ in range(n_im)], F.zero
    for i in range(n):
        fr = fractions(F, terms, ranges, alpha, beta, i)
        row = [F.zero] * n_im
        for u, c in enumerate(cluster):
            if c != DIRECT:
                row[c] = F.add(row[c], fr[u])
        for c in range(n_im):
            im[c].append(row[c])
            acc = F.add(acc, row[c])
        for u, c in enumerate(cluster):
            if c == DIRECT:
                acc = F.add(acc, fr[u])
        s.append(acc)
    return s, im


def members(terms, ranges, cluster, c):
    """the f terms and the ranges of cluster c (or of the DIRECT part)"""
    return ([t for u, t in enumerate(terms) if cluster[u] == c], [r for v, r in enumerate(ranges) if cluster[len(terms) + v] == c])


def plan(n, field):
    """the numbers of pil2gl_logup_cluster_plan, restated: (threads, rows a lane, blocks, launches, depth, width), working bytes.  Goldilocks:
    logup_sum's.  Fr: two kernels of its own around the inversion's and the scan's 2 levels - 1 launches each; bn_scan's levels and P"""
    info, nbytes = lref.plan(n, 1, field)
    if field == "gl" or not n:
        return info, nbytes
    levels = info[4]
    return (info[0], info[1], info[2], 2 + 2 * (2 * levels - 1), levels, info[5]), nbytes - 32 * n
