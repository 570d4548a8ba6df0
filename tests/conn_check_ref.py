"""The checker of the connection check: the statement of include/pil2gl.h over Python integers and one dictionary -- id(i, j) = w^i ks'[j],
every S[c] must be the id of exactly one cell c' and a[c] must equal a[c'].  It knows nothing of the device's hash table, its power tables
or its minima.  Its S comes from tests/conn_pols_ref.py's sequential swaps.  Nothing here touches the library."""
from conn_pols_ref import P, R, MONT

NONE = (1 << 64) - 1
CLEAN, NAMES_NO_CELL, VALUES_DIFFER, IDS_NOT_DISTINCT = 0, 1, 2, 3


def check(a, S, n_cols, N, w, ks1, q):
    """a, S: flat lists of N * n_cols VALUES mod q (cell i * n_cols + j); ks1 includes ks1[0] -> (cell, partner, kind) as the report's words"""
    where = {}
    x = 1
    for i in range(N):
        for j in range(n_cols):
            ident = x * ks1[j] % q
            if ident in where:
                return i * n_cols + j, where[ident], IDS_NOT_DISTINCT
            where[ident] = i * n_cols + j
        x = x * w % q
    for c in range(N * n_cols):
        to = where.get(S[c] % q)
        if to is None:
            return c, NONE, NAMES_NO_CELL
        if a[c] % q != a[to] % q:
            return c, to, VALUES_DIFFER
    return NONE, NONE, CLEAN


def values(words, q):
    """the library's words (uint64 array, Goldilocks (.) or Fr (., 4) Montgomery) -> flat values mod q"""
    if q == P:
        return [int(v) % P for v in words.reshape(-1)]
    inv = pow(MONT, -1, R)
    rows = words.reshape(-1, 4)
    return [sum(int(r[k]) << (64 * k) for k in range(4)) % R * inv % R for r in rows]
