"""The checker of the lookup multiplicities: the statement of include/pil2gl.h over Python integers and one dictionary -- count the selected
rows of every f side per tuple of values mod the modulus, then walk t in row order.  It knows nothing of the device's hash table, its
slots or its atomics.  Nothing here touches the library."""
from conn_pols_ref import P, R, MONT

NONE = (1 << 64) - 1


def multiplicities(fs, t, q, sel_fs=None, sel_t=None):
    """fs: the f sides, each n rows, a row a sequence of k integers (any bit patterns: they count mod q; over Fr the Montgomery patterns,
    which are equal mod r exactly when the values are); t alike; sel_fs: per side n integers or None; sel_t: n integers or None
    -> (m as n plain counts, (kind, side, row, matched) as the report's words)"""
    key = lambda row: tuple(v % q for v in row)                                  # noqa: E731
    on = lambda sel, i: sel is None or sel[i] % q != 0                           # noqa: E731
    first = {}                                        # tuple -> its smallest selected row of t
    for j, row in enumerate(t):
        if on(sel_t, j):
            first.setdefault(key(row), j)
    m = [0] * len(t)
    missing, matched = None, 0
    for s, f in enumerate(fs):
        sel = None if sel_fs is None else sel_fs[s]
        for i, row in enumerate(f):
            if not on(sel, i):
                continue
            j = first.get(key(row))
            if j is None:
                missing = missing or (s, i)           # sides and rows are walked in order: the first is the smallest pair
            else:
                m[j] += 1
                matched += 1
    assert sum(m) == matched
    return m, ((1,) + missing if missing else (0, NONE, NONE)) + (matched,)


def element(count, q):
    """a count as the library writes it: itself over Goldilocks, its Montgomery form over Fr"""
    return count if q == P else count * MONT % R
