"""The checker of the range-check multiplicities: the statement of include/pil2gl.h over Python integers -- a value is in range when its
difference from lo, taken mod the modulus, is below size, and counts at that difference.  It knows nothing of the device's counters, its
LDS or its atomics.  Nothing here touches the library."""
from conn_pols_ref import P, R, MONT

NONE = (1 << 64) - 1
MONT_INV = pow(MONT, -1, R)


def value(pattern, q):
    """the field value of a bit pattern as the library reads it: the word mod p; the normal form of a Montgomery pattern mod r"""
    return pattern % q if q == P else pattern % R * MONT_INV % R


def multiplicities(fs, lo, size, n, q, sel_fs=None, row0=0):
    """fs: the f sides, each n bit patterns; lo: an integer, negative allowed; sel_fs: per side n patterns or None
    -> (m as n plain counts, (kind, side, row, matched) as the report's words)"""
    assert 1 <= size and row0 + size <= n
    m = [0] * n
    missing, matched = None, 0
    for s, f in enumerate(fs):
        sel = None if sel_fs is None else sel_fs[s]
        for i in range(n):
            if sel is not None and sel[i] % q == 0:   # a selector is zero as a pattern mod q exactly when its value is
                continue
            j = (value(f[i], q) - lo) % q
            if j < size:
                m[row0 + j] += 1
                matched += 1
            else:
                missing = missing or (s, i)           # sides and rows are walked in order: the first is the smallest pair
    assert sum(m) == matched
    return m, ((1,) + missing if missing else (0, NONE, NONE)) + (matched,)


def pattern(v, q):
    """the integer v as the library stores it: v mod p, or the Montgomery form of v mod r"""
    return v % q if q == P else v % R * MONT % R


def table_column(lo, size, n, q):
    """the materialised, padded range column of lookup_mult's equivalence: t[i] = field(lo + min(i, size - 1)), as patterns"""
    return [pattern(lo + min(i, size - 1), q) for i in range(n)]


def element(count, q):
    """a count as the library writes it: itself over Goldilocks, its Montgomery form over Fr"""
    return count if q == P else count * MONT % R
