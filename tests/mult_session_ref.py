"""The checker of the multiplicity sessions: the statement of include/pil2gl.h over Python integers and one dictionary -- open makes the
table, every add counts sides of their own lengths and reports on itself alone, m shows the counts so far.  It knows nothing of slots,
LDS, atomics or 32-bit halves: a counter is a Python integer.  Nothing here touches the library."""
from conn_pols_ref import P, R, MONT
from range_mult_ref import value

NONE = (1 << 64) - 1


def element(count, q):
    """a count as the library writes it: itself over Goldilocks, its Montgomery form over Fr"""
    return count if q == P else count * MONT % R


class _Session:
    def add(self, fs, sel_fs=None):
        """fs: the sides of ONE add, each a list of rows of its own length; sel_fs: per side a list of patterns or None
        -> this add's (kind, side, row, matched)"""
        missing, matched = None, 0
        for s, f in enumerate(fs):
            sel = None if sel_fs is None else sel_fs[s]
            for i, row in enumerate(f):
                if sel is not None and sel[i] % self.q == 0:
                    continue
                c = self.counter(row)
                if c is None:
                    missing = missing or (s, i)       # sides and rows are walked in order: the first is the smallest pair
                else:
                    self.cnt[c] += 1
                    matched += 1
        self.total += matched
        return ((1,) + missing if missing else (0, NONE, NONE)) + (matched,)


class LookupSession(_Session):
    """t: nT rows, a row a sequence of k patterns (they count mod q); sel_t: nT patterns or None; seed: what every counter starts from"""

    def __init__(self, t, q, sel_t=None, seed=0):
        self.q, self.n, self.total, self.first, self.cnt = q, len(t), 0, {}, {}
        for j, row in enumerate(t):
            if sel_t is None or sel_t[j] % q:
                self.first.setdefault(tuple(v % q for v in row), j)
        self.cnt = {j: seed for j in self.first.values()}

    def counter(self, row):
        return self.first.get(tuple(v % self.q for v in row))

    def m(self):
        return [self.cnt.get(j, 0) for j in range(self.n)]


class RangeSession(_Session):
    """the range [lo, lo + size) over the field of q; a side's row is one pattern"""

    def __init__(self, lo, size, q, seed=0):
        self.q, self.lo, self.size, self.total = q, lo, size, 0
        self.cnt = [seed] * size

    def counter(self, pattern):
        j = (value(pattern, self.q) - self.lo) % self.q
        return j if j < self.size else None

    def m(self, n_m, row0=0):
        assert row0 + self.size <= n_m
        return [0] * row0 + list(self.cnt) + [0] * (n_m - row0 - self.size)
