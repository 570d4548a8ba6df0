"""The checker of the lookup and permutation checks: the statement of include/pil2gl.h over Python integers and one dictionary -- count the
selected rows of f and of t per tuple of values mod the modulus, then apply the mode's criterion in row order.  It knows nothing of the
device's hash table, its slots or its minima.  Nothing here touches the library."""
from conn_pols_ref import P, R

NONE = (1 << 64) - 1
LOOKUP, PERMUTATION = 0, 1
CLEAN, F_NOT_IN_T, F_MORE_THAN_T, T_MORE_THAN_F = 0, 1, 2, 3
CLEAN_REPORT = (CLEAN, NONE, NONE, 0, 0)


def check(f, t, mode, q, sel_f=None, sel_t=None):
    """f, t: n rows each, a row a sequence of k integers (any bit patterns: they count mod q; over Fr the Montgomery patterns, which are
    equal mod r exactly when the values are); sel_f, sel_t: n integers each or None -> (kind, row, partner, cntF, cntT) as the report's words"""
    count = {}                                        # tuple -> [cntF, cntT, first selected row of f, of t]

    def rows(side, sel, which):
        for i, row in enumerate(side):
            if sel is not None and sel[i] % q == 0:
                continue
            e = count.setdefault(tuple(v % q for v in row), [0, 0, NONE, NONE])
            e[which] += 1
            e[2 + which] = min(e[2 + which], i)
            yield i
    sel_rows_f, sel_rows_t = list(rows(f, sel_f, 0)), list(rows(t, sel_t, 1))
    of = lambda side, i: count[tuple(v % q for v in side[i])]                    # noqa: E731
    for i in sel_rows_f:
        cnt_f, cnt_t, _, first_t = of(f, i)
        if cnt_t == 0 if mode == LOOKUP else cnt_f > cnt_t:
            return (F_NOT_IN_T if cnt_t == 0 else F_MORE_THAN_T), i, first_t, cnt_f, cnt_t
    if mode == PERMUTATION:
        for i in sel_rows_t:
            cnt_f, cnt_t, first_f, _ = of(t, i)
            if cnt_t > cnt_f:
                return T_MORE_THAN_F, i, first_f, cnt_f, cnt_t
    return CLEAN_REPORT


def patterns(words, q):
    """the library's words of a matrix, (rows, stride) uint64 over Goldilocks or (rows, stride, 4) over Fr -> rows of integers as they are"""
    if q == P:
        return [[int(v) for v in row] for row in words]
    return [[sum(int(e[k]) << (64 * k) for k in range(4)) for e in row] for row in words]


def tuples(words, cols, q):
    """the k columns `cols`, in that order, of every row"""
    return [[row[c] for c in cols] for row in patterns(words, q)]


def column(words, col, q):
    return [row[col] for row in patterns(words, q)]

