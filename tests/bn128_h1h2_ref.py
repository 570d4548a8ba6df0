"""The checker of the BN254 Fr plookup hint (a plain module: tests/test_bn128_h1h2_cpu.py, tests/test_gpu_bn128_h1h2.py and the Node test's
expectations build on it): calculateH1H2 of src/helpers/polutils.js:105-130 transcribed line by line over hashable Python values -- a
dict for the last index of every value of t, the pairs (value, index) of t and then of f, a STABLE sort by the index, and the even and
odd entries.  The device never sorts (it repeats t[i] 1 + cnt[i] times); `by_counts` below is that second formulation, kept apart so that
the CPU test can set one against the other.  Values are compared as they are: integers for the words the device compares as bytes."""


class NotIncluded(Exception):
    def __init__(self, row, value):
        Exception.__init__(self, "Number not included: w:%d, value:%s" % (row, value))
        self.row, self.value = row, value


def h1h2(f, t):
    """statement for statement what polutils.js:106-129 does; the line of the reference beside each step"""
    idx_t = {}                                      # :106  the last index of every value of t
    s = []                                          # :107  the pairs (value, index)
    for i in range(len(t)):                         # :108
        idx_t[t[i]] = i                             # :109  a later occurrence overwrites an earlier one
        s.append((t[i], i))                         # :110
    for i in range(len(f)):                         # :112
        idx = idx_t.get(f[i])                       # :113
        if idx is None:                             # :114  no such key
            raise NotIncluded(i, f[i])              # :115  the first such row ends the call
        s.append((f[i], idx))                       # :117
    s.sort(key=lambda a: a[1])                      # :120  by the index alone; stable, as the reference's sort is
    h1 = [None] * len(f)                            # :122
    h2 = [None] * len(f)                            # :123
    for i in range(len(f)):                         # :124
        h1[i] = s[2 * i][0]                         # :125  the even entries
        h2[i] = s[2 * i + 1][0]                     # :126  the odd entries
    return h1, h2                                   # :129


def by_counts(f, t, first_occurrence=False):
    """the second formulation: t[i] repeated 1 + cnt[i] times, the counts of a value at its last occurrence (first_occurrence: at its
    first -- the mistake the tests must tell apart)"""
    where = {}
    for i, v in enumerate(t):
        if not (first_occurrence and v in where):
            where[v] = i
    cnt = [0] * len(t)
    for j, v in enumerate(f):
        if v not in where:
            raise NotIncluded(j, v)
        cnt[where[v]] += 1
    s = [v for i, v in enumerate(t) for _ in range(1 + cnt[i])]
    return s[0::2], s[1::2]
