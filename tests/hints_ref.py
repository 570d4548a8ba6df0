"""The Goldilocks stage-2 hints over Python integers, written from the definitions and sharing no code with the C oracle or the library:
F_p with p = 2^64 - 2^32 + 1; the cubic extension F_p[x] / (x^3 - x - 1) of the reference's src/helpers/f3g.js (schoolbook product, then
x^3 = x + 1 and x^4 = x^2 + x; the inverse solves the 3 x 3 system `a y = 1` by cofactors, not f3g.js's closed formula); calculateZ /
calculateS of polutils.js:128-164 with a zero denominator giving ratio 0; calculateH1H2 of polutils.js:105-126 as a merge (t[i], then the
rows of f with that value once i is the value's last row).  Beside them the plan arithmetic and the key hash of csrc/hint_plan.h, restated."""
P = 2 ** 64 - 2 ** 32 + 1
M64 = 2 ** 64 - 1
THREADS, ITEMS = 256, 8
CHUNK = THREADS * ITEMS


# ---- the field and its cubic extension ----
def e3(v, dim):
    """row v of a column of dimension dim -> an extension element"""
    return (int(v[0]), int(v[1]), int(v[2])) if dim == 3 else (int(v[0]), 0, 0)


def add3(a, b):
    return ((a[0] + b[0]) % P, (a[1] + b[1]) % P, (a[2] + b[2]) % P)


def mul3(a, b):
    c = [0] * 5
    for i in range(3):
        for j in range(3):
            c[i + j] += a[i] * b[j]
    # x^3 = x + 1, x^4 = x^2 + x
    return ((c[0] + c[3]) % P, (c[1] + c[3] + c[4]) % P, (c[2] + c[4]) % P)


def inv3(a):
    """0 -> 0 (what 0^(p-2) gives); else y with a y = 1, from the matrix of `times a` in the basis 1, x, x^2"""
    if a == (0, 0, 0):
        return (0, 0, 0)
    cols = [a, mul3(a, (0, 1, 0)), mul3(a, (0, 0, 1))]
    m = [[cols[j][i] for j in range(3)] for i in range(3)]            # m[i][j]: coefficient of x^i in a x^j

    def cof(i, j):
        r = [k for k in range(3) if k != i]
        c = [k for k in range(3) if k != j]
        return (-1) ** (i + j) * (m[r[0]][c[0]] * m[r[1]][c[1]] - m[r[0]][c[1]] * m[r[1]][c[0]])
    det = sum(m[0][j] * cof(0, j) for j in range(3)) % P
    di = pow(det, P - 2, P)
    return tuple(cof(0, j) * di % P for j in range(3))                # the first column of the inverse matrix: adj[j][0] = cof(0, j)


def _ratios(num, dim_num, den, dim_den, one_num):
    n = len(den)
    return [mul3(e3(num[0 if one_num else i], dim_num), inv3(e3(den[i], dim_den))) for i in range(n)]


def _flat(rows, dim):
    return [w for r in rows for w in r[:dim]]


def gprod(num, dim_num, den, dim_den):
    """num, den: n rows of dim words -> the words of z, z[0] = 1, z[i] = z[i-1] num[i-1] / den[i-1]"""
    z, out = (1, 0, 0), []
    for r in _ratios(num, dim_num, den, dim_den, False):
        out.append(z)
        z = mul3(z, r)
    return _flat(out, max(dim_num, dim_den))


def gsum(num, dim_num, den, dim_den):
    """num: ONE row -> the words of s, s[i] = s[i-1] + num / den[i]"""
    s, out = (0, 0, 0), []
    for r in _ratios(num, dim_num, den, dim_den, True):
        s = add3(s, r)
        out.append(s)
    return _flat(out, max(dim_num, dim_den))


def h1h2(f, t):
    """f, t: lists of hashable values -> (h1, h2); raises ValueError("Number not included: w:j") at the first j with f[j] not in t"""
    last = {v: i for i, v in enumerate(t)}
    cnt = {}
    for j, v in enumerate(f):
        if v not in last:
            raise ValueError("Number not included: w:%d" % j)
        cnt[v] = cnt.get(v, 0) + 1
    s = []
    for i, v in enumerate(t):
        s.append(v)
        if last[v] == i:
            s.extend([v] * cnt.get(v, 0))
    return s[0::2], s[1::2]


# ---- csrc/hint_plan.h ----
def plan(n):
    nb = -(-n // CHUNK)
    cap = 2
    while cap < 2 * n:
        cap *= 2
    return {"threads": THREADS, "items": ITEMS, "chunk": CHUNK, "blocks": nb, "totalsPerLane": -(-nb // THREADS),
            "h1h2CapBits": cap.bit_length() - 1 if n <= 1 << 30 else 0}


def key_hash(words):
    g = 0x9E3779B97F4A7C15
    h = g
    for w in words:
        h ^= (int(w) + g + (h << 6) + (h >> 2)) & M64
        h = h * 0xBF58476D1CE4E5B9 & M64
        h ^= h >> 31
    return h


def home(words, capacity):
    return key_hash(words) & (capacity - 1)
