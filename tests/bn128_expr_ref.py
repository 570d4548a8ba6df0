"""Pure-Python checker of the BN254 Fr expression evaluator (pil2gl.bn128.eval_program over csrc/bn_expr.hip).

What pins the expected values: the reference tree holds no fflonk op-list and no Fr arithmetic of its own (ffjavascript is not vendored
there), so nothing recorded from it can serve.  The values come from here instead: Python integers mod r, and a row loop written from
the reference's compileCode / getRef / setRef / evalMap (src/prover/prover_helpers.js:83-107, :109-259) as calculateExps runs it
(:31-45): rows one after the other, the ops of a row in order, every operand resolved as the generated JavaScript would.

Elements are handled as the integers ffjavascript's Fr keeps in memory, a * 2^256 mod r (Montgomery form), because that is what crosses
the library's API: F.add and F.sub are the plain sum and difference mod r, F.mul(x, y) = x * y * 2^-256 mod r.

Programs are lists of op tuples (op, dest, src0, src1) of refs (kind, dim, section, prime, index), the tuples pil2gl.bn128.encode_program
returns; a section is a list of rows, each a list of `width` integers, and is changed in place."""
import random

import numpy as np

from bn128_fft_ref import R, MONT, MONT_INV, to_mont, from_mont, words_of, ints_of       # noqa: F401  (re-exported for the tests)

ADD, SUB, MUL, COPY = 0, 1, 2, 3
TMP, SEC, SCALAR = 0, 1, 2


def tmp(i):
    return (TMP, 1, 0, 0, i)


def sec(section, column=0, prime=0):
    return (SEC, 1, section, prime, column)


def scalar(i):
    return (SCALAR, 1, 0, 0, i)


def f_mul(x, y):
    return x * y * MONT_INV % R


def row_index(i, prime, n_bits, prime_shift):
    """evalMap, prover_helpers.js:223-230: next = prime < 0 ? prime + N : prime, shifted left by extendBits on "ext"; ((i + next) % N)"""
    n = 1 << n_bits
    if not prime:
        return i
    nxt = (prime + n if prime < 0 else prime) << prime_shift
    return (i + nxt) % n


def evaluate(ops, sections, scalars, n_bits, prime_shift=0):
    """calculateExps: for i in 0..N-1, every op in order.  sections[s][row][column] and scalars[k] are Montgomery integers."""
    n = 1 << n_bits
    n_tmp = 1 + max([r[4] for o in ops for r in o[1:] if r is not None and r[0] == TMP], default=-1)

    def get(r, i, t):
        if r[0] == TMP:
            return t[r[4]]
        if r[0] == SCALAR:
            return scalars[r[4]]
        return sections[r[2]][row_index(i, r[3], n_bits, prime_shift)][r[4]]

    for i in range(n):
        t = [None] * n_tmp
        for op, d, a, b in ops:
            x = get(a, i, t)
            if op == ADD:
                v = (x + get(b, i, t)) % R
            elif op == SUB:
                v = (x - get(b, i, t)) % R
            elif op == MUL:
                v = x * get(b, i, t) * MONT_INV % R
            elif op == COPY:
                v = x
            else:
                raise ValueError("Invalid op:%r" % (op,))
            if d[0] == TMP:
                t[d[4]] = v
            elif d[0] == SEC:
                sections[d[2]][row_index(i, d[3], n_bits, prime_shift)][d[4]] = v
            else:
                raise ValueError("Invalid reference type set")


# ---- the library's buffers -------------------------------------------------------------------------------------------------------
def section_words(rows):
    """[row][column] Montgomery integers -> (rows, width, 4) uint64"""
    raw = b"".join(v.to_bytes(32, "little") for row in rows for v in row)
    return np.frombuffer(raw, dtype="<u8").reshape(len(rows), len(rows[0]), 4).copy()


def section_of(words):
    rows, width = words.shape[0], words.shape[1]
    raw = np.ascontiguousarray(words, dtype="<u8").tobytes()
    flat = [int.from_bytes(raw[k:k + 32], "little") for k in range(0, len(raw), 32)]
    return [flat[j * width:(j + 1) * width] for j in range(rows)]


def random_section(rng, rows, width):
    return [[rng.randrange(R) for _ in range(width)] for _ in range(rows)]


# ---- programs the tests share ----------------------------------------------------------------------------------------------------
def live_program(k, out_section=1):
    """k cells of section 0 (width >= k) loaded into k temporaries that are all alive at once, then summed into column 0 of out_section:
    k temporary slots after live-range renumbering, no fewer"""
    ops = [(COPY, tmp(j), sec(0, j), None) for j in range(k)]
    if k == 1:
        return ops + [(COPY, sec(out_section), tmp(0), None)]
    acc = k
    ops.append((ADD, tmp(acc), tmp(0), tmp(1)))
    for j in range(2, k):
        ops.append((ADD, tmp(acc + 1), tmp(acc), tmp(j)))
        acc += 1
    return ops + [(COPY, sec(out_section), tmp(acc), None)]


def random_program(seed, n_ops, in_width, n_scalars, hold=0, primes=(0,)):
    """a seeded op-list of about n_ops ops: reads section 0 (in_width columns, row offsets from `primes`) and the scalar pool, keeps a
    window of recent temporaries, writes column 0 of section 1 at the end.  hold > 0: that many products of a cell and a scalar are formed first and added in
    only at the end, so that the distinct ones among them stay alive throughout (the planner hook says how many slots that takes)."""
    rng = random.Random(seed)
    ops, nxt = [], 0
    held = []
    for j in range(hold):
        ops.append((MUL, tmp(nxt), sec(0, j % in_width, primes[j % len(primes)]), scalar(j % n_scalars)))
        held.append(nxt)
        nxt += 1
    recent = []

    def operand():
        k = rng.randrange(10)
        if recent and k < 5:
            return tmp(rng.choice(recent))
        if k < 8:
            return sec(0, rng.randrange(in_width), rng.choice(primes))
        return scalar(rng.randrange(n_scalars))

    while len(ops) < n_ops:
        op = rng.choice((ADD, SUB, MUL, MUL, COPY))
        a = operand()
        b = operand() if op != COPY else None
        ops.append((op, tmp(nxt), a, b))
        recent.append(nxt)
        nxt += 1
        if len(recent) > 6:
            recent.pop(rng.randrange(len(recent)))
    acc = recent[-1]
    for t in recent[:-1] + held:
        ops.append((ADD, tmp(nxt), tmp(acc), tmp(t)))
        acc = nxt
        nxt += 1
    ops.append((COPY, sec(1), tmp(acc), None))
    return ops
