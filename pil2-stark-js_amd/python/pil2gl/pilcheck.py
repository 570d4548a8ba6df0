"""PIL's two non-polynomial identity kinds beside `connect`, checked on the device as statements about the trace (csrc/tuple_check.hip):

    selF {f0..fk-1} in selT {t0..tk-1}     plookup        lookup_check / lookup_check_dev
    selF {f0..fk-1} is selT {t0..tk-1}     permutation    perm_check / perm_check_dev

    rep = lookup_check(f, [0, 1, 2], t, [0, 1, 2], n)                      # host matrices in
    rep = perm_check_dev(cm1, [7, 3], cm1, [4, 5], n, sel_f=(cm1, 9))     # column sets of one resident matrix, a selector column

A matrix is (rows, stride) uint64 words over Goldilocks and (rows, stride, 4) Montgomery words over Fr (or flat, with the stride given);
cols are element offsets within a row, in the tuple's order; a selector is (matrix, col) or (matrix, col, stride), or None.  Every form
returns the library's five words (kind, row, partner, cntF, cntT) -- include/pil2gl.h states them; a clean trace gives
(0, NONE, NONE, 0, 0).  No arithmetic happens here: hashing, counting and judging are the library's.

The column that PROVES a lookup in pil2, the multiplicities of its grand sum (csrc/lookup_mult.hip), is lookup_mult / lookup_mult_dev at the
end of this module, then its form for a range check, which needs no table column (range_mult / range_mult_dev, csrc/range_mult.hip), and
after them the grand sum that consumes the column (logup_sum / logup_sum_dev), its form for range checks, which takes the ranges as
numbers (range_sum / range_sum_dev, and range_logup for both halves), the sessions that count a table's m over the f sides of other
AIRs, each of its own length (LookupSession, RangeSession, and range_logup_cross for a table AIR with its user AIRs), the clustered form of both that writes the im columns beside s
(logup_cluster / logup_cluster_dev, range_logup_clustered), and the grand product of a permutation or a connection
(grand_prod / grand_prod_dev, with perm_prod and conn_prod as spellings of the two identities), and last pil1's plookup argument
(plookup_fold, plookup_h1h2, plookup_prod and their _dev forms).
"""
import ctypes as C

import numpy as np

from ._lib import Pil2glError, call, load
from . import _is_dev, _ptr, _stream, torch

NONE = 0xFFFFFFFFFFFFFFFF
LOOKUP, PERMUTATION = 0, 1
_WORDS = {"gl": 1, "bn128": 4}


def _plan(entry, args, names, bytes_name="scratchBytes"):
    """a host-only plan entry: six words under their names and a byte count"""
    info = (C.c_uint32 * 6)()
    nbytes = C.c_uint64()
    call(entry, *args, info, C.byref(nbytes))
    return dict(zip(names, (int(x) for x in info)), **{bytes_name: nbytes.value})


_TABLE_PLAN = ("capBits", "threads", "blocks", "launches", "headerBytes", "slotBytes")


def tuple_check_plan(n, k, field="gl", mode=LOOKUP):
    """pil2gl_tuple_check_plan (host-only): the hash table's capacity, the launch geometry, the working buffer"""
    return _plan("pil2gl_tuple_check_plan", (n, k, _WORDS[field], mode), _TABLE_PLAN)


def tuple_home(words, k, field="gl", capacity=16):
    """pil2gl_debug_tuple_home (host-only): the home slot of a tuple of k CANONICAL elements given as words (k, or (k, 4) over Fr)"""
    w = np.ascontiguousarray(words, np.uint64).reshape(-1)
    if w.size != k * _WORDS[field]:
        raise Pil2glError("the tuple holds %d words, k = %d elements of %d words expected" % (w.size, k, _WORDS[field]))
    home = int(load().pil2gl_debug_tuple_home(C.c_void_p(w.ctypes.data), k, _WORDS[field], capacity))
    if home == NONE:
        raise Pil2glError("tuple_home: k is 1 .. 16 and the capacity a power of two")
    return home


def tuple_check_probe():
    """pil2gl_debug_tuple_check_probe: the longest distance between a tuple of the last call's hash table and its home slot"""
    return int(load().pil2gl_debug_tuple_check_probe())


def _matrix(m, stride, words, dev, what):
    """a matrix as (buffer, words it holds, stride in elements)"""
    if _is_dev(m) != dev:
        raise Pil2glError("%s: the _dev forms take device tensors, the others host arrays" % what)
    if not dev:
        m = np.ascontiguousarray(m, np.uint64)
    shape = tuple(m.shape)
    if stride is None:
        if len(shape) != (2 if words == 1 else 3) or (words == 4 and shape[2] != 4):
            raise Pil2glError("%s: give a (rows, stride%s) matrix or its stride" % (what, ", 4" if words == 4 else ""))
        stride = shape[1]
    return m, (m.numel() if dev else m.size), stride


def _side(m, cols, stride, sel, n, words, dev, what):
    """one side as the entries take it: (buffer, stride, cols array, selector buffer, its stride, its column); sizes checked here, because
    the library cannot know where a buffer ends"""
    m, held, stride = _matrix(m, stride, words, dev, what)
    cols = np.ascontiguousarray(cols, np.uint64).reshape(-1)
    if n and cols.size and held < ((n - 1) * stride + int(cols.max()) + 1) * words:
        raise Pil2glError("%s holds %d words, %d rows of stride %d need more" % (what, held, n, stride))
    if sel is None:
        return m, stride, cols, None, 0, 0
    sm, sheld, sstride = _matrix(sel[0], sel[2] if len(sel) > 2 else None, words, dev, "the selector of " + what)
    if n and sheld < ((n - 1) * sstride + sel[1] + 1) * words:
        raise Pil2glError("the selector of %s holds %d words, %d rows of stride %d need more" % (what, sheld, n, sstride))
    return m, stride, cols, sm, sstride, sel[1]


def _check(mode, dev, f, f_cols, t, t_cols, n, field, f_stride, t_stride, sel_f, sel_t):
    words = _WORDS[field]
    F = _side(f, f_cols, f_stride, sel_f, n, words, dev, "f")
    T = _side(t, t_cols, t_stride, sel_t, n, words, dev, "t")
    k = F[2].size
    if T[2].size != k:
        raise Pil2glError("f has %d columns and t %d" % (k, T[2].size))
    ptr = _ptr if dev else (lambda a: None if a is None else C.c_void_p(a.ctypes.data))
    cp = lambda c: C.c_void_p(c.ctypes.data)                                     # noqa: E731
    args = [ptr(F[0]), F[1], cp(F[2]), ptr(T[0]), T[1], cp(T[2]), ptr(F[3]), F[4], F[5], ptr(T[3]), T[4], T[5], n, k, mode]
    rep = (C.c_uint64 * 5)()
    name = "pil2gl_tuple_check" if words == 1 else "pil2gl_bn128_tuple_check"
    if dev:
        plan = tuple_check_plan(n, k, field, mode)
        work = torch.empty(max(plan["scratchBytes"] // 8, 2), dtype=torch.int64, device=F[0].device)
        call(name + "_dev", *args, _ptr(work), plan["scratchBytes"], rep, _stream())
    else:
        call(name, *args, rep)
    return tuple(int(x) for x in rep)


def lookup_check(f, f_cols, t, t_cols, n, field="gl", f_stride=None, t_stride=None, sel_f=None, sel_t=None):
    """does every selected row of f occur among the selected rows of t: host matrices -> (kind, row, partner, cntF, cntT)"""
    return _check(LOOKUP, False, f, f_cols, t, t_cols, n, field, f_stride, t_stride, sel_f, sel_t)


def perm_check(f, f_cols, t, t_cols, n, field="gl", f_stride=None, t_stride=None, sel_f=None, sel_t=None):
    """are the selected rows of f a permutation of the selected rows of t: host matrices -> (kind, row, partner, cntF, cntT)"""
    return _check(PERMUTATION, False, f, f_cols, t, t_cols, n, field, f_stride, t_stride, sel_f, sel_t)


def lookup_check_dev(f, f_cols, t, t_cols, n, field="gl", f_stride=None, t_stride=None, sel_f=None, sel_t=None):
    """lookup_check on device tensors, e.g. column sets of the stage-1 buffer before it is committed; the working buffer comes from the
    plan and lives for the call; blocks for the report"""
    return _check(LOOKUP, True, f, f_cols, t, t_cols, n, field, f_stride, t_stride, sel_f, sel_t)


def perm_check_dev(f, f_cols, t, t_cols, n, field="gl", f_stride=None, t_stride=None, sel_f=None, sel_t=None):
    """perm_check on device tensors"""
    return _check(PERMUTATION, True, f, f_cols, t, t_cols, n, field, f_stride, t_stride, sel_f, sel_t)


# ---- lookup multiplicities: the logUp column m of `selF_s {f_s} in selT {t}` (csrc/lookup_mult.hip) ----
#     rep = lookup_mult_dev([(cm1, [7, 3]), (cm1, [4, 5], (cm1, 9))], (cm1, [0, 1]), (cm1, 12), n)
# A side is (matrix, cols), (matrix, cols, sel) or (matrix, cols, sel, stride) with sel a selector as above or None; m is (matrix, col) or
# (matrix, col, stride) and may be a spare column of t's or of an f's matrix.  The column is written in place -- the host form takes m's
# matrix as a C-contiguous uint64 array -- and the four words (kind, side, row, matched) come back; clean is (0, NONE, NONE, matched).
def lookup_mult_plan(n, k, n_f=1, field="gl"):
    """pil2gl_lookup_mult_plan (host-only): the hash table's capacity, the launch geometry, the working buffer"""
    return _plan("pil2gl_lookup_mult_plan", (n, k, n_f, _WORDS[field]), _TABLE_PLAN)


def lookup_mult_probe():
    """pil2gl_debug_lookup_mult_probe: the longest distance between a tuple of the last call's hash table and its home slot"""
    return int(load().pil2gl_debug_lookup_mult_probe())


def _dev_ptr(dev):
    """a buffer's address as the entries take it; None stays null"""
    return (lambda a: _ptr(a)) if dev else (lambda a: None if a is None else a.ctypes.data)


def _sides(specs, whats, at, n, words, dev):
    """side specs (matrix, cols, sel, .., stride at `at`) as a TupleSide array (one element at least), each side's column count, and what
    must stay alive until the call returns: the buffers and the column arrays"""
    from ._lib import TupleSide
    ptr, keep, ks = _dev_ptr(dev), [], []
    arr = (TupleSide * max(len(specs), 1))()
    for i, (spec, what) in enumerate(zip(specs, whats)):
        spec = tuple(spec) + (None,) * (at + 1 - len(spec))
        b, stride, cols, sm, sstride, scol = _side(spec[0], spec[1], spec[at], spec[2], n, words, dev, what)
        keep.extend((b, cols, sm))
        ks.append(cols.size)
        arr[i] = TupleSide(ptr(b), stride, cols.ctypes.data, ptr(sm), sstride, scol)
    return arr, ks, keep


def _column(m, what, width, n, words, dev):
    """a column written in place, (matrix, col) or (matrix, col, stride), `width` words wide: its address, stride and column"""
    if not dev and not (isinstance(m[0], np.ndarray) and m[0].dtype == np.uint64 and m[0].flags.c_contiguous and m[0].flags.writeable):
        raise Pil2glError("%s: the host form writes in place and takes a C-contiguous writeable uint64 array" % what)
    mm, held, stride = _matrix(m[0], m[2] if len(m) > 2 else None, words, dev, what)
    if n and held < ((n - 1) * stride + m[1] + width) * words:
        raise Pil2glError("%s holds %d words, %d rows of stride %d need more" % (what, held, n, stride))
    return mm, [_dev_ptr(dev)(mm), stride, m[1]]


def _report4(dev, host_entry, dev_entry, args, plan, like, *dev_tail):
    """a multiplicity entry -> its four words; the device form takes its scratch from plan() on like's device"""
    rep = (C.c_uint64 * 4)()
    if dev:
        nbytes = plan()["scratchBytes"]
        work = torch.empty(max(nbytes // 8, 2), dtype=torch.int64, device=like.device)
        call(dev_entry, *args, _ptr(work), nbytes, rep, _stream(), *dev_tail)
    else:
        call(host_entry, *args, rep)
    return tuple(int(x) for x in rep)


def _mult(dev, fs, t, m, n, field):
    words = _WORDS[field]
    F, ks, keep = _sides(fs, ["f %d" % i for i in range(len(fs))], 3, n, words, dev)
    T, (k,), keep_t = _sides([t], ["t"], 3, n, words, dev)
    if any(kk != k for kk in ks):
        raise Pil2glError("t has %d columns, every f must have as many" % k)
    mm, col = _column(m, "m", 1, n, words, dev)
    name = "pil2gl_lookup_mult" if words == 1 else "pil2gl_bn128_lookup_mult"
    return _report4(dev, name, name + "_dev", [F, len(fs), T] + col + [n, k], lambda: lookup_mult_plan(n, k, min(max(len(fs), 1), 8), field), mm)


def lookup_mult(fs, t, m, n, field="gl"):
    """the multiplicity column of the lookups `f_s in t`: host matrices; m's column is written in place -> (kind, side, row, matched)"""
    return _mult(False, fs, t, m, n, field)


def lookup_mult_dev(fs, t, m, n, field="gl"):
    """lookup_mult on device tensors, e.g. columns of the stage-1 buffer with m one more column of it; the working buffer comes from the
    plan and lives for the call; blocks for the report"""
    return _mult(True, fs, t, m, n, field)


# ---- range-check multiplicities: the column m of `selF_s f_s in [lo, lo + size)` (csrc/range_mult.hip; include/pil2gl.h states it) ----
#     rep = range_mult_dev([(cm1, [7]), (cm1, [4], (cm1, 9))], -128, 256, (cm1, 12), n)
# The sides, m and the four words that come back are lookup_mult's; a side has ONE column.  There is no t: the table is the integers
# lo .. lo + size - 1 as field elements, and m's rows row0 .. row0 + size - 1 take their counts, every other row 0.  path: the count kernel,
# for the tests and the benchmark (0 LDS, 1 global, None the planner's choice).
def range_mult_plan(n, size, n_f=1, field="gl", path=None):
    """pil2gl_range_mult_plan (host-only): the count path, the launch geometry, the working buffer"""
    names = ("path", "threads", "blocks", "launches", "headerBytes", "ldsCounters")
    if path is None:
        return _plan("pil2gl_range_mult_plan", (n, size, n_f, _WORDS[field]), names)
    return _plan("pil2gl_debug_range_mult_plan", (n, size, n_f, _WORDS[field], path), names)


def _range(dev, fs, lo, size, m, n, field, row0, path):
    words = _WORDS[field]
    whats = ["f %d" % i for i in range(len(fs))]
    F, ks, keep = _sides(fs, whats, 3, n, words, dev)
    for what, k in zip(whats, ks):
        if k != 1:
            raise Pil2glError("%s: a side of a range check has one column" % what)
    mm, col = _column(m, "m", 1, n, words, dev)
    name = "pil2gl_range_mult" if words == 1 else "pil2gl_bn128_range_mult"
    dev_entry, tail = (name + "_dev", ()) if path is None else ("pil2gl_debug_range_mult_dev", (words, path))
    return _report4(dev, name, dev_entry, [F, len(fs), lo, size, row0] + col + [n], lambda: range_mult_plan(n, size, min(max(len(fs), 1), 8), field, path), mm, *tail)


def range_mult(fs, lo, size, m, n, field="gl", row0=0):
    """the multiplicity column of the range checks `f_s in [lo, lo + size)`: host matrices; m's column is written in place
    -> (kind, side, row, matched)"""
    return _range(False, fs, lo, size, m, n, field, row0, None)


def range_mult_dev(fs, lo, size, m, n, field="gl", row0=0, path=None):
    """range_mult on device tensors, e.g. columns of the stage-1 buffer with m one more column of it; the working buffer comes from the
    plan and lives for the call; blocks for the report"""
    return _range(True, fs, lo, size, m, n, field, row0, path)


# ---- lookup grand sum: the logUp column s from f, t and m (csrc/logup_sum_plan.h; include/pil2gl.h states it) ----
#     lookup_mult_dev([(cm1, [7, 3])], (cm1, [0, 1]), (cm1, 12), n)
#     logup_sum_dev([(cm1, [7, 3], None, 1, bus), (cm1, [0, 1], (cm1, 12), P - 1, bus)], alpha, beta, (cm2, 0), n)
# A term is (matrix, cols, numerator-or-None, coef, bus_id) or that with the matrix's stride as a sixth part; the numerator is a selector
# as above (its FIELD VALUE multiplies coef; for t it is m).  coef and bus_id are integers over Goldilocks (canonical) and 4 Montgomery
# words over Fr; alpha and beta are 3 words of a cubic-extension element, or 4 Montgomery words.  out is (matrix, col) or (matrix, col,
# stride): over Goldilocks a matrix of u64 words whose columns col .. col + 2 take s, over Fr one element column.  Written in place.
def logup_sum_plan(n, n_terms=1, field="gl"):
    """pil2gl_logup_sum_plan (host-only): the launch geometry, the launches and the working bytes"""
    return _plan("pil2gl_logup_sum_plan", (n, n_terms, _WORDS[field]), ("threads", "items", "blocks", "launches", "depth", "outWidth"), "workBytes")


def _elem4(dst, v, words, what):
    """a host base-field element into a uint64[4] field of a term: an integer over Goldilocks, four Montgomery words over Fr"""
    w = np.ascontiguousarray([v] if words == 1 else v, np.uint64).reshape(-1)
    if w.size != words:
        raise Pil2glError("%s is %d words" % (what, words))
    for i in range(words):
        dst[i] = int(w[i])


def _logup_terms(terms, n, words, dev):
    """term specs as a LogupTerm array (one element at least) and what must stay alive until the call returns"""
    from ._lib import LogupTerm
    T = (LogupTerm * max(len(terms), 1))()
    keep = []
    for u, spec in enumerate(terms):
        spec = tuple(spec) + (None,) * (6 - len(spec))
        side, (T[u].k,), kept = _sides([spec], ["term %d" % u], 5, n, words, dev)
        T[u].side = side[0]
        keep.append(kept)
        for name, v in (("coef", spec[3]), ("busId", spec[4])):
            _elem4(getattr(T[u], name), v, words, "term %d: %s" % (u, name))
    return T, keep


def _logup(dev, terms, alpha, beta, out, n, field):
    words = _WORDS[field]
    T, keep = _logup_terms(terms, n, words, dev)
    ch = [np.ascontiguousarray(c, np.uint64).reshape(-1) for c in (alpha, beta)]
    if any(c.size != (3 if words == 1 else 4) for c in ch):
        raise Pil2glError("alpha and beta are %d words each" % (3 if words == 1 else 4))
    om, col = _column(out, "out", 3 if words == 1 else 1, n, words, dev)
    name = "pil2gl_logup_sum" if words == 1 else "pil2gl_bn128_logup_sum"
    args = [T, len(terms), C.c_void_p(ch[0].ctypes.data), C.c_void_p(ch[1].ctypes.data)] + col + [n]
    if dev:
        call(name + "_dev", *args, _stream())
    else:
        call(name, *args)
    return out[0]


def logup_sum(terms, alpha, beta, out, n, field="gl"):
    """the grand-sum column of a lookup: host matrices; out's column is written in place -> out's matrix (s[n-1] is the hint's result)"""
    return _logup(False, terms, alpha, beta, out, n, field)


def logup_sum_dev(terms, alpha, beta, out, n, field="gl"):
    """logup_sum on device tensors, e.g. columns of the stage-1 buffer with m one of them; only enqueues on the current stream"""
    return _logup(True, terms, alpha, beta, out, n, field)


# ---- range-check grand sum: the logUp column s from f, m and the ranges as numbers (csrc/range_sum_plan.h; include/pil2gl.h states it) ----
#     range_mult_dev([(cm1, [7])], -128, 256, (cm1, 12), n)
#     range_sum_dev([(cm1, [7], None, 1, bus)], [((cm1, 12), -128, 256, 0, P - 1, bus)], alpha, beta, (cm2, 0), n)
# The f terms are logup_sum's and may be none (the range table's own AIR).  A range is (m, lo, size, row0, coef, bus_id) with m a column
# (matrix, col) or (matrix, col, stride): no t column exists; outside rows row0 .. row0 + size - 1 the range adds 0 and m is not read.
def range_sum_plan(n, n_f=0, n_r=1, field="gl"):
    """pil2gl_range_sum_plan (host-only): logup_sum_plan's numbers for the same n"""
    return _plan("pil2gl_range_sum_plan", (n, n_f, n_r, _WORDS[field]), ("threads", "items", "blocks", "launches", "depth", "outWidth"), "workBytes")


def _range_terms(ranges, n, words, dev, keep):
    """range specs as a RangeTerm array (one element at least); the m matrices are appended to keep"""
    from ._lib import RangeTerm
    Rg = (RangeTerm * max(len(ranges), 1))()
    for r, (m, lo, size, row0, coef, bus) in enumerate(ranges):
        m = tuple(m) + (None,)
        mm, stride = _side(m[0], [m[1]], m[2], None, n, words, dev, "m of range %d" % r)[:2]
        keep.append(mm)
        Rg[r].m, Rg[r].mStride, Rg[r].mCol = _dev_ptr(dev)(mm), stride, m[1]
        Rg[r].lo, Rg[r].size, Rg[r].row0 = lo, size, row0
        _elem4(Rg[r].coef, coef, words, "range %d: coef" % r)
        _elem4(Rg[r].busId, bus, words, "range %d: busId" % r)
    return Rg


def _range_sum(dev, terms, ranges, alpha, beta, out, n, field):
    words = _WORDS[field]
    T, keep = _logup_terms(terms, n, words, dev)
    Rg = _range_terms(ranges, n, words, dev, keep)
    ch, chp = _challenges((alpha, beta), "alpha and beta", words)
    om, col = _column(out, "out", 3 if words == 1 else 1, n, words, dev)
    name = "pil2gl_range_sum" if words == 1 else "pil2gl_bn128_range_sum"
    args = [T if terms else None, len(terms), Rg, len(ranges)] + chp + col + [n]
    if dev:
        call(name + "_dev", *args, _stream())
    else:
        call(name, *args)
    return out[0]


def range_sum(terms, ranges, alpha, beta, out, n, field="gl"):
    """the grand-sum column of range checks: host matrices; out's column is written in place -> out's matrix (s[n-1] is the hint's result)"""
    return _range_sum(False, terms, ranges, alpha, beta, out, n, field)


def range_sum_dev(terms, ranges, alpha, beta, out, n, field="gl"):
    """range_sum on device tensors, e.g. f and m columns of the stage-1 buffer; only enqueues on the current stream"""
    return _range_sum(True, terms, ranges, alpha, beta, out, n, field)


def range_logup(fs, lo, size, m, alpha, beta, out, n, field="gl", row0=0, bus_id=None):
    """the whole prove side of the range checks `f_s in [lo, lo + size)` on device tensors: range_mult_dev writes m, then range_sum_dev
    writes s with coef 1 for every f side (its selector, a field 0 / 1, the numerator), -1 for the range, and one bus id (0 by default)
    -> (range_mult's report, s[n-1] as a host array of 3 words or of 4 Montgomery words); s[n-1] is zero when the report is clean.  Blocks
    for the report and for s[n-1]."""
    words = _WORDS[field]
    report = range_mult_dev(fs, lo, size, m, n, field, row0)
    terms, rng = _range_logup_terms(fs, lo, size, m, row0, bus_id, words)
    range_sum_dev(terms, [rng], alpha, beta, out, n, field)
    return report, _last_element(out, n, words)


def _range_logup_terms(fs, lo, size, m, row0, bus_id, words):
    """the terms of `f_s in [lo, lo + size)`: coef 1 for every f side, -1 for the range, one bus id (0 by default)"""
    if words == 1:
        one, minus, bus = 1, 0xFFFFFFFF00000000, 0 if bus_id is None else bus_id
    else:
        from .bn128 import _words, R
        one, minus = _words([(1 << 256) % R])[0], _words([R - (1 << 256) % R])[0]
        bus = [0, 0, 0, 0] if bus_id is None else bus_id
    terms = []
    for f in fs:
        f = tuple(f) + (None,) * (4 - len(f))
        terms.append((f[0], f[1], f[2], one, bus, f[3]))
    return terms, (m, lo, size, row0, minus, bus)


def _last_element(out, n, words):
    """s[n-1] of a device column (matrix, col[, stride]) as a host array of 3 words or of 4 Montgomery words; None when n = 0"""
    if not n:
        return None
    width = 3 if words == 1 else 1
    mat, stride = out[0], (out[2] if len(out) > 2 else None)
    flat = mat.reshape(-1)
    if stride is None:
        stride = mat.shape[1]
    at = ((n - 1) * stride + out[1]) * words
    return flat[at:at + width * words].cpu().numpy().view(np.uint64).copy()


# ---- multiplicity sessions: m of a table in an AIR of its own, counted over f sides of their own lengths (csrc/mult_session.hip) ----
#     s = RangeSession(0, 1 << 16)                       # the U16 table's AIR
#     for cm1, n in instances: rep = s.add([(cm1, [7]), (cm1, [4], (cm1, 9))], [n, n])
#     total = s.write((table_cm1, 0), 1 << 16)
# open, add, write of include/pil2gl.h as objects that own the scratch.  A side is lookup_mult's spec, (matrix, cols[, sel[, stride]]), and
# has its own row count; a host array among the sides of an add is staged up for that add.  m is a device column (matrix, col[, stride]).
def _session_plan(entry, args, first, unit):
    p = _plan(entry, args, (first, "threads", "blocks", "launches", "headerBytes", unit))
    w = p.pop("launches")
    return dict(p, openLaunches=w & 255, addLaunches=w >> 8 & 255, writeLaunches=w >> 16 & 255)


def lookup_session_plan(n_t, k, field="gl"):
    """pil2gl_lookup_session_plan (host-only): the table's capacity, the geometry of a full-size count, the launches, the working buffer"""
    return _session_plan("pil2gl_lookup_session_plan", (n_t, k, _WORDS[field]), "capBits", "slotBytes")


def range_session_plan(size, field="gl", path=None):
    """pil2gl_range_session_plan (host-only): the count path, the geometry of a full-size count, the launches, the working buffer"""
    if path is None:
        return _session_plan("pil2gl_range_session_plan", (size, _WORDS[field]), "path", "counterBytes")
    return _session_plan("pil2gl_debug_range_session_plan", (size, _WORDS[field], path), "path", "counterBytes")


def mult_session_grids():
    """pil2gl_debug_mult_session_grids (host-only): the workgroups of the count launch of each of the 8 sides of the last add, 0 for a side
    that launched nothing"""
    out = (C.c_uint32 * 8)()
    load().pil2gl_debug_mult_session_grids(out)
    return [int(x) for x in out]


class _Session:
    def _scratch(self, device):
        self.bytes = self.plan["scratchBytes"]
        self.work = torch.empty(max(self.bytes // 8, 2), dtype=torch.int64, device=device)

    def _f_sides(self, fs, rows, k):
        """the sides of an add as a TupleSide array, each sized against its own rows; host arrays go up for the call"""
        from ._lib import TupleSide
        if len(rows) != len(fs):
            raise Pil2glError("%d sides and %d row counts" % (len(fs), len(rows)))
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.uint64).view(np.int64)).to(self.work.device) if isinstance(a, np.ndarray) else a   # noqa: E731
        arr, keep = (TupleSide * max(len(fs), 1))(), []
        for i, (spec, n) in enumerate(zip(fs, rows)):
            spec = tuple(spec) + (None,) * (4 - len(spec))
            sel = None if spec[2] is None else (up(spec[2][0]),) + tuple(spec[2][1:])
            one, (kk,), kept = _sides([(up(spec[0]), spec[1], sel, spec[3])], ["f %d" % i], 3, n, self.words, True)
            if kk != k:
                raise Pil2glError("f %d has %d columns, %d expected" % (i, kk, k))
            arr[i] = one[0]
            keep.append(kept)
        return arr, np.ascontiguousarray(rows, np.uint64), keep

    def _total(self, entry, args, total):
        out = C.c_uint64()
        call(entry, *args, _ptr(self.work), self.bytes, C.byref(out) if total else None, _stream())
        return out.value if total else None


class LookupSession(_Session):
    """the multiplicities of the lookup table t = (matrix, cols[, sel[, stride]]) of n_t rows, device tensors that stay unchanged while the
    session lives.  seed: the debug open, every counter starting from it."""

    def __init__(self, t, n_t, field="gl", seed=None):
        self.words, self.n_t = _WORDS[field], n_t
        self.T, (self.k,), self._keep = _sides([t], ["t"], 3, n_t, self.words, True)
        self.plan = lookup_session_plan(n_t, self.k, field)
        self._scratch(self._keep[0].device)
        self._name = "pil2gl_lookup_session_%s_dev" if self.words == 1 else "pil2gl_bn128_lookup_session_%s_dev"
        head = [self.T, n_t, self.k, _ptr(self.work), self.bytes, _stream()]
        if seed is None:
            call(self._name % "open", *head)
        else:
            call("pil2gl_debug_lookup_session_open_dev", *head, self.words, seed)

    def add(self, fs, rows):
        """counts the sides fs, side i over its first rows[i] rows -> this add's (kind, side, row, matched); blocks"""
        F, R, keep = self._f_sides(fs, rows, self.k)
        rep = (C.c_uint64 * 4)()
        call(self._name % "add", self.T, self.n_t, self.k, F, C.c_void_p(R.ctypes.data), len(fs), _ptr(self.work), self.bytes, rep, _stream())
        return tuple(int(x) for x in rep)

    def write(self, m, total=True):
        """m = (matrix, col[, stride]), a device column of n_t rows -> the session's matched rows; total=False only enqueues -> None"""
        mm, col = _column(m, "m", 1, self.n_t, self.words, True)
        return self._total(self._name % "write", [self.T, self.n_t, self.k] + col, total)


class RangeSession(_Session):
    """the multiplicities of the range table [lo, lo + size).  path: the count kernel of every add, for the tests and the benchmark
    (0 LDS, 1 global, None the planner's choice); seed: the debug open."""

    def __init__(self, lo, size, field="gl", path=None, seed=None, device="cuda"):
        self.words, self.lo, self.size, self.path, self.k = _WORDS[field], lo, size, path, 1
        self.plan = range_session_plan(size, field, path)
        self._scratch(device)
        self._name = "pil2gl_range_session_%s_dev" if self.words == 1 else "pil2gl_bn128_range_session_%s_dev"
        if seed is None:
            call("pil2gl_range_session_open_dev", size, _ptr(self.work), self.bytes, _stream())
        else:
            call("pil2gl_debug_range_session_open_dev", size, _ptr(self.work), self.bytes, _stream(), seed)

    def add(self, fs, rows):
        """counts the one-column sides fs, side i over its first rows[i] rows -> this add's (kind, side, row, matched); blocks"""
        F, R, keep = self._f_sides(fs, rows, 1)
        rep = (C.c_uint64 * 4)()
        args = [self.lo, self.size, F, C.c_void_p(R.ctypes.data), len(fs), _ptr(self.work), self.bytes, rep, _stream()]
        if self.path is None:
            call(self._name % "add", *args)
        else:
            call("pil2gl_debug_range_session_add_dev", *args, self.words, self.path)
        return tuple(int(x) for x in rep)

    def write(self, m, n_m, row0=0, total=True):
        """m = (matrix, col[, stride]), a device column of n_m rows: the counts at rows row0 .. row0 + size - 1, 0 elsewhere -> the session's
        matched rows; total=False only enqueues -> None"""
        mm, col = _column(m, "m", 1, n_m, self.words, True)
        return self._total(self._name % "write", [self.size, row0] + col + [n_m], total)


def range_logup_cross(users, lo, size, m, n_table, alpha, beta, outs, out_table, field="gl", row0=0, bus_id=None):
    """one range table AIR and several user AIRs end to end, on device tensors.  users: (fs, n) per user AIR, fs range_mult's sides over
    that AIR's n rows.  One RangeSession takes one add per user AIR and writes m, a column of the table AIR's n_table rows; every user's s
    is logup_sum_dev with f terms only, into outs[i]; the table's s is range_sum_dev with no f term, into out_table
    -> (the adds' reports, the session's matched rows, the last element of every s, users first).  The last elements sum to zero in the
    field (the cubic extension over Goldilocks) when every report is clean."""
    words = _WORDS[field]
    session = RangeSession(lo, size, field, device=m[0].device)
    reports = [session.add(fs, [n] * len(fs)) for fs, n in users]
    total = session.write(m, n_table, row0)
    last = []
    for (fs, n), out in zip(users, outs):
        terms, rng = _range_logup_terms(fs, lo, size, m, row0, bus_id, words)
        logup_sum_dev(terms, alpha, beta, out, n, field)
        last.append(_last_element(out, n, words))
    range_sum_dev([], [_range_logup_terms([], lo, size, m, row0, bus_id, words)[1]], alpha, beta, out_table, n_table, field)
    last.append(_last_element(out_table, n_table, words))
    return reports, total, last


# ---- clustered logUp sum: s and one im column a cluster in one call (csrc/logup_cluster_plan.h; include/pil2gl.h states it) ----
#     logup_cluster_dev([(cm1, [7], None, 1, bus), (cm1, [8], None, 1, bus)], [((cm1, 12), -128, 256, 0, P - 1, bus)], [0, 0, DIRECT],
#                       [(cm2, 3)], alpha, beta, (cm2, 0), n)
# terms and ranges are logup_sum's and range_sum's (either may be empty, nine together at most); cluster holds one entry a term, f terms
# first: a cluster id 0 .. len(im) - 1, or DIRECT for a term that stays in the sum constraint; im holds one column (matrix, col) or
# (matrix, col, stride) a cluster, of out's shape.  s and the im columns as neighbouring columns of one matrix is the normal case.
DIRECT = (1 << 64) - 1


def logup_cluster_plan(n, n_f=1, n_r=0, n_im=1, field="gl"):
    """pil2gl_logup_cluster_plan (host-only): threads a workgroup, rows a lane, workgroups, launches, depth, words of an output element,
    working bytes"""
    return _plan("pil2gl_logup_cluster_plan", (n, n_f, n_r, n_im, _WORDS[field]), ("threads", "items", "blocks", "launches", "depth", "outWidth"), "workBytes")


def _logup_cluster(dev, terms, ranges, cluster, im, alpha, beta, out, n, field):
    from ._lib import LogupImCol
    words = _WORDS[field]
    T, keep = _logup_terms(terms, n, words, dev)
    Rg = _range_terms(ranges, n, words, dev, keep)
    cl = np.ascontiguousarray([int(c) for c in cluster], np.uint64).reshape(-1)
    if cl.size != len(terms) + len(ranges):
        raise Pil2glError("cluster holds %d entries for %d terms and ranges" % (cl.size, len(terms) + len(ranges)))
    width = 3 if words == 1 else 1
    Im = (LogupImCol * max(len(im), 1))()
    for c, spec in enumerate(im):
        mm, col = _column(spec, "im %d" % c, width, n, words, dev)
        keep.append(mm)
        Im[c].base, Im[c].stride, Im[c].col = col
    ch, chp = _challenges((alpha, beta), "alpha and beta", words)
    om, col = _column(out, "out", width, n, words, dev)
    name = "pil2gl_logup_cluster" if words == 1 else "pil2gl_bn128_logup_cluster"
    args = [T if terms else None, len(terms), Rg if ranges else None, len(ranges), C.c_void_p(cl.ctypes.data), Im, len(im)] + chp + col + [n]
    if dev:
        call(name + "_dev", *args, _stream())
    else:
        call(name, *args)
    return out[0]


def logup_cluster(terms, ranges, cluster, im, alpha, beta, out, n, field="gl"):
    """s and the im columns of a clustered logUp sum: host matrices, every output column written in place -> out's matrix"""
    return _logup_cluster(False, terms, ranges, cluster, im, alpha, beta, out, n, field)


def logup_cluster_dev(terms, ranges, cluster, im, alpha, beta, out, n, field="gl"):
    """logup_cluster on device tensors, e.g. s and the im columns as columns of the stage-2 buffer; only enqueues on the current stream"""
    return _logup_cluster(True, terms, ranges, cluster, im, alpha, beta, out, n, field)


def range_logup_clustered(fs, lo, size, m, cluster, im, alpha, beta, out, n, field="gl", row0=0, bus_id=None):
    """range_logup with the terms clustered: range_mult_dev writes m, then logup_cluster_dev writes s and the im columns, with coef 1 for
    every f side and -1 for the range; cluster holds an entry for every f side, then the range's -> (range_mult's report, s[n-1] as a host
    array).  Blocks for the report and for s[n-1]."""
    words = _WORDS[field]
    report = range_mult_dev(fs, lo, size, m, n, field, row0)
    terms, rng = _range_logup_terms(fs, lo, size, m, row0, bus_id, words)
    logup_cluster_dev(terms, [rng], cluster, im, alpha, beta, out, n, field)
    return report, _last_element(out, n, words)


# ---- grand product: the column z of a permutation or a connection (csrc/grand_prod_plan.h; include/pil2gl.h states it) ----
#     perm_prod_dev((cm1, [7, 3], (cm1, 9)), (cm1, [4, 5], (cm1, 10)), alpha, beta, gamma, (cm2, 0), n)
#     conn_prod_dev([(cm1, 0), (cm1, 1)], [(const, 4), (const, 5)], (x, 0), ks, gamma, delta, (cm2, 0), n)
# A term is (matrix, cols, selector-or-None, den, id-or-None, id_coef) or that with the matrix's stride as a seventh part; den is 0 for a
# factor of the numerator and 1 for one of the denominator; id is a column as a selector is, (matrix, col) or (matrix, col, stride), and
# id_coef its coefficient: 3 canonical words over Goldilocks, 4 Montgomery words over Fr (None with no id).  alpha, beta, gamma are 3
# words of a cubic-extension element, or 4 Montgomery words.  out is logup_sum's.  Written in place; z[n-1] is the hint's result.
def grand_prod_plan(n, n_terms=1, sum_k=None, field="gl"):
    """pil2gl_grand_prod_plan (host-only): the launch geometry, the launches and the working bytes"""
    names = ("threads", "items", "blocks", "launches", "depth", "outWidth")
    return _plan("pil2gl_grand_prod_plan", (n, n_terms, n_terms if sum_k is None else sum_k, _WORDS[field]), names, "workBytes")


def _grand_prod(dev, terms, alpha, beta, gamma, out, n, field):
    from ._lib import GrandProdTerm
    words = _WORDS[field]
    cw = 3 if words == 1 else 4
    T = (GrandProdTerm * max(len(terms), 1))()
    keep = []
    for u, spec in enumerate(terms):
        spec = tuple(spec) + (None,) * (7 - len(spec))
        side, (T[u].k,), kept = _sides([(spec[0], spec[1], spec[2], spec[6])], ["term %d" % u], 3, n, words, dev)
        T[u].side = side[0]
        T[u].den = int(spec[3] or 0)
        keep.append(kept)
        if spec[4] is not None:
            idc = tuple(spec[4]) + (None,)
            idm, id_stride = _side(idc[0], [idc[1]], idc[2], None, n, words, dev, "the id of term %d" % u)[:2]
            keep.append(idm)
            T[u].id, T[u].idStride, T[u].idCol = _dev_ptr(dev)(idm), id_stride, idc[1]
            w = np.ascontiguousarray(spec[5], np.uint64).reshape(-1)
            if w.size != cw:
                raise Pil2glError("term %d: idCoef is %d words" % (u, cw))
            for i in range(cw):
                T[u].idCoef[i] = int(w[i])
    ch = [np.ascontiguousarray(c, np.uint64).reshape(-1) for c in (alpha, beta, gamma)]
    if any(c.size != cw for c in ch):
        raise Pil2glError("alpha, beta and gamma are %d words each" % cw)
    om, col = _column(out, "out", 3 if words == 1 else 1, n, words, dev)
    name = "pil2gl_grand_prod" if words == 1 else "pil2gl_bn128_grand_prod"
    args = [T, len(terms)] + [C.c_void_p(c.ctypes.data) for c in ch] + col + [n]
    if dev:
        call(name + "_dev", *args, _stream())
    else:
        call(name, *args)
    return out[0]


def grand_prod(terms, alpha, beta, gamma, out, n, field="gl"):
    """the grand-product column of a permutation or a connection: host matrices; out's column is written in place -> out's matrix"""
    return _grand_prod(False, terms, alpha, beta, gamma, out, n, field)


def grand_prod_dev(terms, alpha, beta, gamma, out, n, field="gl"):
    """grand_prod on device tensors, e.g. columns of the stage-1 buffer and of the constants; only enqueues on the current stream"""
    return _grand_prod(True, terms, alpha, beta, gamma, out, n, field)


def perm_terms(f, t):
    """the two terms of `selF {f} is selT {t}` (grandProductPermutation.js): f, t = (matrix, cols[, sel[, stride]])"""
    f, t = (tuple(s) + (None, None) for s in (f, t))
    return [(f[0], f[1], f[2], 0, None, None, f[3]), (t[0], t[1], t[2], 1, None, None, t[3])]


def conn_terms(a_cols, S_cols, x, ks, delta, field="gl"):
    """the 2 len(a_cols) terms of `{a} connect {S}` (grandProductConnection.js): a_cols, S_cols = lists of (matrix, col[, stride]), x = the
    column of the domain's points, ks = the cosets' shifts k_1 .. (column 0 takes 1), delta = the challenge's words.  Builds lists only: the
    one product here is delta ks'_j, by the library's scalar multiply over Goldilocks and on the Montgomery words as integers over Fr"""
    if len(S_cols) != len(a_cols) or len(ks) < len(a_cols) - 1:
        raise Pil2glError("a connection of %d columns takes as many S columns and %d shifts" % (len(a_cols), len(a_cols) - 1))
    delta = [int(v) for v in np.ascontiguousarray(delta, np.uint64).reshape(-1)]
    terms = []
    for j, (a, S) in enumerate(zip(a_cols, S_cols)):
        k = 1 if j == 0 else int(ks[j - 1])
        if _WORDS[field] == 1:
            coef = [int(load().pil2gl_mul(d, k)) for d in delta]
        else:
            from .bn128 import _ints, _words
            coef = _words([_ints(delta)[0] * k])[0]
        a = tuple(a) + (None,)
        terms.append((a[0], [a[1]], None, 0, x, coef, a[2]))
        terms.append((a[0], [a[1]], None, 1, S, delta, a[2]))
    return terms


def perm_prod(f, t, alpha, beta, gamma, out, n, field="gl"):
    """z of one permutation, host matrices: grand_prod over perm_terms(f, t)"""
    return grand_prod(perm_terms(f, t), alpha, beta, gamma, out, n, field)


def perm_prod_dev(f, t, alpha, beta, gamma, out, n, field="gl"):
    return grand_prod_dev(perm_terms(f, t), alpha, beta, gamma, out, n, field)


def conn_prod(a_cols, S_cols, x, ks, gamma, delta, out, n, field="gl"):
    """z of one connection, host matrices: grand_prod over conn_terms(..); alpha and beta are unused by its terms and passed as gamma"""
    return grand_prod(conn_terms(a_cols, S_cols, x, ks, delta, field), gamma, gamma, gamma, out, n, field)


def conn_prod_dev(a_cols, S_cols, x, ks, gamma, delta, out, n, field="gl"):
    return grand_prod_dev(conn_terms(a_cols, S_cols, x, ks, delta, field), gamma, gamma, gamma, out, n, field)


# ---- plookup: pil1's lookup argument from the trace columns, h1 and h2 (csrc/plookup_plan.h; include/pil2gl.h states it) ----
#     F, T = plookup_fold_dev((cm1, [7, 3], (cm1, 9)), (const, [4, 5], (const, 10)), alpha, beta, (work, 0), (work, 3), n)
#     h1, h2 = plookup_h1h2_dev((cm1, [7, 3], (cm1, 9)), (const, [4, 5], (const, 10)), alpha, beta, n)
#     plookup_prod_dev(f, t, (cm2, 0), (cm2, 3), alpha, beta, gamma, delta, (cm3, 0), n)
# f and t are sides (matrix, cols[, sel[, stride]]) with their own column counts; h1, h2 and the outputs are columns (matrix, col) or
# (matrix, col, stride) of h_dim words an element (Goldilocks 1 or 3; Fr one element); the challenges are 3 words of a cubic-extension
# element, or 4 Montgomery words.  Written in place; z[n-1] is the hint's result.
def plookup_plan(n, k_f=1, k_t=1, field="gl"):
    """pil2gl_plookup_plan (host-only): the product call's launch geometry, its launches and its working bytes"""
    names = ("threads", "items", "blocks", "launches", "depth", "outWidth")
    return _plan("pil2gl_plookup_plan", (n, k_f, k_t, _WORDS[field]), names, "workBytes")


def _plookup_sides(f, t, n, words, dev):
    sides, ks, keep = _sides([f, t], ["f", "t"], 3, n, words, dev)
    return [C.pointer(sides[0]), ks[0], C.pointer(sides[1]), ks[1]], (sides, keep)


def _challenges(chs, names, words):
    cw = 3 if words == 1 else 4
    ch = [np.ascontiguousarray(c, np.uint64).reshape(-1) for c in chs]
    if any(c.size != cw for c in ch):
        raise Pil2glError("%s are %d words each" % (names, cw))
    return ch, [C.c_void_p(c.ctypes.data) for c in ch]


def _plookup_fold(dev, f, t, alpha, beta, out_f, out_t, n, field, h_dim):
    words = _WORDS[field]
    sides, keep = _plookup_sides(f, t, n, words, dev)
    ch, chp = _challenges((alpha, beta), "alpha and beta", words)
    width = h_dim if words == 1 else 1
    cols = _column(out_f, "outF", width, n, words, dev)[1] + _column(out_t, "outT", width, n, words, dev)[1]
    name = "pil2gl_plookup_fold" if words == 1 else "pil2gl_bn128_plookup_fold"
    args = sides + chp + [h_dim] + cols + [n]
    if dev:
        call(name + "_dev", *args, _stream())
    else:
        call(name, *args)
    return out_f[0], out_t[0]


def plookup_fold(f, t, alpha, beta, out_f, out_t, n, field="gl", h_dim=None):
    """the two kept expressions F and T of a plookup (its stage-1 half): host matrices; the two columns are written in place -> their
    matrices.  h_dim defaults to 3 over Goldilocks and is 1 over Fr"""
    return _plookup_fold(False, f, t, alpha, beta, out_f, out_t, n, field, (3 if field == "gl" else 1) if h_dim is None else h_dim)


def plookup_fold_dev(f, t, alpha, beta, out_f, out_t, n, field="gl", h_dim=None):
    """plookup_fold on device tensors; only enqueues on the current stream"""
    return _plookup_fold(True, f, t, alpha, beta, out_f, out_t, n, field, (3 if field == "gl" else 1) if h_dim is None else h_dim)


def _plookup_prod(dev, f, t, h1, h2, alpha, beta, gamma, delta, out, n, field, h_dim):
    words = _WORDS[field]
    sides, keep = _plookup_sides(f, t, n, words, dev)
    ch, chp = _challenges((alpha, beta, gamma, delta), "alpha, beta, gamma and delta", words)
    width = h_dim if words == 1 else 1
    hcols = []
    for h, what in ((h1, "h1"), (h2, "h2")):
        h = tuple(h) + (None,)
        hm, hs = _side(h[0], [h[1] + width - 1], h[2], None, n, words, dev, what)[:2]
        keep = (keep, hm)
        hcols += [_dev_ptr(dev)(hm), hs, h[1]]
    om, col = _column(out, "out", 3 if words == 1 else 1, n, words, dev)
    name = "pil2gl_plookup_prod" if words == 1 else "pil2gl_bn128_plookup_prod"
    args = sides + hcols + [h_dim] + chp + col + [n]
    if dev:
        call(name + "_dev", *args, _stream())
    else:
        call(name, *args)
    return out[0]


def plookup_prod(f, t, h1, h2, alpha, beta, gamma, delta, out, n, field="gl", h_dim=None):
    """the grand-product column z of a plookup (its stage-2 half) from f, t, h1 and h2: host matrices; out's column is written in place
    -> out's matrix.  h_dim defaults to 3 over Goldilocks and is 1 over Fr"""
    return _plookup_prod(False, f, t, h1, h2, alpha, beta, gamma, delta, out, n, field, (3 if field == "gl" else 1) if h_dim is None else h_dim)


def plookup_prod_dev(f, t, h1, h2, alpha, beta, gamma, delta, out, n, field="gl", h_dim=None):
    """plookup_prod on device tensors, e.g. columns of the stage buffers with z spare columns of one of them; only enqueues on the current
    stream"""
    return _plookup_prod(True, f, t, h1, h2, alpha, beta, gamma, delta, out, n, field, (3 if field == "gl" else 1) if h_dim is None else h_dim)


def _plookup_h1h2(dev, f, t, alpha, beta, n, field, h_dim):
    """fold into scratch, then the field's own h1h2: a value of F that is not in T comes back as that call reports it"""
    import pil2gl
    from . import bn128
    if field == "gl":
        h_dim = 3 if h_dim is None else h_dim
        if dev:
            like = f[0]
            F = torch.empty(n * h_dim, dtype=torch.int64, device=like.device)
            T = torch.empty_like(F)
            _plookup_fold(True, f, t, alpha, beta, (F, 0, h_dim), (T, 0, h_dim), n, field, h_dim)
            return pil2gl.calculateH1H2(F, T, h_dim)
        F = np.zeros((n, h_dim), np.uint64)
        T = np.zeros((n, h_dim), np.uint64)
        _plookup_fold(False, f, t, alpha, beta, (F, 0), (T, 0), n, field, h_dim)
        h1, h2 = pil2gl.calculateH1H2(torch.from_numpy(F.view(np.int64).reshape(-1)).cuda(), torch.from_numpy(T.view(np.int64).reshape(-1)).cuda(), h_dim)
        return tuple(h.cpu().numpy().view(np.uint64).reshape(n, h_dim) for h in (h1, h2))
    if dev:
        FT = torch.empty((n, 2, 4), dtype=torch.int64, device=f[0].device)
    else:
        FT = np.zeros((n, 2, 4), np.uint64)
    _plookup_fold(dev, f, t, alpha, beta, (FT, 0), (FT, 1), n, field, 1)
    flat = FT.reshape(-1)
    return bn128.h1h2(flat, flat[4:], n, 2, 2)


def plookup_h1h2(f, t, alpha, beta, n, field="gl", h_dim=None):
    """h1 and h2 of a plookup from the trace columns, host matrices: plookup_fold into scratch, then calculateH1H2 of the field (over
    Goldilocks that one is resident: F and T go up for it and h1, h2 come back) -> (h1, h2) as new arrays"""
    return _plookup_h1h2(False, f, t, alpha, beta, n, field, h_dim)


def plookup_h1h2_dev(f, t, alpha, beta, n, field="gl", h_dim=None):
    """plookup_h1h2 on device tensors -> (h1, h2) as new dense device columns; blocks as the field's h1h2 does, for the missing row"""
    return _plookup_h1h2(True, f, t, alpha, beta, n, field, h_dim)
