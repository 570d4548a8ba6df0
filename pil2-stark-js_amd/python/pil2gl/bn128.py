"""Host-side mirror of the reference's BN128 Merkle commitment modules over libpil2gl (no arithmetic of its own):
  buildMerkleHash(arity, custom)  <-> src/helpers/hash/merklehash/merklehash_bn128_p.js:10-285
  LinearHashBN                    <-> src/helpers/hash/linearhash/linearhash.bn128.js:4-62
  Transcript                      <-> src/helpers/transcript/transcript.bn128.js:1-106
  poseidon(inputs, initState, nOut) <-> circomlibjs buildPoseidon() as the reference calls it
  fft / ifft / interpolate        <-> src/helpers/fft/fft_p.bn128.js:178-285 (Montgomery words in and out)
  g1_msm                          <-> G1.toAffine(G1.multiExpAffine(bases, scalars)) of ffjavascript, the fflonk commit
  g1_commit                       <-> the G1 points of fflonk's commit(stage, ...): several packed polynomials (CPolynomial) in one call,
                                      read as columns of the coefficient matrix ifft left
  encode_program / eval_program / first_nonzero_row
                                  <-> src/prover/prover_helpers.js:31-259 calculateExps over ctx.F = curve.Fr (Montgomery words in and out)
  poly_div / poly_eval / poly_plan <-> Polynomial.divZh / divByXNSubValue / evaluate as fflonk_prover_helpers.js:147-148, :212 use them
  poly_fma / poly_degree          <-> Polynomial.add / sub / mulScalar / byXSubValue / byXNSubValue / degree as shplonkjs open (:212) uses them
  batch_inverse / gprod / gsum / gsum_col / scan_plan
                                  <-> F.batchInverse, calculateZ, calculateS of src/helpers/polutils.js:132-164 over curve.Fr, as
                                      hints_helpers.js:92-113 resolves gprod / gsum hints (Montgomery words in and out)
  h1h2 / h1h2_plan                <-> calculateH1H2 of src/helpers/polutils.js:105-130 over curve.Fr, the h1h2 hint (hints_helpers.js:115-121)
Field elements cross this API as Python ints in normal form (the JS modules use BigInt / F.toObject)."""
import ctypes as C

import numpy as np

from ._lib import Pil2glError, G1Poly, load, call
from . import _is_dev, _ptr, _stream, _check_len, _same_side, _to_host, torch

R = 21888242871839275222246405745257275088548364400416034343698204186575808495617


def _words(vals, keep256=False):
    """the 4 words of every value reduced mod r; keep256 leaves values < 2^256 as they are (the library reduces them mod r)"""
    a = np.zeros((len(vals), 4), np.uint64)
    for i, v in enumerate(vals):
        v = int(v)
        if not (keep256 and 0 <= v < (1 << 256)):
            v %= R
        for k in range(4):
            a[i, k] = (v >> (64 * k)) & 0xFFFFFFFFFFFFFFFF
    return a


def _ints(words):
    w = np.asarray(words, dtype=np.uint64).reshape(-1, 4)
    return [sum(int(x) << (64 * k) for k, x in enumerate(r)) for r in w]


def _dispatch(name, buf, *args):
    """the library's entry `name` over host buffers, or its `_dev` twin on the current stream where `buf` is a device tensor"""
    if _is_dev(buf):
        call(name + "_dev", *args, _stream())
    else:
        call(name, *args)


def _new_like(like, shape):
    """a new buffer of this shape and of the kind of `like`: a tensor next to it, or a numpy array of words"""
    if _is_dev(like):
        return torch.empty(shape, dtype=like.dtype, device=like.device)
    return np.empty(shape, np.uint64)


def poseidon(inputs, initState=0, nOut=1):
    if not 1 <= len(inputs) <= 16:
        raise Pil2glError("BN128 Poseidon takes 1..16 inputs")
    i = _words(inputs); s = _words([initState]); o = np.zeros((nOut, 4), np.uint64)
    call("pil2gl_bn128_poseidon", _ptr(i), _ptr(s), 1, len(inputs), nOut, _ptr(o))
    return _ints(o)


def poseidon_chain(blocks, initState=0):
    """blocks: [nBlocks][nIn] ints absorbed one after the other, each permutation's output 0 being the next one's state
    element 0 (transcript.bn128.js:56-66) -> the nIn+1 outputs of the last permutation; one launch, nIn+1 lanes"""
    nB, nIn = len(blocks), len(blocks[0])
    i = _words([v for row in blocks for v in row]); s = _words([initState]); o = np.zeros((nIn + 1, 4), np.uint64)
    call("pil2gl_bn128_sponge_absorb", _ptr(i), nB, nIn, _ptr(s), _ptr(o))
    return _ints(o)


def poseidon_batch(inputs, init=None, nOut=1):
    """inputs: [count][nIn] ints, init: [count] ints or None -> [count][nOut] ints"""
    count, nIn = len(inputs), len(inputs[0])
    i = _words([v for row in inputs for v in row]); s = _words(init) if init is not None else None
    o = np.zeros((count * nOut, 4), np.uint64)
    call("pil2gl_bn128_poseidon", _ptr(i), _ptr(s), count, nIn, nOut, _ptr(o))
    flat = _ints(o)
    return [flat[k * nOut:(k + 1) * nOut] for k in range(count)]


def from_montgomery(words):
    w = np.ascontiguousarray(words, dtype=np.uint64).reshape(-1, 4); o = np.zeros_like(w)
    call("pil2gl_bn128_convert", _ptr(w), w.shape[0], 0, _ptr(o))
    return _ints(o)


def to_montgomery(vals):
    w = _words(vals); o = np.zeros_like(w)
    call("pil2gl_bn128_convert", _ptr(w), w.shape[0], 1, _ptr(o))
    return o


def _transform(name, words, nPols, nBits, out):
    _same_side(words, out)
    _check_len(words, (nPols << nBits) * 4, "words")
    if out is None:
        out = _new_like(words, words.shape)
    _check_len(out, (nPols << nBits) * 4, "out")
    _dispatch(name, words, _ptr(words), nPols, nBits, _ptr(out))
    return out


def fft(words, nPols, nBits, out=None):
    """fft_p.bn128.js:178: words = (2^nBits, nPols, 4) uint64 Montgomery words, a numpy array or a device tensor; the result (natural
    order, Montgomery words) is a new buffer of the same kind, or `out` (which may be `words`)"""
    return _transform("pil2gl_bn128_fft", words, nPols, nBits, out)


def ifft(words, nPols, nBits, out=None):
    """fft_p.bn128.js:182"""
    return _transform("pil2gl_bn128_ifft", words, nPols, nBits, out)


def interpolate(words, nPols, nBits, nBitsExt, coefs=True):
    """fft_p.bn128.js:225: -> (coefficients (2^nBits, nPols, 4), evaluations on the 2^nBitsExt roots (2^nBitsExt, nPols, 4)), no coset
    shift; coefs=False skips the first output (None in its place)"""
    _check_len(words, (nPols << nBits) * 4, "words")
    ext = _new_like(words, (1 << nBitsExt, nPols, 4))
    co = _new_like(words, (1 << nBits, nPols, 4)) if coefs else None
    _dispatch("pil2gl_bn128_interpolate", words, _ptr(words), nPols, nBits, _ptr(co), _ptr(ext), nBitsExt)
    return co, ext


def g1_msm(bases, scalars, n=None, stride=1, montgomery=True, out=None):
    """G1.toAffine(G1.multiExpAffine(bases, scalars)): bases = n affine points of 8 uint64 words (x, y in Fq Montgomery form, infinity all
    zero), scalars = element i at word 4*i*stride (Fr Montgomery words, or normal form with montgomery=False); numpy arrays or device
    tensors, both of one kind.  n defaults to the number of points in bases.  -> the affine sum as 8 words of the same kind, or `out`"""
    _same_side(bases, scalars, out)
    if n is None:
        n = int(np.prod(bases.shape)) // 8
    if stride < 1:
        raise Pil2glError("stride must be at least 1")
    _check_len(bases, 8 * n, "bases")
    _check_len(scalars, ((n - 1) * stride + 1) * 4 if n else 0, "scalars")
    if out is None:
        out = _new_like(bases, 8)
    _check_len(out, 8, "out")
    _dispatch("pil2gl_bn128_g1_msm", bases, _ptr(bases), _ptr(scalars), n, stride, 1 if montgomery else 0, _ptr(out))
    return out


EMPTY_SLOT = 0xFFFFFFFF


def g1_commit(bases, scalars, polys, row_stride, montgomery=True, out=None):
    """The commitments of K packed polynomials over the same bases in one call.  scalars = a row-major matrix of Fr elements (4 words
    each), row_stride elements per row; polys = [(first, rows, slots)]: polynomial k has len(slots) * rows coefficients, coefficient i is
    the element first + (i div m) * row_stride + slots[i mod m], or 0 where that slot is None (fflonk's CPolynomial).  numpy arrays or
    device tensors, all of one kind.  -> (K, 8) words of the same kind, or `out`: toAffine(sum_i coef_k[i] * bases[i]) per polynomial"""
    _same_side(bases, scalars, out)
    K = len(polys)
    descs, flat, extent, n_max = (G1Poly * max(K, 1))(), [], 0, 0
    for k, (first, rows, slots) in enumerate(polys):
        first, rows = int(first), int(rows)
        if first < 0 or rows < 0:
            raise Pil2glError("polynomial %d: negative first or rows" % k)
        descs[k].first, descs[k].rows, descs[k].m = first, rows, len(slots)
        cols = [int(c) for c in slots if c is not None]
        if any(c < 0 or c >= EMPTY_SLOT for c in cols):
            raise Pil2glError("polynomial %d: bad column index" % k)
        flat += [EMPTY_SLOT if c is None else int(c) for c in slots]
        n_max = max(n_max, rows * len(slots))
        if rows and cols:
            extent = max(extent, first + (rows - 1) * int(row_stride) + max(cols) + 1)
    n_bases = int(np.prod(bases.shape)) // 8
    if n_max > n_bases:
        raise Pil2glError("a polynomial of %d coefficients, bases hold %d points" % (n_max, n_bases))
    _check_len(scalars, 4 * extent, "scalars")         # the C entry cannot know how far the buffers extend
    c_slots = (C.c_uint32 * max(len(flat), 1))(*flat)
    if out is None:
        out = _new_like(bases, (K, 8))
    _check_len(out, 8 * K, "out")
    _dispatch("pil2gl_bn128_g1_commit", bases,
              _ptr(bases), n_bases, _ptr(scalars), int(row_stride), 1 if montgomery else 0, descs, K, c_slots, _ptr(out))
    return out


# ---- calculateExps over Fr: prover_helpers.js:31-72, :83-107 compileCode, :109-259 setRef / getRef / evalMap ----
OPC = {"add": 0, "sub": 1, "mul": 2, "copy": 3}
TMP, SEC, SCALAR = 0, 1, 2


def encode_program(code, ctx, dom, is_global=False):
    """The reference's `code.code` (a list of {op, dest, src[]}) as op tuples (op, dest, src0, src1) of refs (kind, dim, section, prime,
    index), following getRef / setRef / evalMap as they run with ctx.prover === "fflonk": every element is one Fr element, so dim is 1.
    ctx: {"pilInfo": {cmPolsMap, mapSectionsN, nConstants, boundaries}, "publics", "challenges", "subproofValues"} with the scalars as
    Montgomery words (4 uint64 each), the form ctx.F keeps them in.  number{value} becomes F.e(value) through pil2gl_bn128_convert.
    -> (ops, nTmp, sections, scalars): sections = [(name, width, ziIndex or None)] in the order the ops number them, name being the
    ctx member the reference reads ("const_n", "cm1_ext", "x_n", "Zi_ext", "q_ext", ...); scalars = (nScalars, 4) uint64."""
    info = ctx["pilInfo"]
    sections, sec_index, words, numbers = [], {}, [], {}

    def section(name, width, zi=None):
        key = (name, zi)
        if key not in sec_index:
            sec_index[key] = len(sections)
            sections.append((name, width, zi))
        return sec_index[key]

    def scalar(w):
        w = np.asarray(w, dtype=np.uint64).reshape(4)
        words.append(w)
        return (SCALAR, 1, 0, 0, len(words) - 1)

    def ref(r, dest):
        t = r["type"]
        if r.get("dim", 1) != 1:
            raise Pil2glError("dim %s: Fr elements have dim 1" % r.get("dim"))
        if t == "tmp":
            return (TMP, 1, 0, 0, r["id"])
        if t == "cm":                                           # evalMap, prover_helpers.js:220-259
            p = info["cmPolsMap"][r["id"]]
            st = "cm%d" % p["stage"]
            return (SEC, 1, section(st + "_" + dom, info["mapSectionsN"][st]), r.get("prime", 0) or 0, p["stagePos"])
        if t == "q" and dest:                                   # prover_helpers.js:115-129
            if dom != "ext":
                raise Pil2glError("Accessing q in domain n")
            return (SEC, 1, section("q_ext", 1), 0, 0)
        if dest:
            raise Pil2glError("Invalid reference type set: " + t)
        if t == "const":
            return (SEC, 1, section("const_" + dom, info["nConstants"]), r.get("prime", 0) or 0, r["id"])
        if t == "x":
            return (SEC, 1, section("x_" + dom, 1), 0, 0)
        if t == "Zi":                                           # prover_helpers.js:202-215
            bs = info["boundaries"]
            b = bs[r["boundaryId"]]
            if b["name"] == "everyFrame":
                zi = [k for k, o in enumerate(bs) if o["name"] == "everyFrame" and o.get("offsetMin") == b.get("offsetMin") and o.get("offsetMax") == b.get("offsetMax")]
            elif b["name"] in ("everyRow", "firstRow", "lastRow"):
                zi = [k for k, o in enumerate(bs) if o["name"] == b["name"]]
            else:
                raise Pil2glError("Invalid boundary: " + b["name"])
            if not zi:
                raise Pil2glError("Something went wrong")
            return (SEC, 1, section("Zi_ext", 1, zi[0]), 0, 0)
        if t == "number":
            v = int(r["value"]) % R                             # F.e: a negative value is value + r
            if v not in numbers:
                numbers[v] = scalar(to_montgomery([v])[0])
            return numbers[v]
        if t == "public":
            return scalar(ctx["publics"][r["id"]])
        if t == "challenge":
            return scalar(ctx["challenges"][r["stage"] - 1][r["stageId"]])
        if t == "subproofValue":
            return scalar(ctx["subproofValues"][r["subproofId"]][r["id"]] if is_global else ctx["subproofValues"][r["id"]])
        raise Pil2glError("Invalid reference type get: " + t)

    ops, n_tmp = [], 0
    for c in code:
        if c["op"] not in OPC:
            raise Pil2glError("Invalid op:" + c["op"])
        for r in [c["dest"]] + list(c["src"]):
            if r["type"] == "tmp":
                n_tmp = max(n_tmp, r["id"] + 1)
        src = [ref(r, False) for r in c["src"]]
        ops.append((OPC[c["op"]], ref(c["dest"], True), src[0], src[1] if c["op"] != "copy" else None))
    return ops, n_tmp, sections, np.array(words, dtype=np.uint64).reshape(-1, 4)


def make_context(ops, n_tmp, sections, scalars, nBits, primeShift, widths=None):
    """-> (glx_program, bnx_ctx) for the library's entries: what eval_program builds per call, for callers that call more than once"""
    from . import _lib
    from .stark import make_c_program
    prog = make_c_program(ops, n_tmp if n_tmp is not None else 1 + max([r[4] for o in ops for r in o[1:] if r is not None and r[0] == TMP], default=-1))
    cs = (_lib.GlxSection * max(len(sections), 1))()
    for i, b in enumerate(sections):
        if b is not None and (len(b.shape) != 3 or b.shape[2] != 4 or b.shape[0] != 1 << nBits):
            raise Pil2glError("section %d must have shape (2^nBits, width, 4)" % i)
        cs[i].ptr = None if b is None else _ptr(b).value
        cs[i].width = widths[i] if widths is not None else b.shape[1]
    sc = np.ascontiguousarray(scalars if scalars is not None else np.zeros((0, 4)), dtype=np.uint64).reshape(-1, 4)
    ctx = _lib.BnxCtx(nBits, primeShift, len(sections), sc.shape[0], cs, sc.ctypes.data_as(_lib.u64p) if sc.size else None)
    ctx._keep = (cs, sc)
    return prog, ctx


def eval_program(code, sections, scalars, nBits, primeShift=0, nTmp=None):
    """calculateExps(ctx, code, dom) over Fr for every row of a domain of 2^nBits rows (primeShift = 0 on "n", nBitsExt - nBits on "ext").
    code = op tuples as encode_program returns them; sections = one buffer per section index, each (2^nBits, width, 4) uint64 Montgomery
    words, all numpy arrays or all device tensors (then the kernel is enqueued on the current stream); scalars = (nScalars, 4) uint64
    Montgomery words, always a numpy array.  Destination sections are written in place."""
    _same_side(*sections)
    prog, ctx = make_context(code, nTmp, sections, scalars, nBits, primeShift)
    _dispatch("pil2gl_bn128_eval_program", next((b for b in sections if b is not None), None), C.byref(prog), C.byref(ctx))


def plan_program(code, widths, scalars, nBits, primeShift=0, nTmp=None):
    """pil2gl_debug_bn128_plan_program (no device): how eval_program would run `code` on sections of these widths ->
    {slots, ops, form (0 LDS / 1 global), ldsSlotLimit, lanesPerLaunch, threads}"""
    fake = np.zeros(4, np.uint64)                               # a non-null pointer that is never read
    prog, ctx = make_context(code, nTmp, [None] * len(widths), scalars, nBits, primeShift, widths)
    for i in range(len(widths)):
        ctx.sections[i].ptr = fake.ctypes.data
    info = (C.c_uint32 * 6)()
    call("pil2gl_debug_bn128_plan_program", C.byref(prog), C.byref(ctx), info)
    return dict(zip(("slots", "ops", "form", "ldsSlotLimit", "lanesPerLaunch", "threads"), (int(v) for v in info)))


def first_nonzero_row(section, column, first, last):
    """calculateExps with debug = true (prover_helpers.js:46-70): section = a device tensor (rows, width, 4) whose column `column` holds a
    constraint's values -> (row, value words) of the smallest row of [first, last) that is not zero, or None"""
    if not _is_dev(section) or len(section.shape) != 3 or section.shape[2] != 4:
        raise Pil2glError("section must be a device tensor of shape (rows, width, 4)")
    if not 0 <= first <= last <= section.shape[0] or not 0 <= column < section.shape[1]:
        raise Pil2glError("column %d, rows [%d, %d) of a section of %d rows x %d columns" % (column, first, last, section.shape[0], section.shape[1]))
    row = C.c_uint64(); val = np.zeros(4, np.uint64)
    call("pil2gl_bn128_first_nonzero_row_dev", _ptr(section), section.shape[1], column, first, last, C.byref(row), _ptr(val), _stream())
    return None if row.value == 0xFFFFFFFFFFFFFFFF else (int(row.value), val)


# ---- division by x^k - beta and evaluation: Q.divZh of computeQFflonk, the long-vector work of shplonkjs open ----
def _host_elems(a, what, most=None):
    a = np.ascontiguousarray(a, dtype=np.uint64).reshape(-1, 4)
    if a.shape[0] < 1 or (most is not None and a.shape[0] > most):
        raise Pil2glError("%s: %d elements" % (what, a.shape[0]))
    return a


def _column(buf, n, stride, what):
    """-> the rows of a column: n, or what `buf` holds at this stride; checks the stride and the length"""
    if stride < 1:
        raise Pil2glError("stride must be at least 1")
    if n is None:
        n = (int(np.prod(buf.shape)) // 4 + stride - 1) // stride
    _check_len(buf, ((n - 1) * stride + 1) * 4 if n else 0, what)
    return n


def poly_div(words, k, beta, n=None, stride=1, out=None):
    """d[i] = c[i] + beta d[i + k] over the coefficients `words` (element i at word 4*i*stride, Montgomery words; a numpy array or a
    device tensor): d[k..n) is the quotient by x^k - beta (coefficient m at m + k), d[0..k) the remainder.  beta = 4 Montgomery words
    on the host.  n defaults to the elements `words` holds at this stride.  -> a new buffer of the same kind and shape, or `out` (which
    may be `words`; with stride > 1 the words between its elements stay as they are, so give one)"""
    _same_side(words, out)
    n = _column(words, n, stride, "words")
    if out is None:
        if stride != 1:
            raise Pil2glError("a strided division writes into a matrix: pass out")
        out = _new_like(words, words.shape)
    _column(out, n, stride, "out")
    b = _host_elems(beta, "beta", 1)
    _dispatch("pil2gl_bn128_poly_div_xk_sub", words, _ptr(words), n, stride, k, _ptr(b), _ptr(out))
    return out


def poly_eval(words, points, n=None, stride=1):
    """sum_i c[i] z^i for every z of `points` ((P, 4) Montgomery words on the host, 1 <= P <= 64) over the coefficients `words` (as
    poly_div takes them; never written) -> (P, 4) Montgomery words of the same kind as `words`"""
    n = _column(words, n, stride, "words")
    z = _host_elems(points, "points", 64)
    out = _new_like(words, (z.shape[0], 4))
    _dispatch("pil2gl_bn128_poly_eval", words, _ptr(words), n, stride, _ptr(z), z.shape[0], _ptr(out))
    return out


def poly_plan(n, k):
    """pil2gl_debug_bn128_poly_plan (no device): how poly_div runs (n, k), and poly_eval (n, 1) ->
    {L, S, levels, threads, form (0 a lane per chain / 1 segmented), scratchBytes}"""
    info = (C.c_uint32 * 5)(); nbytes = C.c_uint64()
    call("pil2gl_debug_bn128_poly_plan", n, k, info, C.byref(nbytes))
    d = dict(zip(("L", "S", "levels", "threads", "form"), (int(v) for v in info)))
    d["scratchBytes"] = int(nbytes.value)
    return d


# ---- products with a sparse polynomial, scaled sums, degree: Polynomial.add / sub / mulScalar / byXSubValue / byXNSubValue / degree ----
def poly_fma(acc, src, coefs, exps, scale=None, *, n_acc, n_src, acc_stride=1, src_stride=1):
    """acc[i] <- scale acc[i] + sum_j coefs[j] src[i - exps[j]] for i < n_acc, src zero outside [0, n_src): the product of src by the
    sparse polynomial sum_j coefs[j] x^exps[j], added to the scaled accumulator (shplonkjs open, fflonk_prover_helpers.js:212).  acc and
    src are columns (element i at word 4*i*stride, Montgomery words; numpy arrays or device tensors of one kind; src may be None with
    n_src = 0); coefs = (t, 4) Montgomery words and exps = t strictly increasing exponents, 1 <= t <= 64, on the host; scale = 4
    Montgomery words on the host, or None: then acc is written and never read.  n_src + exps[-1] <= n_acc.  acc must share no element
    with src, except as the same column when exps == [0].  -> acc"""
    _same_side(acc, src)
    _column(acc, n_acc, acc_stride, "acc")
    if src is None and n_src:
        raise Pil2glError("src is None with n_src = %d" % n_src)
    _column(src, n_src, src_stride, "src")
    m = np.ascontiguousarray(coefs, dtype=np.uint64).reshape(-1, 4)
    e = np.ascontiguousarray(exps, dtype=np.uint64).reshape(-1)
    if m.shape[0] != e.shape[0]:
        raise Pil2glError("%d coefficients for %d exponents" % (m.shape[0], e.shape[0]))
    s = None if scale is None else _host_elems(scale, "scale", 1)
    _dispatch("pil2gl_bn128_poly_fma", acc,
              _ptr(acc), n_acc, acc_stride, _ptr(s), _ptr(src), n_src, src_stride, _ptr(m), _ptr(e), e.shape[0])
    return acc


def poly_degree(words, n=None, stride=1):
    """Polynomial.degree: the largest i whose element (at word 4*i*stride) is not zero, or None for the zero polynomial and for n = 0"""
    n = _column(words, n, stride, "words")
    d = C.c_uint64()
    _dispatch("pil2gl_bn128_poly_degree", words, _ptr(words), n, stride, C.byref(d))
    return None if d.value == (1 << 64) - 1 else int(d.value)


# ---- gprod / gsum hints over Fr: calculateZ, calculateS and F.batchInverse (polutils.js:132-164, hints_helpers.js:92-113) ----
SCAN_OPS = {"batch_inverse": 0, "gprod": 1, "gsum": 2, "batch_inverse_in_place": 3}


def _out_column(like, n, stride, out):
    """-> `out` checked as a column of n rows, or a new dense one of the kind of `like`"""
    if out is None:
        if stride != 1:
            raise Pil2glError("a strided result is written into a matrix: pass out")
        out = _new_like(like, (n, 4))
    _column(out, n, stride, "out")
    return out


def batch_inverse(words, n=None, stride=1, out=None, out_stride=None):
    """F.batchInverse: out[i] = words[i]^-1, a zero giving zero (element i at word 4*i*stride, Montgomery words; a numpy array or a device
    tensor).  n defaults to the elements `words` holds at this stride.  -> a new buffer of the same kind, or `out` (element i at word
    4*i*out_stride, out_stride defaulting to stride; `out` may be `words` itself at the same stride, and nothing else that overlaps it)"""
    _same_side(words, out)
    n = _column(words, n, stride, "words")
    out_stride = stride if out_stride is None else out_stride
    out = _out_column(words, n, out_stride, out)
    _dispatch("pil2gl_bn128_batch_inverse", words, _ptr(words), stride, n, _ptr(out), out_stride)
    return out


def gprod(num, den, n=None, num_stride=1, den_stride=1, out=None, out_stride=1):
    """calculateZ(F, num, den): out[0] = 1, out[i] = out[i-1] num[i-1] / den[i-1] (Montgomery words; columns as batch_inverse takes them,
    each with its own stride; numpy arrays or device tensors, all of one kind).  A zero denominator makes its ratio 0.  n defaults to the
    elements `den` holds.  -> a new buffer of the same kind, or `out` (which must not overlap num or den); out[n-1] is the hint's result"""
    _same_side(num, den, out)
    n = _column(den, n, den_stride, "den")
    _column(num, n, num_stride, "num")
    out = _out_column(den, n, out_stride, out)
    _dispatch("pil2gl_bn128_gprod", den, _ptr(num), num_stride, _ptr(den), den_stride, n, _ptr(out), out_stride)
    return out


def gsum(num_elem, den, n=None, den_stride=1, out=None, out_stride=1):
    """calculateS(F, num, den): out[i] = out[i-1] + num / den[i] with num ONE element, 4 Montgomery words on the host; den and out as
    gprod takes them.  A zero denominator adds 0."""
    if _is_dev(num_elem):
        raise Pil2glError("num_elem is one element on the host")
    _same_side(den, out)
    n = _column(den, n, den_stride, "den")
    out = _out_column(den, n, out_stride, out)
    e = _host_elems(num_elem, "num_elem", 1)
    _dispatch("pil2gl_bn128_gsum", den, _ptr(e), _ptr(den), den_stride, n, _ptr(out), out_stride)
    return out


def gsum_col(num, den, n=None, num_stride=1, den_stride=1, out=None, out_stride=1):
    """calculateS with a COLUMN numerator: out[i] = out[i-1] + num[i] / den[i]; columns, strides, zeros and aliasing as gprod's"""
    _same_side(num, den, out)
    n = _column(den, n, den_stride, "den")
    _column(num, n, num_stride, "num")
    out = _out_column(den, n, out_stride, out)
    _dispatch("pil2gl_bn128_gsum_col", den, _ptr(num), num_stride, _ptr(den), den_stride, n, _ptr(out), out_stride)
    return out


def scan_plan(n, op="gprod"):
    """pil2gl_debug_bn128_scan_plan (no device): how batch_inverse / gprod / gsum run n rows (op: a key of SCAN_OPS or its number) ->
    {L rows per segment, S segments, levels, threads, segsPerWorkgroup, scratchBytes}"""
    info = (C.c_uint32 * 5)(); nbytes = C.c_uint64()
    call("pil2gl_debug_bn128_scan_plan", n, SCAN_OPS.get(op, op), info, C.byref(nbytes))
    d = dict(zip(("L", "S", "levels", "threads", "segsPerWorkgroup"), (int(v) for v in info)))
    d["scratchBytes"] = int(nbytes.value)
    return d


# ---- the plookup hint over Fr: calculateH1H2 (polutils.js:105-130, hints_helpers.js:115-121) ----
def h1h2(f, t, n=None, f_stride=1, t_stride=1, h1=None, h1_stride=1, h2=None, h2_stride=1):
    """calculateH1H2(F, f, t): the multiset f merged into t -- t[i] repeated 1 + cnt[i] times, the counts of a duplicated value at its LAST
    occurrence -- and read as h1[i] = s[2i], h2[i] = s[2i+1].  Elements are compared as their 32 bytes (Montgomery words, never converted);
    columns as gprod takes them, each with its own stride; numpy arrays or device tensors, all of one kind.  n defaults to the elements
    `t` holds.  -> (h1, h2): new buffers of the same kind, or the ones passed (which must overlap nothing but as columns of one section).
    A value of f that is not in t raises Pil2glError with "Number not included: w:<lowest such row>"; the outputs are untouched then."""
    _same_side(f, t, h1, h2)
    n = _column(t, n, t_stride, "t")
    _column(f, n, f_stride, "f")
    h1 = _out_column(t, n, h1_stride, h1)
    h2 = _out_column(t, n, h2_stride, h2)
    miss = C.c_uint64()
    args = (_ptr(f), f_stride, _ptr(t), t_stride, n, _ptr(h1), h1_stride, _ptr(h2), h2_stride, C.byref(miss))
    try:
        _dispatch("pil2gl_bn128_h1h2", t, *args)
    except Pil2glError as e:
        e.missing_row = None if miss.value == (1 << 64) - 1 else int(miss.value)      # the library's missingRow
        raise
    return h1, h2


def h1h2_plan(n):
    """pil2gl_debug_bn128_h1h2_plan (no device): how h1h2 runs n rows -> {capacity (table slots), threads, scanChunk (groups per
    workgroup of the local scan), scanBlocks, expandRows (output rows per workgroup of the expand step), expandBlocks, scratchBytes}"""
    info = (C.c_uint32 * 6)(); nbytes = C.c_uint64()
    call("pil2gl_debug_bn128_h1h2_plan", n, info, C.byref(nbytes))
    d = dict(zip(("capacity", "threads", "scanChunk", "scanBlocks", "expandRows", "expandBlocks"), (int(v) for v in info)))
    d["scratchBytes"] = int(nbytes.value)
    return d


class LinearHashBN:
    """linearhash.bn128.js: hash(vals) -> Fr (normal form int)"""

    def __init__(self, arity, custom):
        self.arity, self.custom = int(arity), bool(custom)

    def hash(self, vals):
        flat = []
        for v in vals:
            if isinstance(v, (list, tuple, np.ndarray)):
                flat.extend(int(x) for x in v)
            else:
                flat.append(int(v))
        el = [sum(x << (64 * k) for k, x in enumerate(flat[i:i + 3])) % R for i in range(0, len(flat), 3)]
        if not el:
            return 0
        if len(el) == 1:
            return el[0]
        st = 0
        for i in range(0, len(el), self.arity):                 # linearhash.bn128.js:46-57
            chunk = el[i:i + self.arity]
            if len(chunk) < self.arity and self.custom:
                chunk = chunk + [0] * (self.arity - len(chunk))
            st = poseidon(chunk, st, 1)[0]
        return st


class MerkleHashBN128:
    """merklehash_bn128_p.js:16-285.  tree = {elements, nodes, width, height}; nodes = u64 words, Montgomery form."""

    def __init__(self, arity=16, custom=False):
        if arity not in (2, 4, 8, 16):
            raise Pil2glError("arity must be 2, 4, 8 or 16")
        self.arity, self.custom = int(arity), bool(custom)
        self.lh = LinearHashBN(arity, custom)
        load()

    def _getNNodes(self, n):
        return int(load().pil2gl_bn128_merkle_num_nodes(n, self.arity))

    def merkelize(self, buff, width, height):
        if height <= 0:
            raise Pil2glError("height must be > 0")
        _check_len(buff, width * height, "buff")
        n_words = self._getNNodes(height) * 4
        nodes = torch.empty(n_words, dtype=torch.int64, device=buff.device) if _is_dev(buff) else np.zeros(n_words, np.uint64)
        _dispatch("pil2gl_bn128_merkelize", buff, _ptr(buff), width, height, self.arity, int(self.custom), _ptr(nodes))
        return {"elements": buff, "nodes": nodes, "width": width, "height": height}

    def root(self, tree):
        last = tree["nodes"][-4:]
        if _is_dev(last):
            last = last.cpu().numpy().view(np.uint64)
        return from_montgomery(last)[0]

    def getGroupProof(self, tree, idx):
        if idx < 0 or idx >= tree["height"]:
            raise Pil2glError("Out of range")
        width, height, a = tree["width"], tree["height"], self.arity
        if _is_dev(tree["nodes"]):
            vals = np.zeros(max(width, 1), np.uint64); sib = np.zeros((64, a, 4), np.uint64); nl = C.c_uint32()
            call("pil2gl_bn128_group_proof_dev", _ptr(tree["elements"]), _ptr(tree["nodes"]), width, height, a, idx,
                 _ptr(vals), _ptr(sib), C.byref(nl))
            return [int(v) for v in vals[:width]], [_ints(sib[l]) for l in range(nl.value)]
        el = tree["elements"].reshape(-1)
        v = [int(x) for x in el[idx * width:(idx + 1) * width]]
        nodes = tree["nodes"].reshape(-1, 4); nbits = (a - 1).bit_length()
        mp, offset, n = [], 0, height
        while n > 1:                                            # merklehash_bn128_p.js:155-181
            si = idx ^ (idx & (a - 1))
            grp = from_montgomery(nodes[offset + si:offset + si + a])
            mp.append([g if i < n else 0 for i, g in enumerate(grp)])
            nxt = (n - 1) // a + 1
            offset += nxt * a; n = nxt; idx >>= nbits
        return v, mp

    def getGroupProofs(self, tree, idxs):
        """getGroupProof for a batch of rows of a device-resident tree in one launch (pil2gl_bn128_group_proofs_dev); host trees: one by one"""
        idxs = [int(i) for i in idxs]
        if not idxs or not _is_dev(tree["nodes"]):
            return [self.getGroupProof(tree, i) for i in idxs]
        width, height, a, n = tree["width"], tree["height"], self.arity, len(idxs)
        if any(i < 0 or i >= height for i in idxs):
            raise Pil2glError("Out of range")
        ii = np.array(idxs, dtype=np.uint64)
        vals = np.zeros((n, max(width, 1)), np.uint64); nl = C.c_uint32()
        sib_flat = np.zeros(n * 40 * a * 4, np.uint64)
        call("pil2gl_bn128_group_proofs_dev", _ptr(tree["elements"]), _ptr(tree["nodes"]), width, height, a, _ptr(ii), n,
             _ptr(vals), _ptr(sib_flat), C.byref(nl))
        lv = nl.value
        v2 = vals.reshape(-1)[:n * width].reshape(n, width).tolist() if width else [[] for _ in range(n)]
        s2 = sib_flat[:n * lv * a * 4].reshape(n, lv, a, 4)
        return [(v2[q], [_ints(s2[q, l]) for l in range(lv)]) for q in range(n)]

    def calculateRootFromGroupProof(self, mp, idx, vals):
        value = self.lh.hash(vals)                              # merklehash_bn128_p.js:184-232
        nbits = (self.arity - 1).bit_length()
        for sibs in mp:
            cur = idx & (self.arity - 1)
            idx >>= nbits
            group = [int(s) % R for s in sibs]
            group[cur] = value
            value = poseidon(group, 0, 1)[0]
        return value

    def calculateRootsFromGroupProofs(self, proofs, idxs):
        """calculateRootFromGroupProof for a batch of openings [(vals, siblings), ...] of one tree: packing, leaf sponge and every
        level of every opening in ONE launch (pil2gl_bn128_roots_from_group_proofs: a wave per opening walks its whole path)"""
        if not proofs:
            return []
        flat = []
        for vals, _ in proofs:
            f = []
            for v in vals:
                f.extend(int(x) for x in v) if isinstance(v, (list, tuple, np.ndarray)) else f.append(int(v))
            flat.append(f)
        if len({len(f) for f in flat}) != 1 or len({len(mp) for _, mp in proofs}) != 1:
            raise Pil2glError("openings of different shapes in one batch")
        n, width, levels, a = len(proofs), len(flat[0]), len(proofs[0][1]), self.arity
        if any(len(g) != a for _, mp in proofs for g in mp):
            raise Pil2glError("a level's group must hold `arity` siblings")
        vals = np.array(flat, dtype=np.uint64).reshape(n, width)
        sib = _words([s_ for _, mp in proofs for g in mp for s_ in g], keep256=True)
        ii = np.array([int(i) for i in idxs], dtype=np.uint64)
        roots = np.zeros((n, 4), np.uint64)
        call("pil2gl_bn128_roots_from_group_proofs", _ptr(vals) if width else None, _ptr(sib) if levels else None, width, levels, a,
             int(self.custom), 0, _ptr(ii), n, _ptr(roots))
        return _ints(roots)

    def verifyGroupProofs(self, root, proofs, idxs):
        return all(self.eqRoot(r, root) for r in self.calculateRootsFromGroupProofs(proofs, idxs))

    def eqRoot(self, r1, r2):
        return int(r1) == int(r2)

    def verifyGroupProof(self, root, mp, idx, groupElements):
        return self.eqRoot(self.calculateRootFromGroupProof(mp, idx, groupElements), root)

    def writeToFile(self, tree, fileName):
        """merklehash_bn128_p.js:243-263: [width u64][height u64][elements][nodes]"""
        with open(fileName, "wb") as f:
            np.array([tree["width"], tree["height"]], dtype="<u8").tofile(f)
            _to_host(tree["elements"]).astype("<u8", copy=False).tofile(f)
            _to_host(tree["nodes"]).astype("<u8", copy=False).tofile(f)

    def readFromFile(self, fileName, device=None):
        with open(fileName, "rb") as f:
            width, height = (int(v) for v in np.fromfile(f, dtype="<u8", count=2))
            elements = np.fromfile(f, dtype="<u8", count=width * height).astype(np.uint64)
            nodes = np.fromfile(f, dtype="<u8", count=self._getNNodes(height) * 4).astype(np.uint64)
        if device is not None:
            elements = torch.from_numpy(elements.view(np.int64)).to(device)
            nodes = torch.from_numpy(nodes.view(np.int64)).to(device)
        return {"elements": elements, "nodes": nodes, "width": width, "height": height}


def buildMerkleHash(arity=16, custom=False):
    """merklehash_bn128_p.js:10"""
    return MerkleHashBN128(arity, custom)


class Transcript:
    """transcript.bn128.js:1-106 over the device permutation"""

    def __init__(self, nInputs=16):
        self.nInputs, self.state = nInputs, 0
        self.pending, self.out, self.out3 = [], [], []

    def getState(self):
        if self.pending:
            self.updateState()
        return self.state

    def getField(self):
        return [self.getFields1(), self.getFields1(), self.getFields1()]

    def getFields1(self):
        if self.out3:
            return self.out3.pop(0)
        if self.out:
            v = self.out.pop(0)
            self.out3 = [v & 0xFFFFFFFFFFFFFFFF, (v >> 64) & 0xFFFFFFFFFFFFFFFF, (v >> 128) & 0xFFFFFFFFFFFFFFFF]
            return self.getFields1()
        self.updateState()
        return self.getFields1()

    def getFields253(self):
        if self.out:
            return self.out.pop(0)
        self.updateState()
        return self.getFields253()

    def updateState(self):
        while len(self.pending) < self.nInputs:
            self.pending.append(0)
        self.out = poseidon(self.pending, self.state, self.nInputs + 1)
        self.out3, self.pending = [], []
        self.state = self.out[0]

    def put(self, a):
        flat = []

        def walk(v):
            if isinstance(v, (list, tuple)):
                for x in v:
                    walk(x)
            else:
                flat.append(int(v) % R)
        walk(a)
        if not flat:
            return
        n = self.nInputs
        if (len(self.pending) + len(flat)) // n >= 2:      # a chain of dependent permutations: one launch for all of them
            allv = self.pending + flat
            nb = len(allv) // n
            self.out = poseidon_chain([allv[k * n:(k + 1) * n] for k in range(nb)], self.state)
            self.state, self.out3, self.pending = self.out[0], [], allv[nb * n:]
            if self.pending:
                self.out = []
            return
        for v in flat:
            self.out = []
            self.pending.append(v)
            if len(self.pending) == n:
                self.updateState()

    def getPermutations(self, n, nBits):
        total = n * nBits
        fields = [self.getFields253() for _ in range((total - 1) // 253 + 1)]
        res, cf, cb = [], 0, 0
        for _ in range(n):
            a = 0
            for j in range(nBits):
                if (fields[cf] >> cb) & 1:
                    a += 1 << j
                cb += 1
                if cb == 253:
                    cb = 0; cf += 1
            res.append(a)
        return res
