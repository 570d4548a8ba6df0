"""The recursion witness on the device: the `*_exec` step of the reference -- compressorExec (src/compressor/compressor_exec.js:5-32)
over Goldilocks, the loop of src/final/main_final_exec.js:50-67 over the BN254 scalar field -- through csrc/wtns_exec.hip.

    exec_ = read_exec_file("c12a.exec", 12, "gl")            # or (path, nCols, "bn128") for a final .exec
    trace = exec_gl(w, exec_)                                # host arrays in, the N x nCols trace out
    prep = prepare(exec_)                                    # the circuit's constant tables into HBM, once
    trace = exec_dev(prep, w_dev)                            # per proof: w_dev holds the witness in its first nWitness elements

Goldilocks elements are uint64 words, Fr elements 4 words; the Fr witness is in normal form (a .wtns' values), the trace comes out in
Montgomery form unless montgomery=False.  No arithmetic happens here: the planner, the additions and the gather are the library's.

The same resident sMap drives the setups' connection polynomials (csrc/conn_pols.hip), the constant columns S of the copy constraints:

    S = conn_pols(s_map, n_cols, N, w, ks)                   # host arrays in, the (N, nCols) columns out
    S = conn_pols_dev(prep, N, w, ks)                        # from what prepare() left in HBM, into a device matrix

and whether a trace meets the copy constraints those columns state (csrc/conn_check.hip), the connection half of pilcom's verifyPil:

    bad = conn_check(a, S, n_cols, N, w, ks)                 # host arrays in; None, or the first failing cell, its partner and the kind
    bad = conn_check_dev(trace, S, n_cols, N, w, ks)         # on the device matrices exec_dev and conn_pols_dev wrote
"""
import ctypes as C
import os
import struct

import numpy as np

from ._lib import Pil2glError, call
from . import _is_dev, _ptr, _stream, torch

_U32P = C.POINTER(C.c_uint32)
_WORDS = {"gl": 1, "bn128": 4}


def _np_ptr(a):
    return C.c_void_p(a.ctypes.data) if a is not None and a.size else None


def _strides(field):
    """(idxStride, coefStride) of the tables as the files hold them"""
    return (4, 4) if field == "gl" else (2, 8)


def _tables(exec_):
    """(operand table, coefficient table) as the plan reads them"""
    if exec_["field"] == "gl":
        adds = np.ascontiguousarray(exec_["adds"], np.uint64).reshape(-1)
        return adds, adds[2:] if adds.size else adds
    return np.ascontiguousarray(exec_["addsIdx"], np.uint64).reshape(-1), np.ascontiguousarray(exec_["addsCoef"], np.uint64).reshape(-1)


def adds_plan(add_idx, n_witness, coefs=None, coef_words=1, idx_stride=2, coef_stride=None):
    """pil2gl_wtns_adds_plan (host-only): -> {"adds": (nAdds, 4) uint32 records (a, b, dst, source position) sorted by level, "coefs": the
    coefficients permuted alike (None without `coefs`), "levelStart": uint32[nLevels + 1], "nLevels"}"""
    add_idx = np.ascontiguousarray(add_idx, np.uint64).reshape(-1)
    n_adds = (add_idx.size + idx_stride - 2) // idx_stride if add_idx.size else 0
    coef_stride = coef_stride or 2 * coef_words
    if coefs is not None:
        coefs = np.ascontiguousarray(coefs, np.uint64).reshape(-1)
        if n_adds and coefs.size < (n_adds - 1) * coef_stride + 2 * coef_words:
            raise Pil2glError("coefs holds %d words, %d additions need %d" % (coefs.size, n_adds, (n_adds - 1) * coef_stride + 2 * coef_words))
    n = C.c_uint32()
    call("pil2gl_wtns_adds_plan", _np_ptr(add_idx), idx_stride, n_adds, n_witness, None, 0, coef_words, None, None, None, 0, C.byref(n))
    recs = np.zeros((n_adds, 4), np.uint32)
    out_coef = np.zeros(2 * coef_words * n_adds, np.uint64) if coefs is not None else None
    start = np.zeros(n.value + 1, np.uint32)
    call("pil2gl_wtns_adds_plan", _np_ptr(add_idx), idx_stride, n_adds, n_witness, _np_ptr(coefs), coef_stride, coef_words,
         _np_ptr(recs), _np_ptr(out_coef), _np_ptr(start), start.size, C.byref(n))
    return {"adds": recs, "coefs": out_coef, "levelStart": start, "nLevels": n.value}


def plan_info(add_idx, n_witness, idx_stride=2):
    """pil2gl_debug_wtns_plan (host-only): levels, launches, the levels' widths"""
    add_idx = np.ascontiguousarray(add_idx, np.uint64).reshape(-1)
    n_adds = (add_idx.size + idx_stride - 2) // idx_stride if add_idx.size else 0
    info = (C.c_uint32 * 5)()
    call("pil2gl_debug_wtns_plan", _np_ptr(add_idx), idx_stride, n_adds, n_witness, info, None, 0)
    widths = np.zeros(info[0], np.uint32)
    call("pil2gl_debug_wtns_plan", _np_ptr(add_idx), idx_stride, n_adds, n_witness, info, _np_ptr(widths), widths.size)
    return {"levels": info[0], "launches": info[1], "widest": info[2], "threads": info[3], "widestBlocks": info[4], "widths": [int(x) for x in widths]}


def _exec_host(name, w, exec_, words, *tail):
    w = np.ascontiguousarray(w, np.uint64).reshape(-1)
    if w.size % words:
        raise Pil2glError("w holds %d words, no multiple of %d" % (w.size, words))
    idx, coef = _tables(exec_)
    s_map = np.ascontiguousarray(exec_["sMap"], np.uint64).reshape(-1)
    n_rows, n_cols = exec_["nSMap"], exec_["nCols"]
    if s_map.size != n_rows * n_cols:
        raise Pil2glError("sMap holds %d entries, %d x %d expected" % (s_map.size, n_rows, n_cols))
    shape = (n_rows, n_cols) if words == 1 else (n_rows, n_cols, 4)
    dst = np.zeros(shape, np.uint64)
    call(name, _np_ptr(w), w.size // words, _np_ptr(idx), _np_ptr(coef), exec_["nAdds"], _np_ptr(s_map), n_rows, n_cols, _np_ptr(dst), *tail)
    return dst


def exec_gl(w, exec_):
    """compressorExec with the witness in place of the wasm: w = uint64[nWitness] -> the (nSMap, nCols) trace, canonical"""
    return _exec_host("pil2gl_wtns_exec", w, exec_, 1)


def exec_bn128(w, exec_, montgomery=True):
    """main_final_exec.js:50-67: w = (nWitness, 4) normal-form words -> the (nSMap, nCols, 4) trace, Montgomery words by default"""
    return _exec_host("pil2gl_bn128_wtns_exec", w, exec_, 4, 1 if montgomery else 0)


def _to_dev(a):
    """bytes of a host table as a device tensor of whole words (the tail padded with zeros)"""
    raw = a.tobytes()
    raw += b"\0" * (-len(raw) % 16)
    return torch.from_numpy(np.frombuffer(raw, np.int64).copy()).cuda()


def prepare(exec_, n_witness=None):
    """the circuit's constant tables into HBM, once per setup: the levelled additions, their coefficients and the sMap as 32-bit indices.
    n_witness: the circuit's witness length (or exec_["nWitness"]).  An sMap value that names no signal is refused here, as the host form
    refuses it."""
    exec_ = dict(exec_, nWitness=exec_["nWitness"] if n_witness is None else n_witness)
    field = exec_["field"]
    words = _WORDS[field]
    idx, coef = _tables(exec_)
    si, sc = _strides(field)
    n_adds, n_rows, n_cols = exec_["nAdds"], exec_["nSMap"], exec_["nCols"]
    p = adds_plan(idx, exec_["nWitness"], coef, words, si, sc)
    s_map = np.ascontiguousarray(exec_["sMap"], np.uint64).reshape(-1)
    n_w = exec_["nWitness"] + n_adds
    if s_map.size != n_rows * n_cols:
        raise Pil2glError("sMap holds %d entries, %d x %d expected" % (s_map.size, n_rows, n_cols))
    bad = np.flatnonzero(s_map >= n_w)
    if bad.size:
        raise Pil2glError("sMap[%d] = %d names no signal (nWitness + nAdds = %d)" % (bad[0], s_map[bad[0]], n_w))
    return {"field": field, "nWitness": exec_["nWitness"], "nAdds": n_adds, "nW": n_w, "nRows": n_rows, "nCols": n_cols,
            "adds": _to_dev(p["adds"]), "coefs": _to_dev(p["coefs"]), "sMap": _to_dev(s_map.astype(np.uint32)),
            "levelStart": p["levelStart"], "nLevels": p["nLevels"]}


def adds_dev(prep, w_dev):
    """the additions in place: w_dev = device tensor of nW elements whose first nWitness hold the witness; enqueues on the current stream"""
    name = "pil2gl_wtns_adds_dev" if prep["field"] == "gl" else "pil2gl_bn128_wtns_adds_dev"
    if w_dev.numel() < prep["nW"] * _WORDS[prep["field"]]:
        raise Pil2glError("w holds %d words, nW = %d elements needed" % (w_dev.numel(), prep["nW"]))
    call(name, _ptr(w_dev), prep["nWitness"], _ptr(prep["adds"]), _ptr(prep["coefs"]), prep["nAdds"],
         prep["levelStart"].ctypes.data_as(C.c_void_p), prep["nLevels"], _stream())


def gather_dev(prep, w_dev, dst=None, dst_cols=None, montgomery=True, check=False, s_map=None):
    """the fill: -> dst, a (nRows, dstCols[, 4]) device tensor (given or new); check=True blocks and returns (dst, firstBad) with
    firstBad None when every index names a signal.  s_map: another device table of nRows x nCols 32-bit indices in place of prep's."""
    words = _WORDS[prep["field"]]
    dst_cols = dst_cols or prep["nCols"]
    n = prep["nRows"] * dst_cols * words
    if dst is None:
        dst = torch.empty((prep["nRows"], dst_cols) + ((4,) if words == 4 else ()), dtype=w_dev.dtype, device=w_dev.device)
    if dst.numel() < n:
        raise Pil2glError("dst holds %d words, %d needed" % (dst.numel(), n))
    bad = C.c_uint64()
    args = [_ptr(w_dev), prep["nW"], _ptr(s_map if s_map is not None else prep["sMap"]), prep["nRows"], prep["nCols"], _ptr(dst), dst_cols]
    if words == 4:
        args.append(1 if montgomery else 0)
    call("pil2gl_wtns_gather_dev" if words == 1 else "pil2gl_bn128_wtns_gather_dev", *args, C.byref(bad) if check else None, _stream())
    if check:
        return dst, (None if bad.value == 0xFFFFFFFFFFFFFFFF else bad.value)
    return dst


def exec_dev(prep, w_dev, dst=None, dst_cols=None, montgomery=True, check=False):
    """per proof: the additions, then the fill, both on the current stream; the result is what interpolate / bn128.ifft read"""
    if not _is_dev(w_dev):
        raise Pil2glError("exec_dev takes a device tensor (exec_gl / exec_bn128 take host arrays)")
    adds_dev(prep, w_dev)
    return gather_dev(prep, w_dev, dst, dst_cols, montgomery, check)


# ---- connection polynomials ----
_FR_ONE = [((1 << 256) % 21888242871839275222246405745257275088548364400416034343698204186575808495617 >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(4)]


def conn_plan(n_rows, n_cols, n_w, N, field="gl"):
    """pil2gl_conn_plan (host-only): the sort's passes, the launch geometry, the working buffer"""
    info = (C.c_uint32 * 8)()
    nbytes = C.c_uint64()
    call("pil2gl_conn_plan", n_rows, n_cols, n_w, N, _WORDS[field], info, C.byref(nbytes))
    names = ("passes", "threads", "tile", "sortBlocks", "scanChunks", "loBits", "hiBits", "launches")
    return dict(zip(names, (int(x) for x in info)), scratchBytes=nbytes.value)


def _conn_consts(w, ks, n_cols, words):
    """(w, ks1) as the library reads them: ks1 = one, then the caller's n_cols - 1 elements of ks"""
    w = np.ascontiguousarray(w, np.uint64).reshape(-1)
    ks = np.ascontiguousarray(ks, np.uint64).reshape(-1)
    if w.size != words or ks.size != max(n_cols - 1, 0) * words:
        raise Pil2glError("w holds %d words and ks %d; one element and nCols - 1 = %d elements of %d words expected" % (w.size, ks.size, n_cols - 1, words))
    one = np.array([1] if words == 1 else _FR_ONE, np.uint64)
    return w, np.concatenate([one, ks])


def conn_pols(s_map, n_cols, N, w, ks, field="gl", n_w=None):
    """the setups' two S loops (compressor12_setup.js:470-500 and its five siblings): -> the (N, nCols[, 4]) columns, S[j][i] at [i, j].
    s_map: a uint32 array of shape (nCols, N), the setups' own sMap[j][i], or the exec file's table, nRows x nCols row-major (any integer
    type).  w = F.w[nBits] and ks = getKs(F, nCols - 1) as words: uint64 for Goldilocks, (., 4) Montgomery words for Fr, which is also
    what comes out.  n_w: one more than the highest signal (found when absent)."""
    words = _WORDS[field]
    s_map = np.asarray(s_map)
    if s_map.dtype == np.uint32 and s_map.shape == (n_cols, N):
        layout, n_rows, s_map = 1, N, np.ascontiguousarray(s_map)
    else:
        s_map = np.ascontiguousarray(s_map, np.uint64).reshape(-1)
        if n_cols == 0 or s_map.size % n_cols:
            raise Pil2glError("sMap holds %d entries, no multiple of nCols = %d" % (s_map.size, n_cols))
        layout, n_rows = 0, s_map.size // n_cols
    if n_w is None:
        n_w = int(s_map.max()) + 1 if s_map.size else 1
    w, ks1 = _conn_consts(w, ks, n_cols, words)
    dst = np.zeros((N, n_cols) + ((4,) if words == 4 else ()), np.uint64)
    call("pil2gl_conn_pols" if words == 1 else "pil2gl_bn128_conn_pols", _np_ptr(s_map), layout, n_rows, n_cols, n_w, N, _np_ptr(w), _np_ptr(ks1), _np_ptr(dst))
    return dst


def conn_pols_dev(prep, N, w, ks, dst=None, dst_stride=None, dst_offset=0, check=False, s_map=None):
    """the same from what prepare() returned: -> dst, a device matrix of N rows and dst_stride (default nCols) elements a row, of which
    columns [dst_offset, dst_offset + nCols) are written -- the layout interpolate / merkelize read.  The working buffer comes from the
    plan and lives for the call; enqueues on the current stream.  check=True blocks and returns (dst, firstBad), firstBad None when every
    index names a signal.  s_map: another device table of nRows x nCols 32-bit indices in place of prep's."""
    words = _WORDS[prep["field"]]
    n_cols = prep["nCols"]
    dst_stride = n_cols + dst_offset if dst_stride is None else dst_stride
    plan = conn_plan(prep["nRows"], n_cols, prep["nW"], N, prep["field"])
    w, ks1 = _conn_consts(w, ks, n_cols, words)
    if dst is None:
        dst = torch.empty((N, dst_stride) + ((4,) if words == 4 else ()), dtype=torch.int64, device=prep["sMap"].device)
    if dst.numel() < ((N - 1) * dst_stride + dst_offset + n_cols) * words:
        raise Pil2glError("dst holds %d words, %d rows of stride %d need more" % (dst.numel(), N, dst_stride))
    work = torch.empty(max(plan["scratchBytes"] // 8, 2), dtype=torch.int64, device=prep["sMap"].device)
    bad = C.c_uint64()
    call("pil2gl_conn_pols_dev" if words == 1 else "pil2gl_bn128_conn_pols_dev", _ptr(s_map if s_map is not None else prep["sMap"]), prep["nRows"], n_cols,
         prep["nW"], N, _np_ptr(w), _np_ptr(ks1), _ptr(dst), dst_stride, dst_offset, _ptr(work), plan["scratchBytes"], C.byref(bad) if check else None, _stream())
    if check:
        return dst, (None if bad.value == 0xFFFFFFFFFFFFFFFF else bad.value)
    return dst


# ---- connection check ----
_NONE = 0xFFFFFFFFFFFFFFFF


def conn_check_plan(N, n_cols, field="gl"):
    """pil2gl_conn_check_plan (host-only): the hash table's capacity, the launch geometry, the working buffer"""
    info = (C.c_uint32 * 8)()
    nbytes = C.c_uint64()
    call("pil2gl_conn_check_plan", N, n_cols, _WORDS[field], info, C.byref(nbytes))
    names = ("capBits", "threads", "loBits", "hiBits", "buildBlocks", "checkBlocks", "lanesPerCell", "launches")
    return dict(zip(names, (int(x) for x in info)), scratchBytes=nbytes.value)


def _report(rep):
    """the library's three words -> None when clean, else {"cell", "partner" (None when S names no cell), "kind"}"""
    if rep[2] == 0:
        return None
    return {"cell": int(rep[0]), "partner": None if rep[1] == _NONE else int(rep[1]), "kind": int(rep[2])}


def conn_check(a, S, n_cols, N, w, ks, field="gl"):
    """does the trace `a` meet {a} connect {S}: host arrays of N x nCols elements each (uint64 words; Fr Montgomery, 4 words an element),
    w and ks as conn_pols takes them -> None when clean, else the first failing cell (see _report; the kinds are pil2gl.h's)"""
    words = _WORDS[field]
    a = np.ascontiguousarray(a, np.uint64).reshape(-1)
    S = np.ascontiguousarray(S, np.uint64).reshape(-1)
    if a.size != N * n_cols * words or S.size != a.size:
        raise Pil2glError("a holds %d words and S %d; %d x %d elements of %d words expected" % (a.size, S.size, N, n_cols, words))
    w, ks1 = _conn_consts(w, ks, n_cols, words)
    rep = (C.c_uint64 * 3)()
    call("pil2gl_conn_check" if words == 1 else "pil2gl_bn128_conn_check", _np_ptr(a), _np_ptr(S), N, n_cols, _np_ptr(w), _np_ptr(ks1), rep)
    return _report(rep)


def conn_check_dev(a, S, n_cols, N, w, ks, field="gl", a_stride=None, a_offset=0, s_stride=None, s_offset=0):
    """the same on device matrices of N rows: a in columns [a_offset, a_offset + nCols) of rows a_stride elements wide (default nCols +
    a_offset), S alike -- where exec_dev wrote the trace and conn_pols_dev the constants; a and S may be one tensor.  The working buffer
    comes from the plan and lives for the call; blocks for the report."""
    words = _WORDS[field]
    a_stride = n_cols + a_offset if a_stride is None else a_stride
    s_stride = n_cols + s_offset if s_stride is None else s_stride
    for name, t, stride, offset in (("a", a, a_stride, a_offset), ("S", S, s_stride, s_offset)):
        if not _is_dev(t):
            raise Pil2glError("conn_check_dev takes device tensors (conn_check takes host arrays)")
        if n_cols and t.numel() < ((N - 1) * stride + offset + n_cols) * words:
            raise Pil2glError("%s holds %d words, %d rows of stride %d need more" % (name, t.numel(), N, stride))
    plan = conn_check_plan(N, n_cols, field)
    w, ks1 = _conn_consts(w, ks, n_cols, words)
    work = torch.empty(max(plan["scratchBytes"] // 8, 2), dtype=torch.int64, device=a.device)
    rep = (C.c_uint64 * 3)()
    call("pil2gl_conn_check_dev" if words == 1 else "pil2gl_bn128_conn_check_dev", _ptr(a), a_stride, a_offset, _ptr(S), s_stride, s_offset, N, n_cols,
         _np_ptr(w), _np_ptr(ks1), _ptr(work), plan["scratchBytes"], rep, _stream())
    return _report(rep)


def conn_check_probe():
    """pil2gl_debug_conn_check_probe: the longest distance between a key of the last call's hash table and its home slot"""
    from ._lib import load
    return int(load().pil2gl_debug_conn_check_probe())


# ---- files ----
def _short(path, found, expected):
    return Pil2glError("%s: %d bytes found, %d expected" % (path, found, expected))


def _sections(path, kind):
    """the minimal iden3 binfile reader: 4-byte type, u32 version, u32 section count, then (u32 id, u64 size, payload) until the file
    ends -> (version, {id: (offset, size)})"""
    size = os.path.getsize(path)
    with open(path, "rb") as f:
        head = f.read(12)
        if len(head) < 12:
            raise _short(path, size, 12)
        if head[:4] != kind.encode():
            raise Pil2glError("%s: type %r, %r expected" % (path, head[:4], kind))
        version, count = struct.unpack("<II", head[4:])
        out, at = {}, 12
        while at < size and len(out) < count:
            f.seek(at)
            h = f.read(12)
            if len(h) < 12:
                raise _short(path, size, at + 12)
            sid, n = struct.unpack("<IQ", h)
            if at + 12 + n > size:
                raise _short(path, size, at + 12 + n)
            out[sid] = (at + 12, n)
            at += 12 + n
    return version, out


def _section(path, secs, sid, expected=None):
    if sid not in secs:
        raise Pil2glError("%s: no section %d" % (path, sid))
    off, n = secs[sid]
    if expected is not None and n < expected:
        raise _short(path, os.path.getsize(path), os.path.getsize(path) + expected - n)
    return np.fromfile(path, np.uint8, n if expected is None else expected, offset=off)


def read_exec_file(path, n_cols, field="gl", n_witness=None):
    """readExecFile of compressor/exec_helpers.js:26-47 (field "gl": flat u64) or final/exec_helpers.js:14-39 (field "bn128": binfile
    "exec") -> {"field", "nAdds", "nSMap", "nCols", "sMap", and "adds" (gl: 4 nAdds words a, b, ca, cb) or "addsIdx" + "addsCoef" (bn128:
    2 nAdds indices, (2 nAdds, 4) Montgomery words)}.  A file shorter than its header says is refused with name, found and expected size."""
    size = os.path.getsize(path)
    if field == "gl":
        if size < 16:
            raise _short(path, size, 16)
        n_adds, n_smap = (int(x) for x in np.fromfile(path, np.uint64, 2))
        want = 8 * (2 + 4 * n_adds + n_smap * n_cols)
        if size < want:
            raise _short(path, size, want)
        body = np.fromfile(path, np.uint64, 4 * n_adds + n_smap * n_cols, offset=16)
        out = {"adds": body[:4 * n_adds], "sMap": body[4 * n_adds:]}
    elif field == "bn128":
        version, secs = _sections(path, "exec")
        if version != 1:
            raise Pil2glError("%s: exec version %d, 1 expected" % (path, version))
        n_adds, n_smap = (int(x) for x in _section(path, secs, 2, 16).view(np.uint64))
        out = {"addsIdx": _section(path, secs, 3, 16 * n_adds).view(np.uint64),
               "addsCoef": _section(path, secs, 4, 64 * n_adds).view(np.uint64).reshape(-1, 4),
               "sMap": _section(path, secs, 5, 8 * n_smap * n_cols).view(np.uint64)}
    else:
        raise Pil2glError("field is \"gl\" or \"bn128\"")
    out.update(field=field, nAdds=n_adds, nSMap=n_smap, nCols=n_cols)
    if n_witness is not None:
        out["nWitness"] = n_witness
    return out


def read_wtns(path):
    """a .wtns (binfile "wtns"): -> {"n8", "prime", "nWitness", "w": (nWitness, n8 / 8) uint64 words, normal form}"""
    _, secs = _sections(path, "wtns")
    head = _section(path, secs, 1, 4).tobytes()
    n8 = struct.unpack("<I", head[:4])[0]
    head = _section(path, secs, 1, 8 + n8).tobytes()
    n = struct.unpack("<I", head[4 + n8:8 + n8])[0]
    w = _section(path, secs, 2, n * n8).view(np.uint64).reshape(n, n8 // 8)
    return {"n8": n8, "prime": int.from_bytes(head[4:4 + n8], "little"), "nWitness": n, "w": w}
