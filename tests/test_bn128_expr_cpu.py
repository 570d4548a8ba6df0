"""BN254 Fr expression evaluator without a device: the Python checker against values worked out by hand, the encoder from the
reference's `code.code` on every operand kind, the planner through the library's host-only hook, everything the compute entries refuse
before any device call, and the host-side checks and launch geometry (csrc/bn_expr_plan.h) run once more in a stand-alone program built
with the address and undefined-behaviour sanitizers."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import bn128_expr_ref as ref
from bn128_expr_ref import R, ADD, SUB, MUL, COPY, TMP, SEC, SCALAR, tmp, sec, scalar, to_mont, from_mont
from conftest import ROOT

EINVAL, ENODEV = -1, -2
CSRC = os.path.join(ROOT, "pil2-stark-js_amd", "csrc")


# ---- the checker against hand-computed values -------------------------------------------------------------------------------------
# (these three pin the oracle, not the library: they need no new symbol of it, unlike every test below them)
def test_checker_arithmetic_is_montgomery_arithmetic():
    m = to_mont
    a = [[m(3), m(5)]]
    out = [[0, 0, 0, 0]]
    ops = [(ADD, sec(1, 0), sec(0, 0), sec(0, 1)), (SUB, sec(1, 1), sec(0, 0), sec(0, 1)), (MUL, sec(1, 2), sec(0, 0), sec(0, 1)),
           (COPY, sec(1, 3), scalar(0), None)]
    ref.evaluate(ops, [a, out], [m(R - 7)], 0)
    assert [from_mont(v) for v in out[0]] == [8, R - 2, 15, R - 7]
    assert ref.f_mul(m(1), m(1)) == m(1) == (1 << 256) % R and ref.f_mul(1, 1) == pow(1 << 256, -1, R)       # F.mul(x, y) = x y / 2^256


def test_checker_row_addressing_is_evalmaps():
    # domain n, N = 4: out[i] = a[(i + 1) % 4] - a[(i - 1 + 4) % 4]
    a = [[10], [20], [40], [80]]
    out = [[0] for _ in range(4)]
    ref.evaluate([(SUB, sec(1), sec(0, 0, 1), sec(0, 0, -1))], [a, out], [], 2)
    assert [r[0] for r in out] == [(20 - 80) % R, 30, 60, (10 - 40) % R]
    # domain ext, N = 8, extendBits = 1: prime +1 is two rows ahead, prime -1 is (8 - 1) << 1 = 14 = 6 mod 8 rows ahead
    b = [[k] for k in range(8)]
    out = [[0, 0] for _ in range(8)]
    ref.evaluate([(COPY, sec(1, 0), sec(0, 0, 1), None), (COPY, sec(1, 1), sec(0, 0, -1), None)], [b, out], [], 3, 1)
    assert [r[0] for r in out] == [2, 3, 4, 5, 6, 7, 0, 1] and [r[1] for r in out] == [6, 7, 0, 1, 2, 3, 4, 5]
    assert ref.row_index(5, 0, 3, 1) == 5 and ref.row_index(7, -1, 3, 0) == 6 and ref.row_index(0, -1, 3, 0) == 7
    # a destination with a row offset: out[(i + 1) % 4] = a[i]
    out = [[0] for _ in range(4)]
    ref.evaluate([(COPY, sec(1, 0, 1), sec(0), None)], [a, out], [], 2)
    assert [r[0] for r in out] == [80, 10, 20, 40]


def test_checker_rows_run_in_order_and_temporaries_carry_within_a_row():
    x = [[to_mont(2)], [to_mont(3)]]
    ref.evaluate([(MUL, tmp(0), sec(0), sec(0)), (MUL, sec(0), tmp(0), sec(0))], [x], [], 1)      # x = x^3 in place
    assert [from_mont(r[0]) for r in x] == [8, 27]


# ---- the encoder --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def bn():
    from pil2gl import bn128
    return bn128


def words(v):
    return ref.words_of([v])[0]


PIL_INFO = {
    "nConstants": 3,
    "mapSectionsN": {"cm1": 2, "cm2": 4},
    "cmPolsMap": [{"stage": 1, "stagePos": 0, "dim": 1}, {"stage": 1, "stagePos": 1, "dim": 1}, {"stage": 2, "stagePos": 3, "dim": 1}],
    "boundaries": [{"name": "everyRow"}, {"name": "everyFrame", "offsetMin": 1, "offsetMax": 2}, {"name": "everyFrame", "offsetMin": 0, "offsetMax": 1}],
}


def test_encoder_maps_every_reference_operand_kind(bn):
    ctx = {"pilInfo": PIL_INFO, "publics": [words(11), words(12)], "challenges": [[words(21)], [words(22), words(23)]],
           "subproofValues": [words(31), words(32)]}
    T = lambda i: {"type": "tmp", "id": i, "dim": 1}
    code = [
        {"op": "mul", "dest": T(0), "src": [{"type": "const", "id": 2, "prime": -1}, {"type": "cm", "id": 2, "prime": 1}]},
        {"op": "add", "dest": T(1), "src": [T(0), {"type": "number", "value": "-5"}]},
        {"op": "sub", "dest": T(2), "src": [{"type": "public", "id": 1}, {"type": "challenge", "stage": 2, "stageId": 1}]},
        {"op": "mul", "dest": T(3), "src": [{"type": "x"}, {"type": "Zi", "boundaryId": 2}]},
        {"op": "add", "dest": T(4), "src": [{"type": "subproofValue", "id": 1}, {"type": "number", "value": "-5"}]},
        {"op": "copy", "dest": {"type": "cm", "id": 1, "prime": 0}, "src": [T(4)]},
        {"op": "mul", "dest": {"type": "q", "dim": 1}, "src": [T(3), {"type": "Zi", "boundaryId": 0}]},
    ]
    ops, n_tmp, sections, scalars = bn.encode_program(code, ctx, "ext")
    assert n_tmp == 5
    assert sections == [("const_ext", 3, None), ("cm2_ext", 4, None), ("x_ext", 1, None), ("Zi_ext", 1, 2), ("cm1_ext", 2, None),
                        ("Zi_ext", 1, 0), ("q_ext", 1, None)]                      # sources before the destination, as compileCode resolves them
    assert ref.ints_of(scalars) == [to_mont(R - 5), 12, 23, 32]                  # F.e(-5) = r - 5, once; the others as ctx holds them
    assert ops == [
        (MUL, tmp(0), (SEC, 1, 0, -1, 2), (SEC, 1, 1, 1, 3)),
        (ADD, tmp(1), tmp(0), scalar(0)),
        (SUB, tmp(2), scalar(1), scalar(2)),
        (MUL, tmp(3), sec(2), sec(3)),
        (ADD, tmp(4), scalar(3), scalar(0)),
        (COPY, (SEC, 1, 4, 0, 1), tmp(4), None),
        (MUL, sec(6), tmp(3), sec(5)),
    ]
    g_ops, _, _, g_sc = bn.encode_program([{"op": "copy", "dest": T(0), "src": [{"type": "subproofValue", "subproofId": 1, "id": 0}]}],
                                          dict(ctx, subproofValues=[[words(1)], [words(2)]]), "n", is_global=True)
    assert ref.ints_of(g_sc) == [2]


def test_encoder_refuses_what_the_reference_throws_on(bn):
    ctx = {"pilInfo": PIL_INFO, "publics": [], "challenges": [], "subproofValues": []}
    T = {"type": "tmp", "id": 0, "dim": 1}
    for code, msg in (([{"op": "mul", "dest": {"type": "q", "dim": 1}, "src": [T, T]}], "Accessing q in domain n"),
                      ([{"op": "copy", "dest": {"type": "const", "id": 0}, "src": [T]}], "Invalid reference type set"),
                      ([{"op": "copy", "dest": T, "src": [{"type": "eval", "id": 0}]}], "Invalid reference type get"),
                      ([{"op": "muladd", "dest": T, "src": [T, T, T]}], "Invalid op"),
                      ([{"op": "copy", "dest": T, "src": [{"type": "tmp", "id": 1, "dim": 3}]}], "dim")):
        with pytest.raises(bn.Pil2glError, match=msg):
            bn.encode_program(code, ctx, "n")


# ---- the planner hook ---------------------------------------------------------------------------------------------------------------
NO_SCALARS = np.zeros((0, 4), np.uint64)


def test_plan_live_temporaries_at_the_lds_limit_and_one_above(bn):
    limit = bn.plan_program(ref.live_program(1), [1, 1], NO_SCALARS, 6)["ldsSlotLimit"]
    assert limit == 30                                                              # 60 KiB / (32 B x one wave)
    at = bn.plan_program(ref.live_program(limit), [limit, 1], NO_SCALARS, 6)
    above = bn.plan_program(ref.live_program(limit + 1), [limit + 1, 1], NO_SCALARS, 6)
    assert (at["slots"], at["form"], at["threads"]) == (limit, 0, 64)
    assert (above["slots"], above["form"], above["threads"]) == (limit + 1, 1, 256)
    assert at["lanesPerLaunch"] == 512 * 64 and above["lanesPerLaunch"] == 512 * 256


@pytest.mark.parametrize("k,threads", ((1, 256), (7, 256), (8, 128), (15, 128), (16, 64), (30, 64)))
def test_plan_workgroup_shrinks_as_slots_grow(bn, k, threads):
    p = bn.plan_program(ref.live_program(k), [k, 1], NO_SCALARS, 10)
    assert (p["slots"], p["form"], p["threads"]) == (k, 0, threads) and k * 32 * threads <= 60 * 1024


def test_plan_collapses_common_subexpressions_and_repeated_reads(bn):
    a, b = sec(0, 0, 1), sec(0, 1)
    ops = [(MUL, tmp(0), a, b), (MUL, tmp(1), b, a), (ADD, tmp(2), tmp(0), tmp(1)), (MUL, tmp(3), a, b), (ADD, tmp(4), tmp(2), tmp(3)),
           (COPY, tmp(5), tmp(4), None), (COPY, sec(1), tmp(5), None)]
    p = bn.plan_program(ops, [2, 1], NO_SCALARS, 4)
    # two loads, one product, t0 + t0, (t0 + t0) + t0, one store
    assert p["ops"] == 6 and p["slots"] == 2 and p["form"] == 0


def test_plan_of_an_empty_program(bn):
    assert bn.plan_program([], [1], NO_SCALARS, 3, nTmp=0)["ops"] == 0


# ---- refused before any device call ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    import pil2gl
    return pil2gl.load()


def _call(lib, entry, ops, n_tmp, widths, n_scalars, n_bits, prime_shift=0, null_section=None, null_scalars=False, n_sections=None):
    from pil2gl import _lib
    from pil2gl.stark import make_c_program
    prog = make_c_program(ops, n_tmp)
    backing = [np.zeros(((1 << min(n_bits, 6)) * w + 1) * 4, np.uint64) for w in widths]      # never reached: every case is refused first
    cs = (_lib.GlxSection * max(len(widths), 1))()
    for i, w in enumerate(widths):
        cs[i].ptr = None if i == null_section else backing[i].ctypes.data
        cs[i].width = w
    sc = np.zeros((max(n_scalars, 1), 4), np.uint64)
    ctx = _lib.BnxCtx(n_bits, prime_shift, len(widths) if n_sections is None else n_sections, n_scalars, cs if widths else None,
                      None if null_scalars else sc.ctypes.data_as(_lib.u64p))
    if entry == "plan":
        return lib.pil2gl_debug_bn128_plan_program(C.byref(prog), C.byref(ctx), (C.c_uint32 * 6)())
    if entry == "dev":
        return lib.pil2gl_bn128_eval_program_dev(C.byref(prog), C.byref(ctx), None)
    return lib.pil2gl_bn128_eval_program(C.byref(prog), C.byref(ctx))


GOOD = [(MUL, tmp(0), sec(0, 0, 1), scalar(0)), (ADD, sec(1), tmp(0), sec(0, 1))]
REFUSALS = {
    "dim 3 source": dict(ops=[(MUL, tmp(0), (SEC, 3, 0, 0, 0), scalar(0))], msg=b"dim"),
    "dim 3 destination": dict(ops=[(COPY, (TMP, 3, 0, 0, 0), sec(0), None)], msg=b"dim"),
    "dim 0": dict(ops=[(COPY, tmp(0), (SEC, 0, 0, 0, 0), None)], msg=b"dim"),
    "op above copy": dict(ops=[(4, tmp(0), sec(0), sec(0))], msg=b"Invalid op"),
    "section out of range": dict(ops=[(COPY, tmp(0), sec(2), None)], msg=b"section 2 out of range"),
    "column out of range": dict(ops=[(COPY, tmp(0), sec(0, 2), None)], msg=b"column 2 out of range"),
    "destination column out of range": dict(ops=[(COPY, sec(1, 1), sec(0), None)], msg=b"column 1 out of range"),
    "scalar out of range": dict(ops=[(COPY, tmp(0), scalar(1), None)], msg=b"scalar 1 out of range"),
    "tmp out of range": dict(ops=[(COPY, tmp(1), sec(0), None)], msg=b"tmp 1 out of range"),
    "tmp read before written": dict(ops=[(COPY, sec(1), tmp(0), None)], msg=b"read before written"),
    "scalar as destination": dict(ops=[(COPY, scalar(0), sec(0), None)], msg=b"Invalid reference type set"),
    "unknown operand class": dict(ops=[(COPY, tmp(0), (3, 1, 0, 0, 0), None)], msg=b"Invalid reference type get"),
    "too many sections": dict(ops=GOOD, widths=[2, 1] + [1] * 23, msg=b"too many sections"),
    "nBits above 28": dict(ops=GOOD, n_bits=29, msg=b"nBits"),
    "row offset overflow": dict(ops=[(COPY, tmp(0), sec(0, 0, 1 << 20), None)], n_bits=28, prime_shift=12, msg=b"row offset overflow"),
    "negative row offset overflow": dict(ops=[(COPY, tmp(0), sec(0, 0, -(1 << 20) - 1), None)], n_bits=28, prime_shift=11, msg=b"row offset overflow"),
    "null section that is read": dict(ops=GOOD, null_section=0, msg=b"null pointer"),
    "null section that is written": dict(ops=GOOD, null_section=1, msg=b"null pointer"),
    "null scalar pool": dict(ops=GOOD, null_scalars=True, msg=b"null scalar pool"),
    "null section table": dict(ops=GOOD, widths=[], n_sections=2, msg=b"null section table"),
    "reads a written column at an offset": dict(ops=[(MUL, sec(0, 1), sec(0, 1, 1), scalar(0))], msg=b"non-zero row offset"),
    "reads a written column at an offset, later": dict(ops=[(COPY, sec(0, 0), scalar(0), None), (COPY, sec(1), sec(0, 0, -1), None)], msg=b"non-zero row offset"),
    "writes at an offset a column it reads": dict(ops=[(COPY, sec(0, 0, 1), sec(0, 0), None)], msg=b"non-zero row offset"),
    "writes one column at two offsets": dict(ops=[(COPY, sec(1, 0, 1), sec(0), None), (COPY, sec(1, 0, 0), sec(0), None)], msg=b"more than one row offset"),
}


@pytest.mark.parametrize("entry", ("plan", "dev", "host"))
@pytest.mark.parametrize("case", sorted(REFUSALS))
def test_refused_before_any_device_call(lib, entry, case):
    kw = dict(REFUSALS[case])
    msg = kw.pop("msg")
    widths = kw.pop("widths", [2, 1])
    rc = _call(lib, entry, kw.pop("ops"), 1, widths, 1, kw.pop("n_bits", 3), **kw)
    assert rc == EINVAL and msg in lib.pil2gl_last_error(), lib.pil2gl_last_error()


def test_null_program_context_and_op_list_are_refused(lib):
    from pil2gl import _lib
    ctx = _lib.BnxCtx(3, 0, 0, 0, None, None)
    prog = _lib.GlxProgram(2, 1, None)
    info = (C.c_uint32 * 6)()
    for fn, extra in ((lib.pil2gl_bn128_eval_program, ()), (lib.pil2gl_bn128_eval_program_dev, (None,)), (lib.pil2gl_debug_bn128_plan_program, (info,))):
        assert fn(None, C.byref(ctx), *extra) == EINVAL
        assert fn(C.byref(prog), None, *extra) == EINVAL
        assert fn(C.byref(prog), C.byref(ctx), *extra) == EINVAL and b"null op-list" in lib.pil2gl_last_error()
    assert lib.pil2gl_debug_bn128_plan_program(C.byref(_lib.GlxProgram(0, 0, None)), C.byref(ctx), None) == EINVAL


def test_what_is_allowed_passes_the_checks(lib):
    """the same cell read and written at offset 0 (x = x * x), offsets on columns that are only read, a destination with an offset that
    nobody reads: all planned; the largest domain and the largest offsets that fit are too"""
    assert _call(lib, "plan", [(MUL, sec(0, 1), sec(0, 1), sec(0, 1))], 1, [2, 1], 1, 3) == 0
    assert _call(lib, "plan", [(MUL, sec(0, 1), sec(0, 0, -1), sec(0, 0, 2)), (ADD, sec(1, 0, 1), sec(0, 1), scalar(0))], 1, [2, 1], 1, 3) == 0
    assert _call(lib, "plan", [(COPY, tmp(0), sec(0, 0, (1 << 19) - 1), None)], 1, [2, 1], 1, 28, prime_shift=12) == 0
    assert _call(lib, "plan", [(COPY, tmp(0), sec(0, 0, -(1 << 19)), None)], 1, [2, 1], 1, 28, prime_shift=12) == 0
    assert _call(lib, "plan", GOOD, 1, [2, 1] + [1] * 22, 1, 3) == 0                # 24 sections: the table's size


def _have_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


def test_compute_entries_need_a_device(lib):
    """a program that passes the checks reaches the device layer: without a device both forms say so; with one the host form computes
    (the device form takes device pointers: tests/test_gpu_bn128_expr.py)"""
    if not _have_gpu():
        assert _call(lib, "dev", GOOD, 1, [2, 1], 1, 3) == ENODEV and _call(lib, "host", GOOD, 1, [2, 1], 1, 3) == ENODEV
        return
    from pil2gl import bn128
    import random
    rng = random.Random(5)
    a, out, sc = ref.random_section(rng, 8, 2), [[0] for _ in range(8)], [rng.randrange(R)]
    wa, wo = ref.section_words(a), ref.section_words(out)
    bn128.eval_program(GOOD, [wa, wo], ref.words_of(sc), 3)
    ref.evaluate(GOOD, [a, out], sc, 3)
    assert (wo == ref.section_words(out)).all() and (wa == ref.section_words(a)).all()


def test_first_nonzero_row_argument_errors(lib):
    row, val, col = C.c_uint64(5), np.ones(4, np.uint64), np.zeros(64, np.uint64)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    f = lib.pil2gl_bn128_first_nonzero_row_dev
    assert f(p(col), 2, 0, 0, 4, None, p(val), None) == EINVAL and f(p(col), 2, 0, 0, 4, C.byref(row), None, None) == EINVAL
    assert f(p(col), 2, 2, 0, 4, C.byref(row), p(val), None) == EINVAL and b"column" in lib.pil2gl_last_error()
    assert f(p(col), 0, 0, 0, 4, C.byref(row), p(val), None) == EINVAL
    assert f(p(col), 2, 0, 5, 4, C.byref(row), p(val), None) == EINVAL and b"empty range" in lib.pil2gl_last_error()
    assert f(p(col), 2, 0, 0, (1 << 28) + 1, C.byref(row), p(val), None) == EINVAL
    assert f(None, 2, 0, 0, 4, C.byref(row), p(val), None) == EINVAL
    assert row.value == 5 and (val == 1).all()                                       # nothing was written
    assert f(None, 2, 0, 3, 3, C.byref(row), p(val), None) == 0 and row.value == 2 ** 64 - 1 and not val.any()      # an empty range needs no device


# ---- the host code under the sanitizers, in a program of its own -----------------------------------------------------------------
def test_host_checks_and_geometry_under_the_sanitizers(tmp_path, bn):
    exe = str(tmp_path / "bn_expr_dump")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                           os.path.join(ROOT, "tests", "bn_expr_dump.cpp"), "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", "sanitizer report or failure:\n" + run.stderr
    got = json.loads(run.stdout)
    # the geometry of every slot count 0..40 at three domain sizes, against the library's hook where a program reaches that slot count
    for n_bits in (0, 8, 20):
        for k in (1, 7, 8, 15, 16, 30, 31, 40):
            p = bn.plan_program(ref.live_program(k), [k, 1], NO_SCALARS, n_bits)
            form, threads, blocks, lds, lanes, tmp_bytes = got["geometry"]["%d/%d" % (k, n_bits)]
            assert (form, threads, lanes) == (p["form"], p["threads"], p["lanesPerLaunch"]), (k, n_bits)
            assert blocks == min(max((1 << n_bits) // threads, 1), 512)
            assert lds == (k * 32 * threads if form == 0 else 0) and lds <= 60 * 1024
            assert tmp_bytes == (k * 32 * threads * blocks if form == 1 else 0)
    assert got["geometry"]["0/8"] == got["geometry"]["1/8"]
    assert got["verdicts"] == {"good": "", "in place": "", "dim": "dim 3 in op 0: Fr elements have dim 1",
                               "race": "section 0 column 1 is written and also read at a non-zero row offset",
                               "two offsets": "section 1 column 0 is written at more than one row offset",
                               "overflow": "row offset overflow in op 0", "null": "section 0 is read or written in op 0 and has a null pointer"}
