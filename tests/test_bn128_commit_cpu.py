"""BN254 G1 stage commit (pil2gl_bn128_g1_commit) without a device: the exported symbols, every refusal of the two compute entries, the
batch planner through its host-only entry against the checker's statement of it (tests/bn128_g1_packed_ref.py), the lane mapping through
the library, and the same host code run once more in a stand-alone program built with the address and undefined-behaviour sanitizers."""
import ctypes as C
import itertools
import json
import os
import subprocess

import numpy as np
import pytest

import bn128_g1_ref as ref
import bn128_g1_packed_ref as pref
from bn128_g1_ref import G
from conftest import ROOT

EINVAL, ENODEV = -1, -2
CSRC = os.path.join(ROOT, "pil2-stark-js_amd", "csrc")
ENTRIES = ("pil2gl_bn128_g1_commit", "pil2gl_bn128_g1_commit_dev")
MAX_N = 1 << 28


@pytest.fixture(scope="module")
def lib():
    import pil2gl
    return pil2gl.load()


def _have_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


def describe(polys):
    from pil2gl._lib import G1Poly
    descs = (G1Poly * max(len(polys), 1))()
    flat = []
    for k, (first, rows, slots) in enumerate(polys):
        descs[k].first, descs[k].rows, descs[k].m = first, rows, len(slots)
        flat += [pref.EMPTY if s is None else s for s in slots]
    return descs, (C.c_uint32 * max(len(flat), 1))(*flat)


def commit(lib, name, bases, n_bases, scalars, row_stride, polys, out, descs=True, slots=True, K=None):
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    d, s = describe(polys)
    args = [p(bases), n_bases, p(scalars), row_stride, 1, d if descs else None, len(polys) if K is None else K, s if slots else None, p(out)]
    if name.endswith("_dev"):
        args.append(None)
    return getattr(lib, name)(*args)


def test_every_new_symbol_is_exported(lib):
    for name in ENTRIES + ("pil2gl_debug_bn128_msm_batch_plan", "pil2gl_debug_bn128_commit_locate"):
        assert hasattr(lib, name)
    from pil2gl import bn128
    assert callable(bn128.g1_commit)


# ---- refusals: before any device call, the limit named, nothing written ------------------------------------------------------------
@pytest.mark.parametrize("name", ENTRIES)
def test_every_refusal_names_its_limit_and_writes_nothing(lib, name):
    b, s = np.zeros(8 * 64, np.uint64), np.zeros(4 * 64, np.uint64)
    o = np.ones(8 * 16, np.uint64)
    one = (0, 2, [0])

    def refused(word, polys, n_bases=64, row_stride=4, bases=b, scalars=s, out=o, **kw):
        assert commit(lib, name, bases, n_bases, scalars, row_stride, polys, out, **kw) == EINVAL, word
        assert word.encode() in lib.pil2gl_last_error(), (word, lib.pil2gl_last_error())

    refused("K = 0", [], K=0)
    refused("K = 17", [one] * 17)
    refused("m = 0", [one, (0, 2, [])])
    refused("m = 65", [(0, 0, [0] * 65)])
    refused("256 slots", [(0, 0, [0] * 64)] * 4 + [(0, 0, [0])])
    refused("nBases", [(0, 33, [0, 1])])                              # 66 coefficients on 64 bases
    refused("nBases", [one, (0, 1, [None] * 3)], n_bases=2)           # empty slots count as coefficients
    refused("2^28", [(0, MAX_N // 2, [0]), (0, MAX_N // 2, [0]), (0, 1, [0])], n_bases=MAX_N)
    refused("2^28", [(0, MAX_N + 1, [0])], n_bases=1 << 40)
    refused("2^28", [(0, 1 << 40, [0] * 64)], n_bases=1 << 62)
    refused("rowStride", [one], row_stride=0)
    refused("rowStride", [one], row_stride=1 << 32)
    refused("column 4", [(0, 2, [0, 4])])                             # neither the marker nor below rowStride = 4
    refused("column 4294967294", [(0, 2, [0xFFFFFFFE])])
    refused("first", [(1 << 58, 2, [0])])
    refused("null", [one], out=None)
    refused("null", [one], bases=None)
    refused("null", [one], scalars=None)
    refused("null", [one], descs=False)
    refused("null", [one], slots=False)
    assert (o == 1).all()                                             # nothing was written


def test_dev_form_refuses_misaligned_pointers(lib):
    b, s, o = np.zeros(8 * 4 + 2, np.uint64), np.zeros(4 * 4 + 2, np.uint64), np.ones(8, np.uint64)
    b, s = b[(b.ctypes.data // 8) % 2:], s[(s.ctypes.data // 8) % 2:]               # 16-byte aligned; one word further is not
    assert commit(lib, ENTRIES[1], b[1:], 4, s, 1, [(0, 2, [0])], o) == EINVAL and b"aligned" in lib.pil2gl_last_error()
    assert commit(lib, ENTRIES[1], b, 4, s[1:], 1, [(0, 2, [0])], o) == EINVAL and b"aligned" in lib.pil2gl_last_error()
    assert (o == 1).all()


def test_host_form_of_a_batch_without_points_needs_no_device(lib):
    o = np.ones(8 * 3, np.uint64)
    assert commit(lib, ENTRIES[0], None, 0, None, 1, [(0, 0, [0]), (5, 0, [None, 0]), (0, 0, [None])], o) == 0 and not o.any()


def test_compute_entries_need_a_device(lib):
    """valid arguments reach the device layer: without a device both forms say so; with one the host form computes"""
    b, s = ref.point_words([G, G]).reshape(-1), ref.scalar_words([1, 2]).reshape(-1)
    o = np.zeros(16, np.uint64)
    polys = [(0, 1, [0, 1]), (0, 2, [None])]                          # all-empty polynomials still need the device once another has a point
    if _have_gpu():
        assert commit(lib, ENTRIES[0], b, 2, s, 2, polys, o) == 0 and ref.point_of(o[:8]) == ref.mul(3, G) and not o[8:].any()
        return
    for name in ENTRIES:
        assert commit(lib, name, b, 2, s, 2, polys, o) == ENODEV
    assert not o.any()


# ---- the batch planner ---------------------------------------------------------------------------------------------------------------
def lib_batch_plan(lib, counts):
    out, nbytes = (C.c_uint32 * 4)(), C.c_uint64(1)
    rc = lib.pil2gl_debug_bn128_msm_batch_plan(len(counts), (C.c_uint64 * max(len(counts), 1))(*counts), out, C.byref(nbytes))
    return rc, tuple(out), nbytes.value


def lib_plan(lib, n):
    out, nbytes = (C.c_uint32 * 4)(), C.c_uint64(1)
    assert lib.pil2gl_debug_bn128_msm_plan(n, out, C.byref(nbytes)) == 0
    return tuple(out), nbytes.value


def batches():
    """equal and very unequal counts from 0 to 2^28 in total, for K in {1, 2, 5, 16}"""
    for K in (1, 2, 5, 16):
        for total in [0, 1, K, 1000] + [1 << e for e in range(4, 29)] + [(1 << e) + 1 for e in range(4, 28, 3)]:
            yield [total // K] * K                                    # equal
            yield [total - (K - 1) * min(1, total // K)] + [min(1, total // K)] * (K - 1)      # one large, the others 1 (or 0)
            yield [0] * (K - 1) + [total]                             # all in the last
            if K > 1:
                yield [total // 2, 0] + [(total - total // 2) // (K - 2)] * (K - 2) if K > 2 else [total // 2, total - total // 2]


def test_batch_plan_equals_the_checkers_and_keeps_its_bounds(lib):
    seen_lowered = seen_cells = False
    for counts in batches():
        K, total = len(counts), sum(counts)
        assert total <= MAX_N
        rc, (c, n_w, nbw, g), nbytes = lib_batch_plan(lib, counts)
        assert rc == 0, counts
        assert (c, n_w, nbw, g) == pref.batch_plan(counts), counts
        assert 4 <= c <= 16 and n_w * c >= 255 > (n_w - 1) * c and nbw == 1 << (c - 1) and 1 <= g <= n_w
        assert K * n_w * nbw <= pref.BUCKET_BUDGET, counts                              # the bucket budget
        assert K * g * nbw <= pref.PASS_CELLS, counts                                   # what the one-workgroup scan is given
        if total == 0:
            assert nbytes == 0
            continue
        assert 0 < nbytes <= pref.batch_scratch_bound(K, total), counts
        assert nbytes >= 4 * total * g + 128 * K * n_w * nbw                            # a pass's lists and every bucket fit
        seen_lowered |= c < ref.plan(max(counts))[0]
        seen_cells |= 2 * g <= min(n_w, min(max(8 * total, 1 << 19), 1 << 30) // total) and 2 * g <= 64
        if K == 1:
            assert ((c, n_w, nbw, g), nbytes) == lib_plan(lib, counts[0])
            assert nbytes <= ref.scratch_bound(counts[0])                               # no larger than the single MSM's bound
    assert seen_lowered and seen_cells                                # both limits were met in the grid


def test_batch_plan_refuses_bad_arguments(lib):
    assert lib_batch_plan(lib, [])[0] == EINVAL and lib_batch_plan(lib, [1] * 17)[0] == EINVAL
    assert lib_batch_plan(lib, [MAX_N, 1])[0] == EINVAL and b"2^28" in lib.pil2gl_last_error()
    assert lib_batch_plan(lib, [(1 << 64) - 1, 2])[0] == EINVAL
    assert lib.pil2gl_debug_bn128_msm_batch_plan(1, None, None, None) == EINVAL


# ---- the lane mapping ----------------------------------------------------------------------------------------------------------------
MAPPED = [
    (1, [(0, 5, [0])]),                                               # a contiguous vector
    (3, [(0, 4, [2])]),                                               # one strided column
    (4, [(0, 3, [0, 1, 2, 3]), (0, 3, [3, None, 1])]),
    (7, [(14, 2, [6, None, None, 0, 3]), (0, 0, [1]), (7, 1, [None]), (0, 65, [5])]),
    (1, [(0, 4, [0]), (4, 4, [0]), (8, 3, [0])]),                     # pieces of one vector
    (1 << 20, [(1 << 40, 3, [(1 << 20) - 1, 0])]),                    # offsets past 2^32
    (64, [(0, 1, list(range(64)))] * 4),                              # 256 slots
    (2, [(k, 1 + k, [k % 2]) for k in range(16)]),                    # K = 16
]


def test_library_maps_every_lane_to_one_coefficient_and_back(lib):
    for row_stride, polys in MAPPED:
        descs, slots = describe(polys)
        want = [(k, i, e) for k, poly in enumerate(polys) for i, e in enumerate(pref.elements(poly, row_stride))]
        out = (C.c_uint64 * 4)()
        for lane, (k, i, e) in enumerate(want):
            assert lib.pil2gl_debug_bn128_commit_locate(descs, len(polys), slots, row_stride, lane, out) == 0
            assert tuple(out) == (k, i, 0 if e is None else 1, e or 0), (polys, lane)
            assert pref.locate(polys, lane) == (k, i)
        assert lib.pil2gl_debug_bn128_commit_locate(descs, len(polys), slots, row_stride, len(want), out) == EINVAL
        assert len(set((k, i) for k, i, _ in want)) == len(want)


# ---- the host code under the sanitizers, in a program of its own --------------------------------------------------------------------
def test_host_code_under_the_sanitizers_matches_python(tmp_path):
    exe = str(tmp_path / "bn_msm_batch_dump")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                           os.path.join(ROOT, "tests", "bn_msm_batch_dump.cpp"), os.path.join(CSRC, "bn_params.cpp"), "-o", exe])
    plans = [counts for counts in itertools.islice(batches(), 0, None, 3)]
    lines = ["plan %d %s" % (len(c), " ".join(map(str, c))) for c in plans]
    for row_stride, polys in MAPPED:
        lines.append("map %d %d" % (row_stride, len(polys)))
        lines += ["%d %d %d %s" % (first, rows, len(slots), " ".join(str(-1 if s is None else s) for s in slots)) for first, rows, slots in polys]
    (tmp_path / "batches.txt").write_text("\n".join(lines) + "\n")
    run = subprocess.run([exe, str(tmp_path / "batches.txt")], capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", "sanitizer report or failure:\n" + run.stderr
    got = json.loads(run.stdout)
    assert len(got["plans"]) == len(plans) and len(got["maps"]) == len(MAPPED)
    for counts, (c, n_w, nbw, g, nbytes) in zip(plans, got["plans"]):
        assert (c, n_w, nbw, g) == pref.batch_plan(counts) and nbytes <= pref.batch_scratch_bound(len(counts), sum(counts)), counts
    for (row_stride, polys), lanes in zip(MAPPED, got["maps"]):
        want = [[k, i, -1 if e is None else e] for k, poly in enumerate(polys) for i, e in enumerate(pref.elements(poly, row_stride))]
        assert lanes == want, polys
        assert len(lanes) == sum(rows * len(slots) for _, rows, slots in polys)          # every lane of sum n_k, each exactly once
