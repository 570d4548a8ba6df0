"""CPU-side checks of pil2gl_bn128_roots_from_group_proofs: declared in include/pil2gl.h with the argument list the binding uses,
exported by the library, bound by the ctypes table, exported by the Node addon next to the two BN128 opening calls -- and, like every
compute entry, PIL2GL_ENODEV without a device."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

pil2gl = pytest.importorskip("pil2gl")
from pil2gl import _lib  # noqa: E402

NAME = "pil2gl_bn128_roots_from_group_proofs"
NODE = shutil.which("node")


def _prototype(name):
    src = open(os.path.join(ROOT, "include", "pil2gl.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\b(\w[\w ]*?)\s*\b" + name + r"\s*\(([^)]*)\)\s*;", src)
    assert m, name + " is not declared in include/pil2gl.h"
    return m.group(1).strip(), [a.strip() for a in m.group(2).split(",")]


def test_declared_exported_and_bound_with_matching_arguments():
    ret, args = _prototype(NAME)
    assert ret == "int"
    assert [a.split()[-1].lstrip("*") for a in args] == ["hostVals", "hostSiblings", "width", "levels", "arity", "custom", "siblingsMontgomery",
                                                         "hostIdxs", "nIdx", "hostRoots"]
    res, argtypes = _lib.SIGNATURES[NAME]
    assert res is C.c_int and len(argtypes) == len(args)
    for decl, ty in zip(args, argtypes):                  # pointer <-> c_void_p, uint64_t <-> c_uint64, uint32_t <-> c_uint32, int <-> c_int
        want = C.c_void_p if "*" in decl else {"uint64_t": C.c_uint64, "uint32_t": C.c_uint32, "int": C.c_int}[decl.split()[0]]
        assert ty is want, decl
    lib = _lib.load()
    assert hasattr(lib, NAME)
    # the launch counter the GPU tests read: host-only, declared, bound, zero before anything ran
    assert _prototype("pil2gl_debug_bn128_path_launches") == ("uint64_t", ["void"])
    assert _lib.SIGNATURES["pil2gl_debug_bn128_path_launches"] == (C.c_uint64, [])
    assert isinstance(lib.pil2gl_debug_bn128_path_launches(), int)


def test_header_lists_the_entry_among_the_calls_that_block():
    src = open(os.path.join(ROOT, "include", "pil2gl.h")).read()
    head = src[:src.index("#pragma once")]
    assert "bn128_roots_from_group_proofs" in head
    assert "bn128_group_proof / bn128_group_proofs" in head and "BLOCKING streams" in head


@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_addon_exports_the_bn128_opening_calls():
    js = ("const a=require(%r).native;"
          "for (const k of ['bn128GroupProofDev','bn128GroupProofsDev','bn128RootsFromGroupProofs']) if (typeof a[k] !== 'function') throw new Error('missing '+k);"
          "console.log('ok')") % os.path.join(ROOT, "pil2-stark-js_amd", "js", "index.js")
    out = subprocess.run([NODE, "-e", js], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "ok" in out.stdout, out.stderr


def _have_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


@pytest.mark.skipif(_have_gpu(), reason="only meaningful on a machine without a GPU")
def test_enodev_without_a_device():
    lib = _lib.load()
    vals = np.zeros(3, np.uint64); sib = np.zeros(2 * 4 * 4, np.uint64); ii = np.zeros(1, np.uint64); out = np.zeros(4, np.uint64)
    p = lambda a: C.c_void_p(a.ctypes.data)
    before = lib.pil2gl_debug_bn128_path_launches()
    assert lib.pil2gl_bn128_roots_from_group_proofs(p(vals), p(sib), 3, 2, 4, 0, 0, p(ii), 1, p(out)) == -2
    assert lib.pil2gl_bn128_roots_from_group_proofs(None, None, 0, 0, 4, 0, 0, None, 0, None) == -2       # even an empty batch asks for the device first
    assert lib.pil2gl_debug_bn128_path_launches() == before
    from pil2gl import bn128
    with pytest.raises(pil2gl.Pil2glError):
        bn128.buildMerkleHash(4, False).calculateRootsFromGroupProofs([([1, 2, 3], [[0, 0, 0, 0]] * 2)], [0])
