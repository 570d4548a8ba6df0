"""How a transform's launches walk their column chunks, for tests: pil2gl_debug_plan_transform_grid / _walk / _walk_cover (csrc/ntt.hip)
answer from the planner and from walk_at, the one mapping (workgroup, step) -> (hi, gt, cc) the tile kernels run.  Host only: no device."""
import collections
import ctypes as C

import numpy as np

from transform_plan import OPS

WORDS = 5                                                   # PIL2GL_PLAN_GRID_WORDS
Grid = collections.namedtuple("Grid", "grid walk tiles group_tiles chunks")
NONE = 0xFFFFFFFF


def _call(op, n_bits, n_pols, ext_bits, coset_count):
    return OPS.index(op), n_bits, n_pols, n_bits + ext_bits, coset_count


def grids(op, n_bits, n_pols, ext_bits=0, coset_count=0):
    """(grid, W, row tiles, tiles per outer index, column chunks) of each launch of one call, in launch order"""
    from pil2gl import _lib
    lib = _lib.load()
    buf = (C.c_uint32 * (WORDS * 64))()
    n = C.c_uint32()
    rc = lib.pil2gl_debug_plan_transform_grid(*_call(op, n_bits, n_pols, ext_bits, coset_count), buf, 64, C.byref(n))
    assert rc == 0, lib.pil2gl_last_error()
    return [Grid(*buf[WORDS * i:WORDS * (i + 1)]) for i in range(n.value)]


def walk(op, n_bits, n_pols, ext_bits, coset_count, launch, g, first=0, count=None):
    """(hi, gt, cc) of workgroups [first, first + count) x steps [0, W) of one launch: uint32 [count, W, 3], NONE where a workgroup
    has no such step"""
    from pil2gl import _lib
    lib = _lib.load()
    count = g.grid - first if count is None else count
    out = np.empty((count, g.walk, 3), np.uint32)
    rc = lib.pil2gl_debug_transform_walk(*_call(op, n_bits, n_pols, ext_bits, coset_count), launch, first, count, out.ctypes.data)
    assert rc == 0, lib.pil2gl_last_error()
    return out


def cover(op, n_bits, n_pols, ext_bits, coset_count, launch):
    """every workgroup x step of one launch through walk_at: (cells (hi, gt, cc) reached exactly once, cells missed, visits beyond a
    cell's first or outside the launch)"""
    from pil2gl import _lib
    lib = _lib.load()
    out = (C.c_uint64 * 3)()
    rc = lib.pil2gl_debug_transform_walk_cover(*_call(op, n_bits, n_pols, ext_bits, coset_count), launch, out)
    assert rc == 0, lib.pil2gl_last_error()
    return tuple(out)
