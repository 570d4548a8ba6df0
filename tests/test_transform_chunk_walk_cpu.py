"""The chunk walk of the 16-slot pass kernels, from the host: a workgroup of ntt_pass_kernel<.., 8, 16> owns one row tile and a run of W
column chunks (csrc/ntt.hip, walk_at); the mid kernel and the other instances go through the same mapping with W = 1.  For every launch of a table of calls: the workgroups x steps reach
each (hi, gt, cc) of the launch exactly once, W >= 1, the grid is not empty, the recorded `blocks` (tiles of the launch) is the sum of
the workgroups' steps, a large launch keeps 4 x 256 workgroups, and only the 16-slot pass instances walk."""
import numpy as np
import pytest

pytest.importorskip("pil2gl")
import transform_plan as tp  # noqa: E402
import transform_walk as tw  # noqa: E402

ROWS = (8, 9, 16, 17, 24, 27)
COLS = (16, 17, 31, 32, 33, 100, 112, 200)
DUMP_LIMIT = 1 << 20            # launches of up to this many workgroup-steps are also enumerated here, cell by cell, with numpy


def _calls(n_bits):
    yield "fft", 0, 0
    yield "ifft", 0, 0
    for op in ("interpolate", "extend_coefs"):
        for eb in range(4):
            yield op, eb, 0                                 # the whole extension
            if eb >= 2:
                yield op, eb, 2                             # a slice of two cosets (where it starts does not reach the plan)
            if eb == 3:
                yield op, eb, 3


@pytest.fixture(autouse=True)
def _no_hooks(monkeypatch):
    for k in ("PIL2GL_NTT_KMAX", "PIL2GL_NTT_GENERIC", "PIL2GL_LDE_WIDEFWD"):
        monkeypatch.delenv(k, raising=False)


def _check_launch(call, i, l, g):
    assert g.walk >= 1 and g.grid >= 1, (call, i, g)
    assert g.chunks == l.chunks and g.tiles * g.chunks == l.blocks, (call, i, l, g)
    runs = -(-g.chunks // g.walk)
    assert g.grid == g.tiles * runs, (call, i, g)
    if l.fixed != 16 or l.kind == "m":
        assert g.walk == 1 and g.grid == l.blocks, (call, i, l, g)      # the other instances keep one chunk per workgroup
    if l.blocks >= 1024:
        assert g.grid >= 1024, (call, i, l, g)              # several workgroups per CU slot wherever the launch has them
    once, missed, extra = tw.cover(*call, i)
    assert (once, missed, extra) == (l.blocks, 0, 0), (call, i, l, g)
    if g.grid * g.walk <= DUMP_LIMIT:
        w = tw.walk(*call, i, g).reshape(-1, 3).astype(np.int64)
        w = w[w[:, 2] != tw.NONE]
        assert len(w) == l.blocks, (call, i)                # blocks = the steps of all workgroups
        assert (w[:, 1] < g.group_tiles).all() and (w[:, 0] * g.group_tiles + w[:, 1] < g.tiles).all() and (w[:, 2] < g.chunks).all()
        key = (w[:, 0] * g.group_tiles + w[:, 1]) * g.chunks + w[:, 2]
        assert (np.sort(key) == np.arange(l.blocks)).all(), (call, i)


@pytest.mark.parametrize("n_bits", ROWS)
def test_every_launch_reaches_each_tile_chunk_once(n_bits):
    walked = 0
    for cols in COLS:
        for op, eb, cosets in _calls(n_bits):
            call = (op, n_bits, cols, eb, cosets)
            plan, grids = tp.plan(*call), tw.grids(*call)
            assert len(plan) == len(grids) and plan
            for i, (l, g) in enumerate(zip(plan, grids)):
                _check_launch(call, i, l, g)
                walked += g.walk > 1
    # whole 8-stage passes are what walks: 2^8, 2^16 and 2^24 rows have them at every width of the table (the other row counts split
    # into shorter passes, which run the any-geometry instances, around a mid kernel that keeps one tile per workgroup)
    assert walked or n_bits % 8


def test_a_workgroup_walks_consecutive_chunks_of_one_tile_and_runs_of_a_tile_share_an_xcd():
    """the walk as the kernels need it: the steps of a workgroup are consecutive chunks of ONE (hi, gt), a last shorter run takes the
    remainder (100 columns: 7 chunks, 800 columns: 50), and the runs of one row tile are workgroups b, b + 8, .. -- one XCD, one L2"""
    call = ("interpolate", 16, 100, 3, 0)
    plan, grids = tp.plan(*call), tw.grids(*call)
    assert [(l.kind, l.fixed, l.chunks) for l in plan] == [("i", 16, 7), ("m", 16, 7), ("d", 16, 50)]
    assert grids[1].walk == 1 and grids[1].grid == plan[1].blocks          # the mid kernel: one tile per workgroup
    for i, g in ((0, grids[0]), (2, grids[2])):
        assert 1 < g.walk < g.chunks and g.chunks % g.walk       # a remainder run
        w = tw.walk(*call, i, g).astype(np.int64)
        have = w[:, :, 2] != tw.NONE
        assert have[:, 0].all()                             # no workgroup without work
        steps = have.sum(axis=1)
        assert (have == (np.arange(g.walk)[None, :] < steps[:, None])).all()
        assert sorted(set(steps)) == [g.chunks % g.walk, g.walk]
        for s in range(1, g.walk):
            m = have[:, s]
            assert (w[m, s, :2] == w[m, 0, :2]).all() and (w[m, s, 2] == w[m, 0, 2] + s).all()
        tile = w[:, 0, 0] * g.group_tiles + w[:, 0, 1]
        assert g.grid % 8 == 0
        for t in (0, 1, g.tiles - 1):
            assert len(set(np.nonzero(tile == t)[0] % 8)) == 1


def test_headline_launches_walk_whole_rows_of_chunks():
    """2^24 x 100 by 3 bits: every row tile has far more than 4 x 256 peers, so a workgroup takes all the chunks of its tile -- 7 on the
    trace side, 50 on the extended matrix -- and builds its tables once"""
    call = ("interpolate", 24, 100, 3, 0)
    assert [(l.kind, g.walk, g.grid) for l, g in zip(tp.plan(*call), tw.grids(*call))] == [
        ("i", 7, 1 << 16), ("i", 7, 1 << 16), ("m", 1, 7 << 16), ("d", 50, 1 << 16), ("d", 50, 1 << 16)]


def test_the_debug_entries_refuse_what_the_plan_refuses():
    import ctypes as C
    from pil2gl import _lib
    lib = _lib.load()
    n, out = C.c_uint32(), (C.c_uint64 * 3)()
    assert lib.pil2gl_debug_plan_transform_grid(0, 31, 1, 31, 0, None, 0, C.byref(n)) != 0
    assert lib.pil2gl_debug_plan_transform_grid(4, 9, 1, 9, 0, None, 0, C.byref(n)) != 0
    assert lib.pil2gl_debug_transform_walk_cover(0, 16, 100, 16, 0, 2, out) != 0         # two launches: no launch 2
    buf = (C.c_uint32 * 6)()
    assert lib.pil2gl_debug_transform_walk(0, 8, 17, 8, 0, 0, 1, 1, buf) != 0           # one workgroup: none at 1
    assert lib.pil2gl_debug_transform_walk(0, 8, 17, 8, 0, 0, 0, 1, buf) == 0
    assert list(buf) == [0, 0, 0, 0, 0, 1]
