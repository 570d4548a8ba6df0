"""The kernels every proof runs between the transforms, the evaluator and the hashes -- the column sums of csrc/dot.hip, the step
helpers and the FRI fold of csrc/fri.hip, the stage-2 scans of csrc/hints.hip -- at the sizes where their launch geometry changes.
Every comparison is exact equality of canonical words against the host oracle (oracle/gl_oracle.c) or Python integers.

Which constant each shape crosses (move the shape when the constant moves):

cols_dot_kernel / cols_dot_final_kernel (pil2gl_cols_dot_ext_range_dev, csrc/dot.hip)
  - `rpc = 1024` rows per chunk (dot.hip:738): a lane's six unreduced 64-bit sums take 1024 products below 2^54 (dot.hip:403-404).
    1024 rows of maximal halves and limbs fill one chunk; 1025 start a one-row second chunk; 2048 fill two.
  - `nGroups = min(64, nChunks)` (dot.hip:741): 2^16 rows are 64 chunks (per = 1), 2^17 rows 128 chunks (per = 2).
  - `threads = min(256, ..)` and `grid.y = ceil(width / threads)` (dot.hip:753-754): a total width of 288 puts columns 256..287 in a
    second blockIdx.y; the eight-matrix case totals exactly 256, one full block.
  - `CD_MAXSEG = 8` (dot.hip:357): eight matrices pass, nine are refused.
  - `nLev > 4` (dot.hip:729): five weight vectors take two sweeps.
x_div_x_sub_xi_kernel (fri.hip:136)
  - `XD_BATCH = 16` (fri.hip:134) and 256 threads: blocks = ceil(ceil(E / 16) / 256) (fri.hip:507).  E < 16 (nBitsExt 0..3): a lane has
    one row; E = 2^12: one block, every batch full; E = 2^13, 2^14: two and four blocks, T = 512 and 1024.
  - `cosetCount > 256` is refused (fri.hip:492): 256 is the largest slice, 512 the first refused.
  - the norm's constants (fri.hip:500-505) vanish term by term at b = 0, c = 0: opening points with either or both zero.
one_row_zerofier_kernel (fri.hip:81): `CH = 8` rows per lane (fri.hip:83); 2^nBitsExt < 8 leaves tail slots that re-read row i0.
frame_zerofier_kernel (fri.hip:95): no roots -> upload_small (fri.hip:345) stages an empty table.
periodic_kernel behind build_zhinv (fri.hip:352): nBitsExt == nBits is a one-entry table.
fri_horner_kernel + the group iNTT (fri.hip:28, 229): nX = 2^(polBits - outBits) = 1 (no transform, ntt.hip:574), 2 over 3 * 2^16
    columns (768 column chunks of a one-stage pass, ntt.hip:361), 2^12 (two passes), 2^5 over 2^13 groups; scratch slot SCR_FRI_COEF
    (fri.hip:237) re-used by back-to-back calls.  pil2gl_fri_verify_fold: foldBits = 0 skips the transform (fri.hip:256).
hint_scan1/2/3 (hints.hip:45, 93, 107): `SCAN_CHUNK = 256 * 8 = 2048` (hints.hip:17); hint_scan2's 256 threads walk
    per = ceil(nb / 256) block totals (hints.hip:95): n = 524289 gives nb = 257, per = 2; n = 1048581 gives nb = 513, per = 3.
    Zero denominators at rows 2047 | 2048 (a chunk edge), 2055 | 2056 (the first lane batch's edge in the second chunk),
    524287 | 524288 (the edge between chunks 255 and 256: at per = 2 between the totals of hint_scan2's lanes 127 and 128, at per = 3
    between two totals of lane 85).
evals_partial_kernel (fri.hip:181): `nBlocks = min(256, N / 256)` (fri.hip:595): above 65536 rows the grid-stride loop takes a second trip.

No shape of the list was dropped: the oracle takes nBitsExt == nBits, nBits = 0 and empty root lists, as the reference's
polutils.js:39-102 does (F.w[0] = 1).  The tests named test_reference_side_* need no device.
"""
import ctypes as C

import numpy as np
import pytest

from conftest import P, rand_field

pytestmark = pytest.mark.gpu

EINVAL = -1
INV7 = pow(7, P - 2, P)


@pytest.fixture(scope="module")
def gl():
    import pil2gl
    pil2gl.init(0)
    return pil2gl


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


def dev_filled(n, word=0):
    import torch
    return torch.full((n,), word, dtype=torch.int64, device="cuda")


def host(t):
    return t.cpu().numpy().view(np.uint64)


def same(got, want, what=""):
    got, want = np.asarray(got, dtype=np.uint64).reshape(-1), np.asarray(want, dtype=np.uint64).reshape(-1)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, "%s: %d words differ, first at %d: got %#x, want %#x" % (what, bad.size, bad[0], int(got[bad[0]]), int(want[bad[0]]))


def root_of_unity(bits):
    w = 7277203076849721926
    for _ in range(32 - bits):
        w = w * w % P
    return w


# ------------------------------------------------------------------------------------------------------------------ opening points
A_BASE = 5          # a base-field point that is no row of any coset 7<w> used here (checked in test_reference_side_opening_points_are_legal)


def opening_points():
    """a random extension point, then the points at which terms of the norm's polynomial (fri.hip:500-505) vanish"""
    rng = np.random.default_rng(2024)
    r = [int(v) for v in rand_field(rng, 6)]
    a, b, c = r[3] | 1, r[4] | 1, r[5] | 1          # non-zero
    return [(r[0], r[1], r[2]), (A_BASE, 0, 0), (a, b, 0), (a, 0, c), (0, b, c), (0, 0, c)]


POINT_PAIRS = [(0, 1), (2, 3), (4, 5)]              # two openings interleaved per table
XDIV_BITS = [0, 1, 2, 3, 4, 12, 13, 14]
LEV_BITS = [0, 1, 3, 4, 13]


def ext_pow(x, e):
    """x^e in the cubic extension u^3 = u + 1 (f3g.js:94-102), Python integers"""
    def mul(p, q):
        a0, a1, a2 = p; b0, b1, b2 = q
        d0, d1, d2, d3, d4 = a0 * b0, a0 * b1 + a1 * b0, a0 * b2 + a1 * b1 + a2 * b0, a1 * b2 + a2 * b1, a2 * b2
        # u^3 = u + 1, u^4 = u^2 + u
        return ((d0 + d3) % P, (d1 + d3 + d4) % P, (d2 + d4) % P)
    r = (1, 0, 0)
    while e:
        if e & 1:
            r = mul(r, x)
        x = mul(x, x); e >>= 1
    return r


def test_reference_side_opening_points_are_legal():
    """the table refuses a base-field xi with (xi / 7)^E = 1 and LEv leaves its closed form where xi^N = 1: none of the points is one"""
    for nbe in XDIV_BITS:
        assert pow(A_BASE * INV7, 2 ** nbe, P) != 1
    for xi in opening_points():
        assert all(0 <= v < P for v in xi) and any(xi)
        for nb in LEV_BITS:
            assert ext_pow(xi, 1 << nb) != (1, 0, 0), (xi, nb)
        for nbe in XDIV_BITS:
            if xi[1] == 0 and xi[2] == 0:
                assert pow(xi[0] * INV7, 2 ** nbe, P) != 1


def test_reference_side_unreduced_sums_fit():
    """the bound the limb-extreme case leans on: a full chunk of maximal (u32 half) x (22-bit limb) products stays below 2^64"""
    assert 1024 * (2 ** 32 - 1) * (2 ** 22 - 1) < 2 ** 64
    assert 1025 * (2 ** 32 - 1) * (2 ** 22 - 1) >= 2 ** 64        # and not one row more: the chunk cannot grow
    w = 0xFFFFEFFFFFFFFFFF
    assert w < P and (w & 0x3FFFFF, (w >> 22) & 0x3FFFFF, w >> 44) == (0x3FFFFF, 0x3FFFFF, 0xFFFFE)
    assert 0xFFFFFFFEFFFFFFFF < P


ZEROFIER_ONE_ROW = [(0, 0), (0, 1), (1, 2), (2, 2), (1, 3)]
ZHINV_SHAPES = [(3, 3), (0, 2), (9, 13)]
FRAME_SHAPE, FRAMES = (5, 7), [(0, 0), (0, 3), (3, 0), (1, 1)]


def test_reference_side_oracle_takes_the_degenerate_zerofier_shapes(oracle):
    """the oracle at nBitsExt == nBits, nBits = 0 and an empty frame, against polutils.js:39-102 written out in Python integers"""
    def xs(nbe):
        w = root_of_unity(nbe)
        return [7 * pow(w, i, P) % P for i in range(1 << nbe)]

    def zh(nb, nbe):
        ext = 1 << (nbe - nb); we = root_of_unity(nbe - nb); sn = pow(7, 1 << nb, P)
        t = [(sn * pow(we, i, P) - 1) % P for i in range(ext)]
        assert all(t)
        return [t[i % ext] for i in range(1 << nbe)]
    for nb, nbe in ZHINV_SHAPES:
        assert oracle.build_zhinv(nb, nbe).tolist() == [pow(z, P - 2, P) for z in zh(nb, nbe)]
    for nb, nbe in ZEROFIER_ONE_ROW:
        for row in range(1 << nb):
            root = pow(root_of_unity(nb), row, P)
            want = [z * pow((x - root) % P, P - 2, P) % P for x, z in zip(xs(nbe), zh(nb, nbe))]
            assert oracle.build_one_row_zerofier_inv(nb, nbe, row).tolist() == want, (nb, nbe, row)
    nb, nbe = FRAME_SHAPE
    for lo, hi in FRAMES:
        roots = [pow(root_of_unity(nb), i, P) for i in range(lo)] + [pow(root_of_unity(nb), (1 << nb) - i - 1, P) for i in range(hi)]
        want = []
        for x in xs(nbe):
            z = 1
            for r in roots:
                z = z * (x - r) % P
            want.append(z)
        assert oracle.build_frame_zerofier(nb, nbe, lo, hi).tolist() == want, (lo, hi)
    assert oracle.build_frame_zerofier(nb, nbe, 0, 0).tolist() == [1] * (1 << nbe)
    # the smallest tables of the other helpers the device tests lean on
    assert oracle.lev(0, np.array([3, 4, 5], dtype=np.uint64)).tolist() == [[1, 0, 0]]
    t = oracle.x_div_x_sub_xi(0, np.array([[A_BASE, 0, 0]], dtype=np.uint64))
    assert t.tolist() == [[7 * pow(7 - A_BASE, P - 2, P) % P, 0, 0]]


# ------------------------------------------------------------------------------------------------------------------ 1. column sums
def cols_dot(gl, dmats, strides, col_begin, widths, n_rows, row_step, dlevs):
    """pil2gl_cols_dot_ext_range_dev (col_begin given) or pil2gl_cols_dot_ext_multi_dev -> (rc, [nLev x width x 3 per matrix])"""
    lib = gl._lib.load()
    n = len(dmats)
    ptrs = (C.c_void_p * n)(*[t.data_ptr() for t in dmats])
    lv = (C.c_void_p * len(dlevs))(*[t.data_ptr() for t in dlevs])
    outs = [np.full((len(dlevs), w, 3), 0xDEAD, np.uint64) for w in widths]
    po = (C.c_void_p * n)(*[o.ctypes.data for o in outs])
    ws = np.array(widths, dtype=np.uint64); st = np.array(strides, dtype=np.uint64)
    if col_begin is None:
        assert list(strides) == list(widths)
        rc = lib.pil2gl_cols_dot_ext_multi_dev(ptrs, C.c_void_p(ws.ctypes.data), n, n_rows, row_step, lv, len(dlevs), po, None)
    else:
        cb = np.array(col_begin, dtype=np.uint64)
        rc = lib.pil2gl_cols_dot_ext_range_dev(ptrs, C.c_void_p(st.ctypes.data), C.c_void_p(cb.ctypes.data), C.c_void_p(ws.ctypes.data), n,
                                               n_rows, row_step, lv, len(dlevs), po, None)
    return rc, outs


def int_col_sums(m, levs):
    """[nLev][width][3] of sum_k m[k][c] * lev[l][k][q] mod P, Python integers"""
    mo = m.astype(object).T
    return np.array([(mo @ l.astype(object)) % P for l in levs], dtype=np.uint64)


@pytest.mark.parametrize("n_rows", [1024, 1025, 2048])
def test_cols_dot_full_chunk_of_maximal_limbs(gl, n_rows):
    """one matrix of constant columns with both halves at (or next to) their maximum against weights whose three limbs are: a chunk's
    1024 products per unreduced sum are the largest the operands allow, and a 1025th in the same sum would wrap"""
    assert 1024 * (2 ** 32 - 1) * (2 ** 22 - 1) < 2 ** 64           # the reference's own worst unreduced sum
    rng = np.random.default_rng(n_rows)
    m = np.empty((n_rows, 4), np.uint64)
    m[:, 0] = 0xFFFFFFFEFFFFFFFF; m[:, 1] = P - 1; m[:, 2] = 0x00000000FFFFFFFF; m[:, 3] = rand_field(rng, n_rows)
    levs = [np.full((n_rows, 3), 0xFFFFEFFFFFFFFFFF, np.uint64), np.full((n_rows, 3), P - 1, np.uint64), rand_field(rng, (n_rows, 3))]
    want = np.zeros((3, 4, 3), np.uint64)
    for l in range(3):
        for c in range(4):
            for q in range(3):
                want[l, c, q] = sum(int(a) * int(b) for a, b in zip(m[:, c].tolist(), levs[l][:, q].tolist())) % P
    for range_form in (False, True):
        rc, outs = cols_dot(gl, [dev(m)], [4], [0] if range_form else None, [4], n_rows, 1, [dev(l) for l in levs])
        assert rc == 0
        same(outs[0], want, "n_rows %d" % n_rows)


def test_cols_dot_column_ranges_across_the_block_boundary(gl, oracle):
    """columns [colBegin, colBegin + width) of matrices with longer rows; every cell outside the ranges is P - 1, so a read that
    strays changes its sum; the third range lies across column 256 of the launch (the second blockIdx.y)"""
    strides, begins, widths = (37, 9, 300), (5, 0, 41), (20, 9, 259)
    assert sum(widths) == 288
    nb, eb, n_lev = 10, 2, 3
    rng = np.random.default_rng(77)
    mats, compact = [], []
    for s, b, w in zip(strides, begins, widths):
        m = np.full((1 << (nb + eb), s), P - 1, np.uint64)
        m[:, b:b + w] = rand_field(rng, (m.shape[0], w))
        mats.append(m); compact.append(np.ascontiguousarray(m[:, b:b + w]))
    levs = [rand_field(rng, (1 << nb, 3)) for _ in range(n_lev)]
    dlevs = [dev(l) for l in levs]
    rc, outs = cols_dot(gl, [dev(m) for m in mats], strides, begins, widths, 1 << nb, 1 << eb, dlevs)
    assert rc == 0
    for k, (m, b, w) in enumerate(zip(mats, begins, widths)):
        want = np.array([[oracle.eval_pol_at(m, b + c, 1, nb, eb, levs[l]) for c in range(w)] for l in range(n_lev)], dtype=np.uint64)
        same(outs[k], want, "matrix %d" % k)
    rc, outs2 = cols_dot(gl, [dev(m) for m in compact], widths, None, widths, 1 << nb, 1 << eb, dlevs)
    assert rc == 0
    for k in range(3):
        same(outs2[k], outs[k], "compacted matrix %d" % k)
    # a range that leaves its matrix is refused and nothing is written
    rc, outs3 = cols_dot(gl, [dev(m) for m in mats], strides, (5, 1, 41), widths, 1 << nb, 1 << eb, dlevs)
    assert rc == EINVAL and all((o == 0xDEAD).all() for o in outs3)


def test_cols_dot_eight_matrices_and_not_nine(gl):
    widths = (1, 2, 3, 31, 32, 33, 64, 90)
    assert sum(widths) == 256
    n_rows = 256
    rng = np.random.default_rng(8)
    mats = [rand_field(rng, (n_rows, w)) for w in widths]
    levs = [rand_field(rng, (n_rows, 3)) for _ in range(2)]
    dlevs = [dev(l) for l in levs]
    rc, outs = cols_dot(gl, [dev(m) for m in mats], widths, None, widths, n_rows, 1, dlevs)
    assert rc == 0
    for k, m in enumerate(mats):
        same(outs[k], int_col_sums(m, levs), "matrix %d of 8" % k)
    for range_form in (False, True):
        w9 = widths + (4,)
        m9 = [dev(m) for m in mats] + [dev(rand_field(rng, (n_rows, 4)))]
        rc, outs = cols_dot(gl, m9, w9, [0] * 9 if range_form else None, w9, n_rows, 1, dlevs)
        assert rc == EINVAL and all((o == 0xDEAD).all() for o in outs)


@pytest.mark.parametrize("nb,n_lev", [(16, 2), (17, 2), (10, 5), (10, 4)])
def test_cols_dot_two_stage_reduction_and_sweeps(gl, oracle, nb, n_lev):
    """64 chunks (one per group of the first reduction), 128 chunks (two per group); five weight vectors (two sweeps) beside four (one)"""
    width = 6
    rng = np.random.default_rng(100 * nb + n_lev)
    m = rand_field(rng, (1 << nb, width))
    levs = [rand_field(rng, (1 << nb, 3)) for _ in range(n_lev)]
    rc, outs = cols_dot(gl, [dev(m)], [width], None, [width], 1 << nb, 1, [dev(l) for l in levs])
    assert rc == 0
    want = np.array([[oracle.eval_pol_at(m, c, 1, nb, 0, levs[l]) for c in range(width)] for l in range(n_lev)], dtype=np.uint64)
    same(outs[0], want)


# ------------------------------------------------------------------------------------------------------------------ 2. x / (x - xi), LEv
def xdiv_table(gl, nbe, eb, xis, cb, cc, sentinel=0):
    """both forms of the call -> (rc of the last call, rows x 3 nOpen table)"""
    lib = gl._lib.load()
    rows = (1 << (nbe - eb)) * cc
    d = dev_filled(rows * 3 * len(xis), sentinel)
    rc = 0
    for i, xi in enumerate(xis):
        a = np.array(xi, dtype=np.uint64)
        if eb == 0 and (cb, cc) == (0, 1):
            rc = lib.pil2gl_x_div_x_sub_xi_dev(nbe, C.c_void_p(a.ctypes.data), len(xis), i, C.c_void_p(d.data_ptr()), None)
        else:
            rc = lib.pil2gl_x_div_x_sub_xi_cosets_dev(nbe, eb, C.c_void_p(a.ctypes.data), len(xis), i, cb, cc, C.c_void_p(d.data_ptr()), None)
        if rc:
            break
    return rc, host(d).reshape(rows, 3 * len(xis))


@pytest.mark.parametrize("nbe", XDIV_BITS)
def test_x_div_x_sub_xi_small_tables_and_several_blocks(gl, oracle, nbe):
    pts = opening_points()
    for i, j in POINT_PAIRS:
        xis = np.array([pts[i], pts[j]], dtype=np.uint64)
        rc, got = xdiv_table(gl, nbe, 0, xis, 0, 1)
        assert rc == 0
        same(got, oracle.x_div_x_sub_xi(nbe, xis), "nBitsExt %d, points %d and %d" % (nbe, i, j))


def test_x_div_x_sub_xi_coset_slices_up_to_256(gl, oracle):
    nbe, eb = 14, 9
    pts = opening_points()
    for i, j in POINT_PAIRS:
        xis = np.array([pts[i], pts[j]], dtype=np.uint64)
        full = oracle.x_div_x_sub_xi(nbe, xis).reshape(1 << (nbe - eb), 1 << eb, 6)
        for cb, cc in [(0, 256), (256, 256), (511, 1), (3, 1)]:
            rc, got = xdiv_table(gl, nbe, eb, xis, cb, cc)
            assert rc == 0
            same(got, full[:, cb:cb + cc].reshape(-1, 6), "cosets [%d, %d), points %d and %d" % (cb, cb + cc, i, j))
    sentinel = 0x5EA15EA15EA15EA1
    rc, got = xdiv_table(gl, nbe, eb, xis, 0, 512, sentinel)
    assert rc == EINVAL and (got == np.uint64(sentinel)).all()


@pytest.mark.parametrize("nb", LEV_BITS)
def test_lev_at_small_and_multi_block_sizes(gl, oracle, nb):
    lib = gl._lib.load()
    for k, xi in enumerate(opening_points()):
        a = np.array(xi, dtype=np.uint64)
        d = dev_filled(3 << nb, 0x7777)
        assert lib.pil2gl_build_lev_dev(nb, C.c_void_p(a.ctypes.data), C.c_void_p(d.data_ptr()), None) == 0
        same(host(d), oracle.lev(nb, a), "nBits %d, point %d" % (nb, k))


# ------------------------------------------------------------------------------------------------------------------ 3. zerofier tables
def test_one_row_zerofier_below_one_lane_batch(gl, oracle):
    lib = gl._lib.load()
    for nb, nbe, rows in [(a, b, range(1 << a)) for a, b in ZEROFIER_ONE_ROW] + [(9, 13, [257])]:
        for row in rows:
            d = dev_filled(1 << nbe, 0x7777)
            assert lib.pil2gl_build_one_row_zerofier_inv_dev(nb, nbe, row, C.c_void_p(d.data_ptr()), None) == 0
            same(host(d), oracle.build_one_row_zerofier_inv(nb, nbe, row), "(%d, %d) row %d" % (nb, nbe, row))


def test_zhinv_one_entry_table(gl, oracle):
    lib = gl._lib.load()
    for nb, nbe in ZHINV_SHAPES:
        d = dev_filled(1 << nbe, 0x7777)
        assert lib.pil2gl_build_zhinv_dev(nb, nbe, C.c_void_p(d.data_ptr()), None) == 0
        same(host(d), oracle.build_zhinv(nb, nbe), "(%d, %d)" % (nb, nbe))


def test_frame_zerofier_with_and_without_roots(gl, oracle):
    lib = gl._lib.load()
    nb, nbe = FRAME_SHAPE
    for lo, hi in FRAMES:
        d = dev_filled(1 << nbe, 0x7777)
        assert lib.pil2gl_build_frame_zerofier_dev(nb, nbe, lo, hi, C.c_void_p(d.data_ptr()), None) == 0
        same(host(d), oracle.build_frame_zerofier(nb, nbe, lo, hi), "frame (%d, %d)" % (lo, hi))
        if (lo, hi) == (0, 0):
            assert (host(d) == 1).all()


# ------------------------------------------------------------------------------------------------------------------ 4. FRI fold
FOLDS = [(0, 0), (1, 0), (1, 1), (6, 6), (16, 4), (17, 16), (18, 13), (13, 0)]


@pytest.mark.parametrize("pol_bits,out_bits", FOLDS)
def test_fri_fold_group_sizes(gl, oracle, pol_bits, out_bits):
    """nX = 1 (no transform), 2 over 3 * 2^16 columns, 2^12 and 2^13 (two passes of the group transform), 2^5 over 2^13 groups"""
    lib = gl._lib.load()
    rng = np.random.default_rng(1000 * pol_bits + out_bits)
    pol = rand_field(rng, (1 << pol_bits, 3)); ch = rand_field(rng, 3)
    sinv = oracle.fri_shift_inv(20, pol_bits)           # the shift of a layer 20 - pol_bits squarings down from a 2^20 first layer
    out = np.full((1 << out_bits, 3), 0x7777, np.uint64)
    assert lib.pil2gl_fri_fold(gl._ptr(pol), pol_bits, out_bits, sinv, gl._ptr(ch), gl._ptr(out)) == 0
    same(out, oracle.fri_fold(pol, out_bits, sinv, ch), "(%d, %d)" % (pol_bits, out_bits))


def test_fri_fold_dev_twice_on_one_stream(gl, oracle):
    """the coefficient scratch is re-used by the second call while the first may still be in flight on the same stream"""
    import torch
    lib = gl._lib.load()
    pol_bits, out_bits = 18, 13
    rng = np.random.default_rng(1813)
    pols = [rand_field(rng, (1 << pol_bits, 3)) for _ in range(2)]; ch = rand_field(rng, 3)
    sinv = oracle.fri_shift_inv(20, pol_bits)
    dp = [dev(p) for p in pols]
    outs = [dev_filled(3 << out_bits, 0x7777) for _ in range(3)]
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for p, o in ((0, 0), (0, 1), (1, 2)):               # the same fold twice, then another polynomial straight after
        assert lib.pil2gl_fri_fold_dev(C.c_void_p(dp[p].data_ptr()), pol_bits, out_bits, sinv, gl._ptr(ch), C.c_void_p(outs[o].data_ptr()), st) == 0
    torch.cuda.synchronize()
    want = oracle.fri_fold(pols[0], out_bits, sinv, ch)
    same(host(outs[0]), want, "first call")
    same(host(outs[1]), want, "second call")
    same(host(outs[2]), oracle.fri_fold(pols[1], out_bits, sinv, ch), "third call")


@pytest.mark.parametrize("n_queries", [1, 3, 257])
def test_fri_verify_fold_of_one_element_groups(gl, n_queries):
    """foldBits = 0: a group of one element is its own polynomial, whatever the challenge and the position"""
    lib = gl._lib.load()
    rng = np.random.default_rng(n_queries)
    groups = rand_field(rng, (1, n_queries, 3)); groups[0, 0] = [P - 1, 0, P - 1]
    sinv = rand_field(rng, n_queries); ch = rand_field(rng, 3)
    out = np.full((n_queries, 3), 0x7777, np.uint64)
    assert lib.pil2gl_fri_verify_fold(gl._ptr(groups), 0, n_queries, gl._ptr(sinv), gl._ptr(ch), gl._ptr(out)) == 0
    same(out, groups)
    assert (out < np.uint64(P)).all()


def test_fri_verify_fold_of_4096_element_groups(gl, oracle):
    """foldBits = 12, three queries: each is the prover's fold of its group to one element with the query's own shift"""
    lib = gl._lib.load()
    fold_bits, n_queries = 12, 3
    rng = np.random.default_rng(123)
    groups = rand_field(rng, (1 << fold_bits, n_queries, 3))
    sinv = rand_field(rng, n_queries); sinv[sinv == 0] = 1
    ch = rand_field(rng, 3)
    out = np.full((n_queries, 3), 0x7777, np.uint64)
    assert lib.pil2gl_fri_verify_fold(gl._ptr(groups), fold_bits, n_queries, gl._ptr(sinv), gl._ptr(ch), gl._ptr(out)) == 0
    for q in range(n_queries):
        want = oracle.fri_fold(np.ascontiguousarray(groups[:, q]), 0, int(sinv[q]), ch)
        same(out[q], want, "query %d" % q)


@pytest.mark.parametrize("pol_bits,t_bits", [(0, 0), (5, 0), (5, 5), (13, 4)])
def test_fri_transpose_edges(gl, oracle, pol_bits, t_bits):
    lib = gl._lib.load()
    pol = rand_field(np.random.default_rng(pol_bits * 32 + t_bits), (1 << pol_bits, 3))
    out = np.full((1 << pol_bits, 3), 0x7777, np.uint64)
    assert lib.pil2gl_fri_transpose(gl._ptr(pol), pol_bits, t_bits, gl._ptr(out)) == 0
    same(out, oracle.fri_transpose(pol, t_bits))


# ------------------------------------------------------------------------------------------------------------------ 5. hint scans
@pytest.mark.parametrize("n,dim", [(524289, 3), (524289, 1), (1048581, 3), (1048581, 1)])
def test_hint_scans_past_256_block_totals(gl, oracle, n, dim):
    """hint_scan2's lanes walk two (nb = 257) and three (nb = 513) block totals each.  Then zero denominators (they invert to zero, as
    in the oracle) on both sides of a 2048-row chunk edge, of the next lane batch's edge and of the edge between chunks 255 and 256.
    A zero ratio zeroes every later product, so the product column is also run with its only zero in the last row."""
    rng = np.random.default_rng(n + dim)
    num = rand_field(rng, n * dim); den = rand_field(rng, n * dim)
    den[den == 0] = 1; num[num == 0] = 1
    dn = dev(num)
    zeros = np.array([2047, 2048, 2055, 2056, 524287, 524288])
    dz = den.reshape(n, dim).copy(); dz[zeros] = 0; dz = dz.reshape(-1)
    dl = den.reshape(n, dim).copy(); dl[n - 1] = 0; dl = dl.reshape(-1)
    for what, d in (("no zero", den), ("zeros at the edges", dz), ("zero in the last row", dl)):
        want = oracle.gprod(num, d, dim, dim)
        same(host(gl.calculateZ(dn, dev(d), dim, dim)), want, "product, " + what)
        rows = want.reshape(n, -1)
        if d is dz:
            assert rows[2047].any() and not rows[2048:].any()       # what the third run is for
        else:
            assert rows[n - 1].any()
    for what, d in (("no zero", den), ("zeros at the edges", dz)):
        s = host(gl.calculateS(dn[:dim].contiguous(), dev(d), dim, dim))
        same(s, oracle.gsum(num[:dim], d, dim, dim), "sum, " + what)


# ------------------------------------------------------------------------------------------------------------------ 6. evaluations
def test_compute_evals_grid_stride_second_trip(gl, oracle):
    """2^17 rows: 256 blocks of 256 lanes take two rows each"""
    lib = gl._lib.load()
    nb, eb, width = 17, 1, 5
    rng = np.random.default_rng(171)
    buf = rand_field(rng, (1 << (nb + eb), width)); dbuf = dev(buf)
    levs = [rand_field(rng, (1 << nb, 3)) for _ in range(2)]; dlevs = [dev(l) for l in levs]
    cols = [(0, 1), (1, 3), (4, 1)]
    descs = (gl._lib.EvalDesc * 6)()
    for e in range(6):
        off, dim = cols[e % 3]
        descs[e].buf = dbuf.data_ptr(); descs[e].width = width; descs[e].offset = off; descs[e].dim = dim; descs[e].levIndex = e // 3
    lv = (C.c_void_p * 2)(*[t.data_ptr() for t in dlevs])
    res = np.full((6, 3), 0x7777, np.uint64)
    assert lib.pil2gl_compute_evals_dev(descs, 6, nb, eb, lv, 2, gl._ptr(res), None) == 0
    for e in range(6):
        off, dim = cols[e % 3]
        same(res[e], oracle.eval_pol_at(buf, off, dim, nb, eb, levs[e // 3]), "column %d (dim %d), weights %d" % (off, dim, e // 3))
