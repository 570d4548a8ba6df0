"""The BN254 Poseidon parameter tables (csrc/bn_params.cpp) checked on the host: tests/bn_params_dump.cpp, built with the address and
undefined-behaviour sanitizers, writes the three blobs and the named offsets of every width t = 2..17 once; the tests read them.
  * tests/golden/bn_params_digests.json: SHA-256 of every blob and every offset as the commit BEFORE this unit existed uploaded them
    (recorded from that commit's code compiled host-only, its two device calls replaced by malloc / memcpy);
  * the dense constants against the oracle's generator, the sparse form of the partial rounds against the oracle's permutation, the
    operand tiles and row constants against the integer model tools/bn_mfma_model.py -- none of it through a kernel."""
import hashlib
import json
import os
import random
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pil2-stark-js_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import bn128_oracle as O          # noqa: E402
import bn_mfma_model as MM        # noqa: E402

R = O.R
WIDTHS = range(2, 18)
DEEP = (2, 3, 5, 17)              # perm_small's widths, the smallest sparse width, the arity-16 width (rp % 4 == 0)
MONT_INV = pow(1 << 256, -1, R)


class Tables:
    """the dump of one width: words of the element / constant tables as integers, the tile table as bytes, the offsets"""
    def __init__(self, d, t, off):
        self.t, self.rp, self.off = t, off["rp"], off
        self.blob = {k: open(os.path.join(d, "t%02d.%s" % (t, k)), "rb").read() for k in ("elems", "tiles", "consts")}
        self.elems = [int.from_bytes(self.blob["elems"][i:i + 32], "little") for i in range(0, len(self.blob["elems"]), 32)]
        self.consts = [int.from_bytes(self.blob["consts"][i:i + 32], "little") for i in range(0, len(self.blob["consts"]), 32)]

    def raw(self, name, n):            # n elements of a region of the element table as stored (Montgomery form)
        return self.elems[self.off[name]:self.off[name] + n]

    def plain(self, name, n):
        return [v * MONT_INV % R for v in self.raw(name, n)]

    def tile(self, name, k):           # tile k of a region of the tile table
        o = (self.off[name] + k) * 1024
        return self.blob["tiles"][o:o + 1024]


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    d = tmp_path_factory.mktemp("bn_params")
    exe = str(d / "bn_params_dump")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                           os.path.join(ROOT, "tests", "bn_params_dump.cpp"), os.path.join(CSRC, "bn_params.cpp"), "-o", exe])
    run = subprocess.run([exe, str(d)], capture_output=True, text=True)
    assert run.returncode == 0 and run.stderr == "", "sanitizer report or failure:\n" + run.stderr        # -fno-sanitize-recover: a report is also a non-zero exit
    offs = json.load(open(d / "offsets.json"))
    return {t: Tables(str(d), t, offs[str(t)]) for t in WIDTHS}


def test_blobs_and_offsets_equal_the_parent_commits(dump):
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "bn_params_digests.json")))
    assert sorted(want) == sorted(str(t) for t in WIDTHS)
    for t in WIDTHS:
        assert dump[t].off == want[str(t)]["offsets"], t
        assert {k: hashlib.sha256(b).hexdigest() for k, b in dump[t].blob.items()} == want[str(t)]["sha256"], t


def test_dense_constants_equal_the_oracles_generator(dump):
    for t in WIDTHS:
        T = dump[t]
        C, M = O.poseidon_constants(t)
        assert T.rp == O.N_ROUNDS_P[t - 2]
        assert T.plain("Cd", (8 + T.rp) * t) == list(C), t
        assert T.plain("M", t * t) == [M[i][j] for i in range(t) for j in range(t)], t
        assert T.off["m00"] == T.off["M"]


_D = {}


def closing_matrix(T):
    """D = Mh^RP, Mh = M without its first row and column, from the dumped M (computed once per width)"""
    t, n = T.t, T.t - 1
    if t in _D:
        return _D[t]
    M = T.plain("M", t * t)
    Mh = [[M[(i + 1) * t + 1 + j] for j in range(n)] for i in range(n)]
    D = [[int(i == j) for j in range(n)] for i in range(n)]
    for _ in range(T.rp):
        D = [[sum(Mh[i][q] * D[q][j] for q in range(n)) % R for j in range(n)] for i in range(n)]
    _D[t] = D
    return D


def sparse_permutation(T, D, st):
    """the permutation as the kernels' tables state it (csrc/bn_params.cpp derive_sparse), plain integers: four full rounds on C8 and M, RP
    partial rounds u' = [[m00, V_k], [W_k, I]] sigma(u + S_k e0), the closing layer diag(1, D), four full rounds"""
    t, n, rp = T.t, T.t - 1, T.rp
    C8, M, S, V, W = T.plain("C8", 8 * t), T.plain("M", t * t), T.plain("S", rp), T.plain("V", rp * n), T.plain("W", rp * n)
    m00 = T.plain("m00", 1)[0]

    def full(st, r):
        st = [pow((a + c) % R, 5, R) for a, c in zip(st, C8[r * t:(r + 1) * t])]
        return [sum(M[i * t + j] * st[j] for j in range(t)) % R for i in range(t)]
    for r in range(4):
        st = full(st, r)
    x0, y = st[0], st[1:]
    for k in range(rp):
        z = pow((x0 + S[k]) % R, 5, R)
        x0 = (m00 * z + sum(V[k * n + j] * y[j] for j in range(n))) % R
        y = [(y[j] + W[k * n + j] * z) % R for j in range(n)]
    st = [x0] + [sum(D[i][j] * y[j] for j in range(n)) % R for i in range(n)]
    for r in range(4, 8):
        st = full(st, r)
    return st


@pytest.mark.parametrize("t", DEEP)
def test_sparse_form_equals_the_oracles_permutation(dump, t):
    T = dump[t]
    D = closing_matrix(T)
    rnd = random.Random(0xB254 + t)
    for st in ([0] * t, [R - 1] * t, [rnd.randrange(R) for _ in range(t)]):
        assert sparse_permutation(T, D, st) == O.poseidon(st[1:], st[0], t), t


@pytest.mark.parametrize("t", DEEP)
def test_dense_tiles_and_row_constants_equal_the_model(dump, t):
    """Mt multiplies S-box outputs, which carry 2^-20 (bn_field29.cuh): its coefficients are M_ij 2^20; Dt reads the columns the blocks left: D_ij.
    Folded into the row constants, as stored (Montgomery form): after layer 0..2 and 4..6 the next full round's C8, after layer 3 S[0] on row 0,
    after the last layer nothing; after the closing layer C8[4] on elements 1..n."""
    T, n = dump[t], t - 1
    M, D = T.plain("M", t * t), closing_matrix(T)
    Ms = [a * (1 << 20) % R for a in M]
    for k in range(t * t):
        assert MM.decode_tile(T.tile("Mt", k)) == MM.tile_values(Ms[k]), (t, k)
    for k in range(n * n):
        assert MM.decode_tile(T.tile("Dt", k)) == MM.tile_values(D[k // n][k % n]), (t, k)
    C8, S0 = T.raw("C8", 8 * t), T.raw("S", 1)[0]
    for i in range(t):
        own = MM.row_const(Ms[i * t:(i + 1) * t])
        for inst in range(8):
            fold = (S0 if i == 0 else 0) if inst == 3 else C8[(inst + 1) * t + i] if inst < 7 else 0
            assert T.consts[T.off["MK"] + inst * t + i] == (own + fold) % R, (t, inst, i)
    for i in range(n):
        assert T.consts[T.off["DK"] + i] == (MM.row_const(D[i]) + C8[4 * t + 1 + i]) % R, (t, i)
