"""Chosen mid-round states through the device forms of the BN254 Poseidon permutation (csrc/bn128.hip with bn_mfma.cuh, bn_field29.cuh,
bn_field.cuh), the check of their lazy bounds: tests/bn128_chosen.py builds, for every width, inputs whose S-box input, S-box output
or final state at a chosen round IS 0, R - 1, a power of two, an all-ones limb pattern or a 0x7f / 0x80 byte pattern -- as a plain
value, as Montgomery words or in the form bn29::pow5 leaves -- at the first rounds, around both changes of round kind, in the blocked
partial rounds, in the leftover partial rounds on canonical values (rp % 4 != 0) and at the end.  Random inputs reach such a value
with probability about 2^-29 per operation.

The device forms: perm_small (t = 2..4), the blocked pipeline (t = 5..16) and the single-body form (t = 17) behind bn_perm, reached
with a lane per permutation by batches above 2048 rows; chain_perm, a wave per permutation, by batches up to 2048 and by
poseidon_chain; the leaf kernel's S-box on plain integers (plain_sbox_store) through pil2gl_bn128_linear_hash_rows.
Only final outputs are compared (in a partial round the device holds its own linear image of elements 1..t-1), every one by exact
equality with the oracle."""
import numpy as np
import pytest

from conftest import P, rand_field

import bn128_chosen as bc
import bn128_oracle as orc

pytestmark = pytest.mark.gpu

_GOT = {}


@pytest.fixture(scope="module")
def bn():
    import pil2gl
    pil2gl.init(0)
    from pil2gl import bn128
    return bn128


def _lane_form(bn, t):
    """the 2112-row batch of bc.pipeline_rows(t) through bn_poseidon_kernel, all t outputs -> (rows, outputs), once per width"""
    if ("lane", t) not in _GOT:
        cs, rows = bc.cases(t), bc.pipeline_rows(t)
        assert len(rows) > 2048
        _GOT["lane", t] = rows, bn.poseidon_batch([cs[i].inp[1:] for i in rows], [cs[i].inp[0] for i in rows], t)
    return _GOT["lane", t]


def _wave_form(bn, t):
    """the distinct cases of t in one batch (a wave each: bn_sponge_chain_kernel, chain_perm), all t outputs, once per width"""
    if ("wave", t) not in _GOT:
        cs = bc.cases(t)
        assert len(cs) <= 2048
        _GOT["wave", t] = bn.poseidon_batch([c.inp[1:] for c in cs], [c.inp[0] for c in cs], t)
    return _GOT["wave", t]


def _report(bad, total):
    return "%d of %d differ; the first: %s" % (len(bad), total, bad[:4])


@pytest.mark.parametrize("t", bc.WIDTHS)
def test_lane_per_permutation_pipeline(bn, t):
    """bn_poseidon_kernel (count > 2048), bn_perm: the cases of t cycled over 2112 rows, the first case of every (site, round) on lanes
    0, 31, 32, 63 and one on the last row; neighbouring rows differ (the matrix-core operand of a lane comes from another lane's
    bytes); every row against the oracle"""
    cs = bc.cases(t)
    rows, got = _lane_form(bn, t)
    bad = [(k, k % 64, cs[i]) for k, i in enumerate(rows) if got[k] != cs[i].want]
    assert not bad, _report(bad, len(rows))


@pytest.mark.parametrize("t", bc.WIDTHS)
def test_lane_per_permutation_one_output(bn, t):
    """the same rows with nOut = 1, element 0 alone compared.  pil2gl_bn128_poseidon_dev builds its arguments with perm_args(pf):
    firstOnly is false, so this call does NOT set `nout1` (only the leaf, tree-level and path kernels do, and their element 0 is not
    free to choose); the last linear layer still computes all t rows and this is the check of the output copy: row stride nOut,
    element 0 of the right row, at the edge lanes and the last row"""
    cs, rows = bc.cases(t), bc.pipeline_rows(t)
    got = bn.poseidon_batch([cs[i].inp[1:] for i in rows], [cs[i].inp[0] for i in rows], 1)
    bad = [(k, k % 64, cs[i]) for k, i in enumerate(rows) if got[k] != cs[i].want[:1]]
    assert not bad, _report(bad, len(rows))


@pytest.mark.parametrize("t", bc.WIDTHS)
def test_wave_per_permutation_form(bn, t):
    """chain_perm: the distinct cases in one batch of at most 2048 (a wave each), and each again as a one-block poseidon_chain"""
    cs = bc.cases(t)
    got = _wave_form(bn, t)
    bad = [(k, c) for k, c in enumerate(cs) if got[k] != c.want]
    assert not bad, _report(bad, len(cs))
    bad = [(k, c) for k, c in enumerate(cs) if bn.poseidon_chain([c.inp[1:]], c.inp[0]) != c.want]
    assert not bad, _report(bad, len(cs))


@pytest.mark.parametrize("t", bc.WIDTHS)
def test_lane_and_wave_forms_agree(bn, t):
    """the two forms word for word on all rows (both equal the oracle when the tests above pass: asserted apart, so that a failure
    names the pair of forms and not only the one that left the oracle)"""
    rows, lane = _lane_form(bn, t)
    wave = _wave_form(bn, t)
    cs = bc.cases(t)
    bad = [(k, k % 64, cs[i]) for k, i in enumerate(rows) if lane[k] != wave[i]]
    assert not bad, _report(bad, len(rows))


# ---- the leaf kernel's S-box on plain integers
_M64 = (1 << 64) - 1


def _leaf_rows(width, seed):
    """rows of `width` Goldilocks words, three per field element x (linear_hash_worker's packing: word q at bit 64 q).  The leaf kernel adds
    round 0's constant c of width 17 to x as PLAIN integers (x < 2^192, c < r: no reduction) and S-boxes the sum.  Row (q, d): word q
    of x + c, for every element, is 2^64 - 1 (d = -1), 0 or 1, the words below it random; row (d0, d1, d2): all three words of the
    sum chosen, carries included (x_q = d_q - c_q - carry mod 2^64): runs of all-ones and of zero words with a carry through them.
    A word that would be >= the Goldilocks prime is no input: it is skipped (left random).  -> (rows, chosen, skipped)"""
    C = orc.poseidon_constants(17)[0]
    rng = np.random.default_rng(seed)
    specs = [tuple(d if k == q else None for k in range(3)) for q in range(3) for d in (-1, 0, 1)]
    specs += [(d0, d1, d2) for d0 in (-1, 0, 1) for d1 in (-1, 0, 1) for d2 in (-1, 0, 1)]
    rows = rand_field(rng, (len(specs), width))
    chosen = skipped = 0
    for i, spec in enumerate(specs):
        for e in range((width + 2) // 3):
            c = C[1 + e % 16]                                   # round 0, state element 1 + (position in the chunk)
            carry = 0
            for q, d in enumerate(spec):
                if 3 * e + q >= width:
                    break
                cq = (c >> (64 * q)) & _M64
                if d is not None:
                    v = (d - cq - carry) & _M64
                    if v < P:
                        rows[i, 3 * e + q] = v
                        chosen += 1
                    else:
                        skipped += 1
                carry = (int(rows[i, 3 * e + q]) + cq + carry) >> 64
    return rows, specs, chosen, skipped


@pytest.mark.parametrize("width,custom", [(48, False), (48, True), (100, False), (100, True)])
def test_leaf_kernel_plain_sbox_carry_edges(bn, width, custom):
    """plain_sbox_store (arity 16: the full chunks, and the zero-padded last one when custom): the 32-bit add chain of x + c and the
    S-box's limb split on sums whose 64-bit words are all ones, zero and one; every row against the oracle's leaf digest"""
    import pil2gl
    from pil2gl import _lib
    rows, specs, chosen, skipped = _leaf_rows(width, width + int(custom))
    assert (rows < np.uint64(P)).all() and chosen > 0 and 4 * skipped < chosen + skipped
    C = orc.poseidon_constants(17)[0]
    for i, spec in enumerate(specs[:9]):                        # the construction itself, on the first chunk of the single-word rows
        q, d = next((q, d) for q, d in enumerate(spec) if d is not None)
        hit = [(((sum(int(rows[i, 3 * e + k]) << (64 * k) for k in range(3)) + C[1 + e]) >> (64 * q)) & _M64) == (d & _M64) for e in range(16)]
        assert sum(hit) >= 12, (spec, hit)
    out = np.zeros((len(rows), 4), np.uint64)
    _lib.call("pil2gl_bn128_linear_hash_rows", pil2gl._ptr(rows), width, len(rows), 16, int(custom), pil2gl._ptr(out))
    bad = [(specs[i], i) for i in range(len(rows))
           if [int(x) for x in out[i]] != orc.to_montgomery_words(orc.linear_hash_worker(rows[i].tolist(), 16, custom))]
    assert not bad, _report(bad, len(rows))
