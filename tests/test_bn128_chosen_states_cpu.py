"""The chosen-state cases of the BN254 Poseidon tests (tests/bn128_chosen.py) on the CPU: the oracle's round access and inverse, the
pattern table, every built case through the Python oracle and through the C oracle (its first edge-value test: 4 x 64-bit Montgomery
limbs of its own), the placement of the cases on the rows of the device batch, and the integer model of the radix-2^29 S-box columns
on all-ones limbs and on pow5's own chain.  Every comparison is exact equality of field elements."""
import os
import random
import sys

import pytest

from conftest import ROOT

import bn128_chosen as bc
import bn128_oracle as orc

R = orc.R


def _trace(inp, t):
    """the plain permutation, keeping what every site sees: A[r] = the S-box input of round r, B[r] = its output, F = the final state"""
    C, M = orc.poseidon_constants(t)
    A, B, st = [], [], list(inp)
    for r in range(orc.N_ROUNDS_F + orc.N_ROUNDS_P[t - 2]):
        st = [(a + C[t * r + j]) % R for j, a in enumerate(st)]
        A.append(st)
        st = [pow(a, 5, R) if j == 0 or orc.is_full_round(t, r) else a for j, a in enumerate(st)]
        B.append(st)
        st = [sum(M[i][j] * st[j] for j in range(t)) % R for i in range(t)]
    return A, B, st


def test_round_access_and_inverse():
    """poseidon_from_round / poseidon_preimage / poseidon_sbox_input against the forward permutation: t = 2, 5, 17 at the rounds on
    either side of every change of round kind, and every round of t = 3"""
    rng = random.Random(1)
    for t in (2, 3, 5, 17):
        n_rounds = orc.N_ROUNDS_F + orc.N_ROUNDS_P[t - 2]
        Mi, M = orc.matrix_inverse(t), orc.poseidon_constants(t)[1]
        assert all(sum(M[i][k] * Mi[k][j] for k in range(t)) % R == int(i == j) for i in range(t) for j in range(t))
        inp = [rng.randrange(R) for _ in range(t)]
        A, B, F = _trace(inp, t)
        assert F == orc.poseidon(inp[1:], inp[0], t)
        rp = orc.N_ROUNDS_P[t - 2]
        for r in range(n_rounds) if t == 3 else (0, 3, 4, 5, 4 + rp - 1, 4 + rp, n_rounds - 1):
            assert orc.poseidon_from_round(t, r, A[r]) == F and orc.poseidon_preimage(t, r, A[r]) == inp, (t, r)
            assert orc.poseidon_sbox_input(t, r, B[r]) == A[r], (t, r)
        assert orc.poseidon_from_round(t, n_rounds, F) == F and orc.poseidon_preimage(t, n_rounds, F) == inp
        with pytest.raises(ValueError):
            orc.poseidon_from_round(t, n_rounds + 1, F)
        with pytest.raises(ValueError):
            orc.poseidon_sbox_input(t, n_rounds, F)
    assert pow(pow(12345, 5, R), orc.SBOX_INV, R) == 12345


def test_pattern_table():
    assert len(bc.PATTERNS) >= 24 and len({w for _, w in bc.PATTERNS}) == len(bc.PATTERNS)
    ws = dict(bc.PATTERNS)
    assert all(0 <= w < R for w in ws.values())
    dropped = [n for n, w in bc._candidates() if w >= R]
    assert dropped == ["R & ~(2^32-1) | 0xffffffff"]                # R ends in 0xf0000001: the filled low word passes it
    for name in ("0", "R-1", "2^253", "2^232-1", "limbs8 ones, top max", "0x2f 80..80", "R & ~(2^224-1)"):
        assert name in ws
    top = ws["limbs8 ones, top max"]
    assert top & ((1 << 232) - 1) == (1 << 232) - 1 and top < R <= top + (1 << 232)
    assert ws["0x2f 7f..7f"].to_bytes(32, "little") == bytes([0x7F] * 31 + [0x2F])
    assert ws["0x2f 00ff.."].to_bytes(32, "little")[:4] == bytes([0xFF, 0, 0xFF, 0])
    for form, shift in bc.FORM_SHIFT.items():                       # the value's representation is the pattern
        for _, w in bc.PATTERNS:
            v = bc.value_of(form, w)
            assert 0 <= v < R and v * (1 << shift) % R == w == bc.representation(form, v)
    assert orc.to_montgomery_words(bc.value_of("mont", ws["2^64-1"])) == [0xFFFFFFFFFFFFFFFF, 0, 0, 0]


def test_plan_coverage_and_row_placement():
    """plan() asserts the coverage rules itself; here the counts, the round classes and where the cases land in the device batch"""
    plan = bc.plan()
    assert sum(len(cs) for cs in plan.values()) <= bc.MAX_CASES
    for t in bc.WIDTHS:
        rp = orc.N_ROUNDS_P[t - 2]
        rounds = bc.rounds_of(t)
        assert {0, 1, 3, 4, 5, 6, 7, 4 + rp - 1, 4 + rp, 8 + rp - 1} <= set(rounds)
        assert {4 + rp - 1 - k for k in range(rp % 4 + 1)} <= set(rounds)          # the leftover rounds and the end of the last whole block
        got = {c.cls for c in plan[t]}
        assert got == set(bc.classes_of(t)) and ("F", 8 + rp) in got
        for c in plan[t]:
            if c.site != "F" and not orc.is_full_round(t, c.r):
                assert list(c.chosen) == [0], c
        rows = bc.pipeline_rows(t)
        assert len(rows) == bc.PIPELINE_ROWS > 2048 and set(rows) == set(range(len(plan[t])))
        for cls in bc.classes_of(t):
            first = next(i for i, c in enumerate(plan[t]) if c.cls == cls)
            assert {k % 64 for k, i in enumerate(rows) if i == first} >= set(bc.EDGE_LANES), (t, cls)
        assert plan[t][rows[-1]].kind in ("all", "hot") and rows[-1] == min(i for i, c in enumerate(plan[t]) if c.cls == plan[t][rows[-1]].cls)
    assert [t for t in bc.WIDTHS if orc.N_ROUNDS_P[t - 2] % 4] == [3, 7, 9, 11, 13, 14]           # the widths with leftover partial rounds


@pytest.mark.parametrize("t", bc.WIDTHS)
def test_cases_python_oracle(t):
    """preimage then poseidon gives the from_round output, and the forward run passes through the chosen state: at the case's site the
    chosen elements, in the case's form, are the patterns"""
    ws = dict(bc.PATTERNS)
    for c in bc.cases(t):
        assert len(c.inp) == t and all(0 <= v < R for v in c.inp + c.want)
        A, B, F = _trace(c.inp, t)
        assert F == c.want, c                       # (Case.build asserted bn128_oracle.poseidon(inp) == want)
        at = F if c.site == "F" else (A if c.site == "A" else B)[c.r]
        assert c.chosen and all(bc.representation(c.form, at[j]) == ws[name] for j, name in c.chosen.items()), c
        if c.kind == "equal":
            assert len(set(at)) == 1 and orc.to_montgomery_words(at[0]) in ([0] * 4, orc.to_montgomery_words(bc.value_of("mont", R - 1)))


@pytest.mark.parametrize("t", bc.WIDTHS)
def test_cases_c_oracle(t):
    for c in bc.cases(t):
        assert orc.c_poseidon(c.inp[1:], c.inp[0], t) == c.want, c
        assert orc.c_poseidon(c.inp[1:], c.inp[0], 1) == c.want[:1], c


def test_bn29_column_model_edges_and_pow5_chain():
    """csrc/gen_bn29_columns.py: the reduction digit in the form that ships equals -lo / r mod 2^29 (asserted inside the model), the
    products on every pair of edge operands -- the eight low limbs all ones under the largest top limb the precondition (operands
    below 0.9 * 2^256) admits among them --, pow5's chain with the unmasked top limb and the doubled operand feeding the next
    squaring: every column sum below 2^64, results a b / 2^261 and x^5 / 2^1044 mod r.  The patterns of the chosen-state cases
    and their lazy representatives W + r go through the S-box model as well."""
    sys.path.insert(0, os.path.join(ROOT, "pil2-stark-js_amd", "csrc"))
    import gen_bn29_columns as g
    assert g.LIM == int(0.9 * 2 ** 256) and g.ALL_ONES < g.LIM and g.limbs(g.ALL_ONES)[:8] == [g.MASK] * 8
    assert g.ALL_ONES in g.edge_operands()
    g.check_products()
    g.check_pow5()
    inv = pow(1 << 1044, -1, R)
    for _, w in bc.PATTERNS:
        for x in (w, w + R, w + 2 * R):
            assert x < g.LIM
            got = g.model_pow5(x)
            assert got % R == pow(w, 5, R) * inv % R and got < 2 ** 252 + R
    with pytest.raises(AssertionError):                              # the 64-bit bound is live: nine limbs of 2^32 - 1 pass it
        g.model_limbs([0xFFFFFFFF] * 9, [0xFFFFFFFF] * 9, False)
