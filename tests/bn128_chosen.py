"""Chosen mid-round states of the BN254 Poseidon permutation (a plain module: tests/test_bn128_chosen_states_cpu.py and
tests/test_gpu_bn128_chosen_states.py build their cases here).

After the first round every state of the permutation is pseudorandom, so random inputs never make an S-box input, an operand of
the linear layer or a final value equal to 0, R - 1, a power of two, an all-ones limb pattern or a 0x7f / 0x80 byte pattern.
The permutation is invertible round by round (oracle/bn128_oracle.py: poseidon_preimage), so a case picks the state it wants at
one round, runs the oracle backwards to the input that produces it and forwards to the output it must give.

A case is (t, site, round, form, kind, {element: pattern}):
  site  A = the S-box input of round r, B = the S-box output of round r (the operand of the linear layer), F = the final state;
  form  which representation of the value carries the pattern W (the device holds Montgomery words, not the value):
        plain: value = W;  mont: value * 2^256 = W;  sboxed (site B): value * 2^236 = W, what bn29::pow5 leaves;
  kind  all = every element its own pattern (full rounds and F), hot = one element a pattern and the rest seeded random (the one
        chosen element of a partial round is element 0: the device holds its own linear image of the others there, only
        element 0's S-box input and output are values of the permutation whatever the formulation), equal = every element the
        same value.
Patterns at or above R are dropped, never reduced.

Rounds, per t (rp = N_ROUNDS_P[t - 2]): 0, 1, 3; 4 (the first partial round), 5, 6, 7; the last round of the last whole block of
four partial rounds; every one of the rp % 4 leftover rounds; 4 + rp - 1, 4 + rp, the last round; the final site.

Coverage (asserted by plan()): per t every (site, round) has at least two forms and two patterns; over all t every pattern
occurs at every site in every applicable form.  Two families on top: all elements 0 and all elements R - 1 as Montgomery words
at A of round 0, at F and at A of the first closing full round; and the hot element of the full-round `hot` cases walks 0, 1,
9, 10 (the LDS / private-memory boundary of the device state, BN_LDS_ELEMS) and t - 1.

The count: a partial round has one chosen element, so two forms there are two cases; one form per case makes that two cases in
a full round as well.  The rounds above are 172 over t = 2..17 (92 partial, 80 full), at sites A and B, plus 16 F: 360 classes,
720 cases at the least, plus 96 of the `equal` family: 816.  That is more than the 600 first estimated for this set; the round
classes, the patterns and the two-forms rule were kept and the count left where they put it (MAX_CASES), the cost being host
time alone (the device runs the same 2112-row batch whatever the count; LAB_NOTES.md section 20 has the measured build time).
"""
import random

import bn128_oracle as orc

R = orc.R
WIDTHS = tuple(range(2, 18))
FORM_SHIFT = {"plain": 0, "mont": 256, "sboxed": 236}
SITE_FORMS = {"A": ("plain", "mont"), "B": ("plain", "mont", "sboxed"), "F": ("plain", "mont")}
HOT_INDICES = (0, 1, 9, 10)                  # and t - 1
MAX_CASES = 816
PIPELINE_ROWS = 2112                         # 33 waves of 64 lanes: above the 2048 at which a batch gets a lane per permutation
EDGE_LANES = (0, 31, 32, 63)


def _bytes_under_2f(b):
    return (0x2F << 248) | int.from_bytes(bytes([b]) * 31, "little")


def _candidates():
    ones232 = (1 << 232) - 1
    c = [("0", 0), ("1", 1), ("2", 2), ("R-1", R - 1), ("R-2", R - 2), ("(R-1)/2", (R - 1) // 2), ("(R+1)/2", (R + 1) // 2)]
    c += [("2^%d" % k, 1 << k) for k in (28, 29, 31, 32, 58, 63, 64, 224, 252, 253)]
    c += [("2^%d-1" % k, (1 << k) - 1) for k in (29, 32, 58, 64, 232, 253)]
    top = (R - ones232 - 1) >> 232           # the largest top limb that keeps W < R under eight all-ones limbs
    c += [("limbs8 ones, top 0", ones232), ("limbs8 ones, top max", (top << 232) | ones232)]
    c += [("0x2f 7f..7f", _bytes_under_2f(0x7F)), ("0x2f 80..80", _bytes_under_2f(0x80)), ("0x2f ff..ff", _bytes_under_2f(0xFF))]
    c += [("0x2f 00ff..", (0x2F << 248) | int.from_bytes(bytes([0xFF, 0x00] * 15 + [0xFF]), "little")),
          ("0x2f ff00..", (0x2F << 248) | int.from_bytes(bytes([0x00, 0xFF] * 15 + [0x00]), "little"))]
    c += [("R & ~(2^224-1)", R >> 224 << 224), ("R & ~(2^32-1)", R >> 32 << 32), ("R & ~(2^32-1) | 0xffffffff", (R >> 32 << 32) | 0xFFFFFFFF)]
    return c


def pattern_table():
    """[(name, W)]: the candidates below R, a value kept once (2^232 - 1 is also the eight all-ones limbs under a zero top limb)"""
    seen, out = set(), []
    for name, w in _candidates():
        if w < R and w not in seen:
            seen.add(w)
            out.append((name, w))
    assert len(out) >= 24
    return out


PATTERNS = pattern_table()
_W = dict(PATTERNS)


def value_of(form, w):
    """the field value whose `form` representation is the pattern w"""
    return w * pow(1 << FORM_SHIFT[form], -1, R) % R


def representation(form, value):
    return value * (1 << FORM_SHIFT[form]) % R


def rounds_of(t):
    rp = orc.N_ROUNDS_P[t - 2]
    whole = 4 + 4 * (rp // 4)
    rs = {0, 1, 3, 4, 5, 6, 7, whole - 1, 4 + rp - 1, 4 + rp, orc.N_ROUNDS_F + rp - 1}
    rs |= {whole + k for k in range(rp % 4)}
    return sorted(rs)


def classes_of(t):
    """the (site, round) classes of width t; the final site carries round RF + rp"""
    return [(s, r) for r in rounds_of(t) for s in ("A", "B")] + [("F", orc.N_ROUNDS_F + orc.N_ROUNDS_P[t - 2])]


class Case:
    __slots__ = ("t", "site", "r", "form", "kind", "chosen", "seed", "u", "inp", "want")

    def __init__(self, t, site, r, form, kind, chosen, seed):
        self.t, self.site, self.r, self.form, self.kind, self.chosen, self.seed = t, site, r, form, kind, chosen, seed
        self.u = self.inp = self.want = None

    @property
    def cls(self):
        return (self.site, self.r)

    def __repr__(self):
        return "Case(t=%d, site=%s, round=%d, form=%s, kind=%s, %s)" % (self.t, self.site, self.r, self.form, self.kind, self.chosen)

    def site_values(self):
        """the t values at the site: the chosen elements from their patterns, the others seeded random"""
        rng = random.Random(self.seed)
        vals = [rng.randrange(R) for _ in range(self.t)]
        for j, name in self.chosen.items():
            vals[j] = value_of(self.form, _W[name])
        return vals

    def build(self):
        vals = self.site_values()
        self.u = orc.poseidon_sbox_input(self.t, self.r, vals) if self.site == "B" else vals
        self.inp = orc.poseidon_preimage(self.t, self.r, self.u)
        self.want = orc.poseidon_from_round(self.t, self.r, self.u)
        assert orc.poseidon(self.inp[1:], self.inp[0], self.t) == self.want, self
        return self


_PLAN = None


def plan():
    """{t: [Case, not built]}: cheap (no field arithmetic), for all widths at once so that the patterns rotate over all of them:
    a slot (site, form) takes the patterns it has used least so far"""
    global _PLAN
    if _PLAN is not None:
        return _PLAN
    use = {(s, f, n): 0 for s, fs in SITE_FORMS.items() for f in fs for n, _ in PATTERNS}
    form_use = {(s, f): 0 for s, fs in SITE_FORMS.items() for f in fs}
    order = {n: i for i, (n, _) in enumerate(PATTERNS)}

    def pick(site, form, k, exclude=()):
        names = sorted((n for n, _ in PATTERNS if n not in exclude), key=lambda n: (use[site, form, n], order[n]))[:k]
        for n in names:
            use[site, form, n] += 1
        return names

    def two_forms(site):
        fs = sorted(SITE_FORMS[site], key=lambda f: (form_use[site, f], SITE_FORMS[site].index(f)))[:2]
        form_use[site, fs[0]] += 3             # the first form gets the case with the most patterns: weigh it, so that the forms take turns at it
        form_use[site, fs[1]] += 1
        return fs

    out = {}
    for t in WIDTHS:
        rp = orc.N_ROUNDS_P[t - 2]
        hots = sorted({j for j in HOT_INDICES + (t - 1,) if j < t})
        cases, n_hot = [], 0

        def add(site, r, form, kind, chosen):
            cases.append(Case(t, site, r, form, kind, chosen, 1000 * t + len(cases)))
        for site, r in classes_of(t):
            f1, f2 = two_forms(site)
            if site == "F" or orc.is_full_round(t, r):
                first = pick(site, f1, t)
                add(site, r, f1, "all", dict(enumerate(first)))
                add(site, r, f2, "hot", {hots[n_hot % len(hots)]: pick(site, f2, 1, first[:1])[0]})
                n_hot += 1
            else:
                first = pick(site, f1, 1)
                add(site, r, f1, "hot", {0: first[0]})
                add(site, r, f2, "hot", {0: pick(site, f2, 1, first)[0]})
        for site, r in (("A", 0), ("F", orc.N_ROUNDS_F + rp), ("A", 4 + rp)):
            for name in ("0", "R-1"):
                add(site, r, "mont", "equal", {j: name for j in range(t)})
        # per t: every class with two forms and two patterns, every hot index taken
        for c in classes_of(t):
            mine = [x for x in cases if x.cls == c]
            assert len({x.form for x in mine}) >= 2 and len({n for x in mine for n in x.chosen.values()}) >= 2, (t, c)
        assert {j for x in cases if x.kind == "hot" and (x.site == "F" or orc.is_full_round(t, x.r)) for j in x.chosen} == set(hots), t
        out[t] = cases
    for key in use:                            # over all t: every pattern at every site in every applicable form
        assert any(x.site == key[0] and x.form == key[1] and key[2] in x.chosen.values() for cs in out.values() for x in cs), key
    assert sum(len(cs) for cs in out.values()) <= MAX_CASES
    _PLAN = out
    return out


_BUILT = {}


def cases(t):
    """the built cases of width t (inp, want set and checked against bn128_oracle.poseidon), cached"""
    if t not in _BUILT:
        _BUILT[t] = [c.build() for c in plan()[t]]
    return _BUILT[t]


def pipeline_rows(t, n_rows=PIPELINE_ROWS):
    """case index per row of the lane-per-permutation batch: the cases of t cycled, then the first case of class k placed on lanes 0
    and 32 of wave k and on lanes 31 and 63 of wave k + 1 (the four lanes where the halves of a wave meet and end), and the first case
    of one class, another for each t, on the last row.  Neighbouring rows hold different cases."""
    cs = plan()[t]
    first = {}
    for i, c in enumerate(cs):
        first.setdefault(c.cls, i)
    firsts = [first[c] for c in classes_of(t)]
    assert 64 * (len(firsts) + 1) < n_rows - 64
    rows = [i % len(cs) for i in range(n_rows)]
    placed = {}
    for k, i in enumerate(firsts):
        for row in (64 * k, 64 * k + 32, 64 * (k + 1) + 31, 64 * (k + 1) + 63):
            placed[row] = i
    placed[n_rows - 1] = firsts[t % len(firsts)]
    for row, i in placed.items():
        rows[row] = i
    for k in range(n_rows):                    # a placed row may have met its own case in the cycle beside it: move the neighbour on
        if k not in placed and rows[k] in (rows[k - 1] if k else None, rows[k + 1] if k + 1 < n_rows else None):
            rows[k] = next(i for i in range(len(cs)) if i != rows[k - 1] and i != rows[(k + 1) % n_rows])
    assert all(rows[k] != rows[k - 1] for k in range(1, n_rows)) and all(rows[k] == i for k, i in placed.items())
    return rows
