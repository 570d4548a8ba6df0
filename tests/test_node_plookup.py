"""The plookup argument from Node: js/pil_checks.js plookupFold / plookupProduct (host matrices as words and as bytes) and their Dev forms
(DevBuffer sections), and the spellings calculateH1H2Plookup[Dev] / calculateZPlookup[Dev] of js/polutils.js and js/polutils_bn128.js, one
Goldilocks and one Fr case on a case file written here: a lookup that holds, laid out in one strided matrix; every word of the matrix after
the product and after the fold, h1 and h2 word for word, from the checker (tests/plookup_ref.py), and the h1h2 error for a value of f that
t lacks.  Node runs as a fresh child process."""
import json
import os
import random
import shutil
import subprocess

import numpy as np
import pytest

import plookup_ref as pref
import logup_sum_ref as lref
import bn128_hints_ref as bref
import conn_pols_ref as cref
from hints_ref import P
from conftest import ROOT

NODE = shutil.which("node")
R, MONT = bref.R, bref.MONT


def words(field, rows):
    if field == "gl":
        return np.array(rows, np.uint64).reshape(len(rows), -1)
    return cref.fr_words([v for row in rows for v in row]).reshape(len(rows), -1, 4)


def pat_of(field, v):
    return v % P if field == "gl" else v % R * MONT % R


def ext_words(field, vals):
    if field == "gl":
        return np.array(vals, np.uint64).reshape(len(vals), 3)
    return cref.fr_words([v * MONT % R for v in vals])


def chal_hex(field, v):
    """an extension element's VALUE as the words the call takes"""
    return np.array(v, np.uint64).tobytes().hex() if field == "gl" else cref.fr_words([v % R * MONT % R]).tobytes().hex()


def case(field, n, k_f, k_t, sel_f, sel_t, seed):
    """columns of the one matrix: a spare one, f (falling order), selF, t, selT, h1, h2, z, a spare one"""
    rng = random.Random(seed)
    F = lref.FIELDS[field]
    q = F.q
    hw, zw = (3, 3) if field == "gl" else (1, 1)
    ch = lambda: tuple(rng.randrange(P) for _ in range(3)) if field == "gl" else rng.randrange(R)      # noqa: E731
    alpha, beta, gamma, delta = ch(), ch(), ch(), ch()
    f, t, h1, h2, _, _ = pref.valid_lookup(rng, field, n, k_f, k_t, sel_f, sel_t, alpha=alpha, beta=beta)
    f_cols = list(range(1, 1 + k_f))[::-1]
    c_sel_f = 1 + k_f
    t_cols = list(range(c_sel_f + 1, c_sel_f + 1 + k_t))
    c_sel_t = t_cols[-1] + 1
    c_h1, c_h2 = c_sel_t + 1, c_sel_t + 1 + hw
    c_z = c_h2 + hw
    stride = c_z + zw + 1
    top = (1 << 64) if field == "gl" else (1 << 256)
    rows = []
    for i in range(n):
        row = [rng.randrange(q) for _ in range(stride)]
        for j, c in enumerate(f_cols):
            row[c] = pat_of(field, f[0][i][j]) + (q if i % 3 == 0 and 2 * q < top else 0)     # words past p now and then
        for j, c in enumerate(t_cols):
            row[c] = pat_of(field, t[0][i][j])
        row[c_sel_f] = pat_of(field, f[1][i]) if sel_f else rng.randrange(q)
        row[c_sel_t] = pat_of(field, t[1][i]) if sel_t else rng.randrange(q)
        for col, h in ((c_h1, h1), (c_h2, h2)):
            if field == "gl":
                row[col:col + 3] = list(h[i])
            else:
                row[col] = h[i] * MONT % R
        rows.append(row)
    host = words(field, rows)
    z = pref.plookup_z(field, f, t, h1, h2, alpha, beta, gamma, delta)
    assert pref.closing(field, f, t, h1, h2, alpha, beta, gamma, delta) == F.one
    after_prod = host.copy()
    after_prod[:, c_z:c_z + zw] = ext_words(field, z).reshape((n, zw) + host.shape[2:])
    Fx, T = pref.fold(field, f, t, alpha, beta)
    after_fold = host.copy()
    after_fold[:, c_h1:c_h1 + hw] = ext_words(field, Fx).reshape((n, hw) + host.shape[2:])
    after_fold[:, c_h2:c_h2 + hw] = ext_words(field, T).reshape((n, hw) + host.shape[2:])
    bad_row = 5
    bad = [list(r) for r in rows]
    bad[bad_row][c_sel_f] = pat_of(field, 1)
    bad[bad_row][f_cols[-1]] = pat_of(field, max(r[-1] for r in t[0]) + 1)
    plan = pref.plan(n, field)[0]
    return {"name": "%s plookup, kF = %d, kT = %d" % (field, k_f, k_t), "field": field, "n": n, "stride": stride, "hDim": 3 if field == "gl" else 1,
            "mat": host.tobytes().hex(), "f": {"cols": f_cols, "sel": c_sel_f if sel_f else None}, "t": {"cols": t_cols, "sel": c_sel_t if sel_t else None},
            "h1": c_h1, "h2": c_h2, "z": c_z, "alpha": chal_hex(field, alpha), "beta": chal_hex(field, beta), "gamma": chal_hex(field, gamma),
            "delta": chal_hex(field, delta), "afterProd": after_prod.tobytes().hex(), "afterFold": after_fold.tobytes().hex(),
            "h1Words": ext_words(field, h1).tobytes().hex(), "h2Words": ext_words(field, h2).tobytes().hex(), "badMat": words(field, bad).tobytes().hex(),
            "badRow": bad_row, "plan": [plan[3], plan[5]]}


@pytest.mark.gpu
@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_js_plookup_matches_the_checker(tmp_path):
    cases = [case("gl", 100, 3, 3, True, True, 51), case("bn128", 80, 2, 5, True, False, 53)]
    jpath = tmp_path / "job.json"
    jpath.write_text(json.dumps({"cases": cases}))
    out = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "plookup_parity.js"), str(jpath)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "plookup parity OK" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
