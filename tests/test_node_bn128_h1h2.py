"""The BN254 Fr plookup hint from Node: js/polutils_bn128.js calculateH1H2 on arrays of Uint8Array(32) and calculateH1H2Dev on resident
DevBuffer columns, against the Python checker's bytes (tests/bn128_h1h2_ref.py), and the reference's full message -- row and decimal
value -- for a value t lacks.  The test writes a job, Node runs it as a fresh child process and compares bytes."""
import json
import os
import shutil
import subprocess

import pytest

import bn128_h1h2_ref as ref
import bn128_hints_ref as href
from conftest import ROOT

NODE = shutil.which("node")


def hx(vals):
    return href.mont_words(vals).tobytes().hex()


def case(n, distinct, seed):
    """plain values: a duplicate-heavy t of `distinct` values, f drawn from it"""
    pool = href.rand_elems(distinct, seed)
    t = [pool[(i * i + seed) % distinct] for i in range(n)]
    f = [t[(7 * j + 3) % n] for j in range(n)]
    return f, t


@pytest.mark.gpu
@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_js_h1h2_matches_the_checker(tmp_path):
    job = {"arrays": []}
    for n, distinct in ((3, 2), (9, 4), (2500, 700)):
        f, t = case(n, distinct, n)
        assert len(set(t)) < n                                    # duplicates in t
        h1, h2 = ref.h1h2(f, t)
        job["arrays"].append({"n": n, "f": hx(f), "t": hx(t), "h1": hx(h1), "h2": hx(h2)})
    f, t = case(50, 20, 5)
    absent = next(v for v in href.rand_elems(30, 77) if v not in t)
    f[31] = f[44] = absent
    job["missing"] = {"f": hx(f), "t": hx(t), "message": "Number not included: w:31, value:%d" % absent}

    n, width, dst_width = 1500, 3, 4
    f, t = case(n, 400, 8)
    h1, h2 = ref.h1h2(f, t)
    section = href.rand_elems(n * width, 9)
    section[2::width], section[0::width] = f, t
    dst = href.rand_elems(n * dst_width, 10)
    want_dst = list(dst)
    want_dst[1::dst_width], want_dst[3::dst_width] = h1, h2
    bad = list(section)
    bad[2 + 1499 * width] = bad[2 + 600 * width] = absent          # rows 600 and 1499 of f
    assert absent not in t
    job["resident"] = {"n": n, "width": width, "fCol": 2, "tCol": 0, "dstWidth": dst_width, "h1Col": 1, "h2Col": 3,
                       "section": hx(section), "dst": hx(dst), "wantDst": hx(want_dst), "badSection": hx(bad),
                       "message": "Number not included: w:600, value:%d" % absent}
    path = tmp_path / "job.json"
    path.write_text(json.dumps(job))
    out = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "h1h2_bn128_parity.js"), str(path)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "h1h2 bn128 parity OK" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
