"""The BN254 Fr sparse products, sums and degree from Node: js/polynomial_bn128.js add, sub, mulScalar, byXSubValue, byXNSubValue,
mulSparse and degree on DevBuffers and staged arrays, zerofierTerms and the overlap refusal's message, against the Python checker's
bytes (tests/bn128_polymul_ref.py).  The test writes a job, Node runs it as a fresh child process and compares bytes."""
import json
import os
import shutil
import subprocess

import pytest

import bn128_polymul_ref as ref
from bn128_polymul_ref import R
from conftest import ROOT

NODE = shutil.which("node")


def hx(vals):
    return ref.words(vals).tobytes().hex()


def m1(v):
    return hx([ref.mont(v)])


@pytest.mark.gpu
@pytest.mark.skipif(NODE is None, reason="node not installed")
def test_js_polynomial_products_match_the_checker(tmp_path):
    n_acc, n_src = 700, 600
    acc, src = ref.rand_elems(n_acc, 1), ref.rand_elems(n_src, 2)
    v = ref.rand_elems(1, 3)[0]
    job = {"acc": hx(acc), "src": hx(src), "nAcc": n_acc, "nSrc": n_src, "value": m1(v),
           "add": hx(ref.fma(acc, src, [(1, 0)], 1)), "sub": hx(ref.fma(acc, src, [(R - 1, 0)], 1)),
           "mulScalar": hx(ref.fma(src, src, [(v, 0)], None)),
           "byXSubValue": hx(ref.fma([0] * (n_src + 1), src, [(R - v, 0), (1, 1)], None)),
           "xn": 300, "byXNSubValue": hx(ref.fma([0] * (n_src + 300), src, [(R - v, 0), (1, 300)], None))}
    # a column of a section: src column 1 of width 3 into column 0 of a section 2 wide
    sec3, sec2 = ref.rand_elems(3 * 50, 4), ref.rand_elems(2 * 51, 5)
    job["strided"] = {"src": hx(sec3), "dst": hx(sec2), "n": 50,
                      "want": hx(ref.fma_column(sec2, 0, 2, 51, sec3, 1, 3, 50, [(R - v, 0), (1, 1)], None))}
    factors = [(1, ref.rand_elems(1, 6)[0]), (2, 77), (4, R - 1), (4, ref.rand_elems(1, 7)[0])]
    terms = ref.zerofier_terms(factors)
    job["zerofier"] = {"factors": [{"k": k, "beta": m1(b)} for k, b in factors],
                       "terms": [{"coef": m1(m), "exp": e} for m, e in terms],
                       "mulSparse": hx(ref.fma([0] * (n_src + terms[-1][1]), src, terms, None)),
                       "cancel": {"factors": [{"k": 1, "beta": m1(1)}, {"k": 1, "beta": m1(R - 1)}],
                                  "terms": [{"coef": m1(R - 1), "exp": 0}, {"coef": m1(1), "exp": 2}]},
                       "tooMany": [{"k": 3 ** j, "beta": m1(j + 2)} for j in range(7)]}           # 2^7 = 128 distinct exponents
    deg = [0] * 500
    deg[0], deg[321] = 5, 1 << 224
    job["degree"] = [{"c": hx(deg), "want": 321}, {"c": hx([0] * 64), "want": -1}, {"c": hx([9] + [0] * 99), "want": 0}]
    path = tmp_path / "job.json"
    path.write_text(json.dumps(job))
    out = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "polymul_bn128_parity.js"), str(path)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "polymul bn128 parity OK" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
