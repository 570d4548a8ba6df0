"""The checker of the BN254 Fr batch inverse, grand product and grand sum (a plain module: tests/test_bn128_hints_cpu.py,
tests/test_gpu_bn128_hints.py and the Node test's expectations build on it), in Python integers from the definitions

    inv[i]  = src[i]^-1                                   (0 -> 0)
    z[0]    = 1,  z[i] = z[i-1] num[i-1] / den[i-1]       (a zero denominator: that ratio is 0)
    s[i]    = s[i-1] + num / den[i]                       (a zero denominator adds 0; num is one element)

on PLAIN integers mod r.  The device works on Montgomery words a 2^256 mod r: the tests convert with mont / unmont, which are bijections
(inv, products and sums are not linear in that factor, so unlike the polynomial checker nothing runs on the word integers themselves).
Inverses come from the batch trick, one pow() per call, so that 2^20 rows take about a second."""
import numpy as np

from bn128_poly_ref import R, MONT, MONT_INV, mont, words, ints, rand_elems, limb_pattern_elems  # noqa: F401  (re-exported)


def unmont(v):
    return v * MONT_INV % R


def batch_inverse(src):
    """[x^-1 mod r, 0 for 0]"""
    pre, acc = [], 1
    for x in src:
        pre.append(acc)
        if x:
            acc = acc * x % R
    inv = pow(acc, -1, R)
    out = [0] * len(src)
    for i in range(len(src) - 1, -1, -1):
        x = src[i]
        if x:
            out[i] = inv * pre[i] % R
            inv = inv * x % R
    return out


def gprod(num, den):
    assert len(num) == len(den)
    z, acc = [], 1
    for n_, i_ in zip(num, batch_inverse(den)):
        z.append(acc)
        acc = acc * n_ % R * i_ % R
    return z


def gsum(num, den):
    s, acc = [], 0
    for i_ in batch_inverse(den):
        acc = (acc + num * i_) % R
        s.append(acc)
    return s


def mont_words(vals):
    """plain integers -> (n, 4) uint64 Montgomery words"""
    return words([v * MONT % R for v in vals])


def plain(w):
    """Montgomery words -> plain integers"""
    return [v * MONT_INV % R for v in ints(w)]
