#!/usr/bin/env python3
"""Timing of the BN254 Fr sparse products, scaled sums and degree (csrc/bn_polymul.hip): poly_fma over 2^20 and 2^24 source
coefficients at t = 1 (add: coefficient 1, scale 1 -- no product), t = 2 (byXSubValue: one product) and t = 16 general coefficients
with a general scale, and poly_degree over 2^24 coefficients of which only the lowest is not zero (its worst case).  One warm-up, then
the median of five runs timed with device events (poly_degree blocks for its readback, so its time includes it), all under one time
limit.  Coefficients are uniform Montgomery words below 2^252 < r.  Beside each time, the two floors of DESIGN.md section 14, derived without a run:
  issue    non-trivial products x 328 vector instructions (fr_mul in the built ISA) x 4.8 issue cycles per instruction and SIMD
           (profiles/r05_issue_cost_saturated.txt) over 64 lanes x 1024 SIMDs at 2.4 GHz.  Products per output element: the terms
           whose coefficient is neither 1 nor r - 1, and one more for a scale that is neither absent nor 1.
  traffic  the bytes the kernel asks for against 8 TB/s: per output element 32 written, 32 read when there is a scale, 32 per term (the
           overlapping loads of neighbouring lanes are counted as asked, not as served from cache); the degree reads 32 n
           in that case.
  python tools/bench_bn128_polymul.py [--limit SECONDS] [--out FILE] [--small]        one JSON line per case"""
import argparse
import json
import os
import signal
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "pil2-stark-js_amd", "python"))
import numpy as np
import torch
import pil2gl
from pil2gl import bn128

SIMDS = 256 * 4
VALU_PER_PRODUCT = 328      # fr_mul in the gfx950 ISA hipcc builds
ISSUE_CYCLES = 4.8          # per vector instruction per SIMD (profiles/r05_issue_cost_saturated.txt)
HBM_BYTES_PER_S = 8e12
R = 21888242871839275222246405745257275088548364400416034343698204186575808495617


def elem(v):
    v = v * (1 << 256) % R
    return np.array([[(v >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(4)]], dtype=np.uint64)


def timed(fn, runs=5):
    fn(); torch.cuda.synchronize()
    ms = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def coefficients(n, seed):
    g = torch.Generator(device="cuda"); g.manual_seed(seed)
    c = torch.randint(0, 1 << 62, (n, 4), dtype=torch.int64, device="cuda", generator=g)
    c[:, 3] >>= 2                                       # below 2^252 < r: canonical Montgomery words
    return c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--limit", type=int, default=240)
    ap.add_argument("--out")
    ap.add_argument("--small", action="store_true", help="sizes 2^10 times smaller: a rehearsal of the tool, not a measurement")
    a = ap.parse_args()
    signal.alarm(a.limit)
    assert torch.cuda.is_available(), "this is a measurement: it needs the GPU"
    pil2gl.init(0)
    sh = 10 if a.small else 0
    general = 0x1234567890ABCDEF1234567890ABCDEF1234567890ABCDEF
    # (name, terms as (plain coefficient, exponent), scale as a plain integer or None)
    shapes = [("add", [(1, 0)], 1), ("byXSubValue", [(R - general, 0), (1, 1)], None),
              ("t16", [(general + 3 * j, 5 * j) for j in range(16)], general + 1)]
    lines = []

    def report(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    for n_bits in (20 - sh, 24 - sh):
        n_src = 1 << n_bits
        src = coefficients(n_src, n_bits)
        for name, terms, scale in shapes:
            n_acc = n_src + terms[-1][1]
            acc = coefficients(n_acc, n_bits + 50)
            m = np.concatenate([elem(c) for c, _ in terms])
            e = np.array([x for _, x in terms], np.uint64)
            s = None if scale is None else elem(scale)
            med, lo, hi = timed(lambda: bn128.poly_fma(acc, src, m, e, s, n_acc=n_acc, n_src=n_src))
            per_elem = sum(1 for c, _ in terms if c not in (1, R - 1)) + (1 if scale not in (None, 1) else 0)
            products = per_elem * n_acc
            traffic = (32 + (32 if scale is not None else 0) + 32 * len(terms)) * n_acc
            issue_ms = products * VALU_PER_PRODUCT / 64 * ISSUE_CYCLES / SIMDS / 2.4e6
            traffic_ms = traffic / HBM_BYTES_PER_S * 1e3
            report({"op": "poly_fma", "case": name, "nSrc": n_src, "nAcc": n_acc, "t": len(terms), "scale": "none" if scale is None else "one" if scale == 1 else "general",
                    "ms_median": round(med, 3), "ms_min": round(lo, 3), "ms_max": round(hi, 3), "Melems_per_s": round(n_acc / med / 1e3, 1),
                    "products": products, "floor_issue_ms_at_2.4GHz": round(issue_ms, 3), "floor_traffic_ms_at_8TBps": round(traffic_ms, 3),
                    "ratio_to_larger_floor": round(med / max(issue_ms, traffic_ms), 2)})
            del acc
        del src
        torch.cuda.empty_cache()
    n = 1 << (24 - sh)
    c = coefficients(n, 99)
    c[1:] = 0                                           # the degree is 0: the search runs from the top, so every element is read
    deg = []
    med, lo, hi = timed(lambda: deg.append(bn128.poly_degree(c, n)))
    assert set(deg) == {0}, deg
    traffic_ms = 32 * n / HBM_BYTES_PER_S * 1e3
    report({"op": "poly_degree", "n": n, "ms_median": round(med, 3), "ms_min": round(lo, 3), "ms_max": round(hi, 3), "Melems_per_s": round(n / med / 1e3, 1),
            "products": 0, "floor_issue_ms_at_2.4GHz": 0.0, "floor_traffic_ms_at_8TBps": round(traffic_ms, 3), "ratio_to_larger_floor": round(med / traffic_ms, 2)})
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
