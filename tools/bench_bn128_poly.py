#!/usr/bin/env python3
"""Timing of the BN254 Fr polynomial division by x^k - beta and evaluation (csrc/bn_poly.hip): divZh at n = 2^22, k = 2^20 and at
n = 2^26, k = 2^24; division at k = 1 and k = 4 over 2^24 coefficients; evaluation of 2^24 coefficients at 1 and at 8 points.  One
warm-up, then the median of five runs timed with device events, all under one time limit.  Coefficients are uniform Montgomery words
below 2^252 < r, in place on the device.  Beside each time, two floors derived without a run:
  issue    products x 328 vector instructions (fr_mul in the built ISA) x 4.8 issue cycles per instruction and SIMD
           (profiles/r05_issue_cost_saturated.txt) over 64 lanes x 1024 SIMDs.  Products: n - k in the lane-per-chain form (every link but
           a chain's top one); 2 n in the segmented form (reduce and store; the carry levels add less than 1/8); P n for P points.
  traffic  the bytes the kernels ask of memory against 8 TB/s: 64 n (read, write) lane per chain, 96 n (c twice, d once) segmented,
           32 n P for an evaluation (each point's workgroups read the coefficients themselves).
  python tools/bench_bn128_poly.py [--limit SECONDS] [--out FILE] [--small]        one JSON line per case"""
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
    z = elem(0x1234567890ABCDEF1234567890ABCDEF1234567890ABCDEF)
    pts8 = np.concatenate([elem(3 + 7 * i) for i in range(8)])
    cases = [("divZh", 22 - sh, 1 << (20 - sh), 1), ("divZh", 26 - sh, 1 << (24 - sh), 1), ("div", 24 - sh, 1, None), ("div", 24 - sh, 4, None),
             ("eval", 24 - sh, 1, 1), ("eval", 24 - sh, 1, 8)]
    lines = []
    for op, n_bits, k, arg in cases:
        n = 1 << n_bits
        c = coefficients(n, n_bits + k % 97)
        p = bn128.poly_plan(n, k)
        if op == "eval":
            pts = z if arg == 1 else pts8
            med, lo, hi = timed(lambda: bn128.poly_eval(c, pts, n=n))
            products, traffic = arg * n, 32 * n * arg
        else:
            beta = elem(1) if op == "divZh" else z
            med, lo, hi = timed(lambda: bn128.poly_div(c, k, beta, out=c))      # in place: each run divides what the last one left
            products, traffic = (n - k, 64 * n) if p["form"] == 0 else (2 * n, 96 * n)
        issue_cycles = products * VALU_PER_PRODUCT / 64 * ISSUE_CYCLES / SIMDS
        rec = {"op": op, "n": n, "k": k, "points": arg if op == "eval" else None, "ms_median": round(med, 3), "ms_min": round(lo, 3), "ms_max": round(hi, 3),
               "Melems_per_s": round(n / med / 1e3, 1), "plan": p, "products": products,
               "floor_issue_ms_at_2.4GHz": round(issue_cycles / 2.4e6, 3), "floor_traffic_ms_at_8TBps": round(traffic / HBM_BYTES_PER_S * 1e3, 3)}
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
        del c
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
