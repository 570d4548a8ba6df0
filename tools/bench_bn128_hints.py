#!/usr/bin/env python3
"""Timing of the BN254 Fr batch inverse, grand product and grand sum (csrc/bn_scan.hip): each operator at n = 2^20 and 2^24, stride 1
and stride 8 (a column of a section 8 elements wide, inputs and output alike).  One warm-up, then the median of five runs timed with
device events, all under one time limit.  Elements are uniform Montgomery words below 2^252 < r, never zero in practice.  Beside each
time, two floors derived without a run:
  issue    products per row x 328 vector instructions (fr_mul in the built ISA) x 4.8 issue cycles per instruction and SIMD
           (profiles/r05_issue_cost_saturated.txt) over 64 lanes x 1024 SIMDs at 2.4 GHz.  Products per row, level 0 only (the levels above
           add at most 1/15): batch_inverse 4 (reduce 1, prefixes 1, the walk back 2), gsum 5 (the numerator), gprod 7 (the numerator,
           and reduce 1 + store 1 of the running product).
  traffic  the bytes the kernels ask of memory against 8 TB/s: batch_inverse 192 per row (x three times, the prefixes written and read,
           y written), gsum 288 (the running sum reads y twice and writes it), gprod 320 (and the numerators).
The single Fermat ladder (about 380 dependent products on one lane of one wave) is timed alone as batch_inverse of one element.
  python tools/bench_bn128_hints.py [--limit SECONDS] [--out FILE] [--small]        one JSON line per case"""
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
PRODUCTS_PER_ROW = {"batch_inverse": 4, "gsum": 5, "gprod": 7}
BYTES_PER_ROW = {"batch_inverse": 192, "gsum": 288, "gprod": 320}


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


def elements(n, seed):
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
    c = elem(0x1234567890ABCDEF1234567890ABCDEF1234567890ABCDEF)
    lines = []
    one = elements(1, 1).reshape(-1)
    one_out = torch.empty_like(one)
    med, lo, hi = timed(lambda: bn128.batch_inverse(one, n=1, out=one_out))
    lines.append(json.dumps({"op": "single-lane inversion (batch_inverse, n = 1)", "ms_median": round(med, 3), "ms_min": round(lo, 3), "ms_max": round(hi, 3),
                             "products": 380, "us_per_dependent_product": round(med * 1e3 / 380, 3)}))
    print(lines[-1], flush=True)
    for n_bits in (20 - sh, 24 - sh):
        n = 1 << n_bits
        for stride in (1, 8):
            num, den = elements(n * stride, n_bits).reshape(-1), elements(n * stride, n_bits + 50).reshape(-1)
            out = torch.zeros(n * stride * 4, dtype=torch.int64, device="cuda")
            for op in ("batch_inverse", "gprod", "gsum"):
                if op == "batch_inverse":
                    fn = lambda: bn128.batch_inverse(den, n=n, stride=stride, out=out, out_stride=stride)      # noqa: E731
                elif op == "gprod":
                    fn = lambda: bn128.gprod(num, den, n=n, num_stride=stride, den_stride=stride, out=out, out_stride=stride)      # noqa: E731
                else:
                    fn = lambda: bn128.gsum(c, den, n=n, den_stride=stride, out=out, out_stride=stride)      # noqa: E731
                med, lo, hi = timed(fn)
                issue_ms = PRODUCTS_PER_ROW[op] * n * VALU_PER_PRODUCT / 64 * ISSUE_CYCLES / SIMDS / 2.4e6
                traffic_ms = BYTES_PER_ROW[op] * n / HBM_BYTES_PER_S * 1e3
                rec = {"op": op, "n": n, "stride": stride, "ms_median": round(med, 3), "ms_min": round(lo, 3), "ms_max": round(hi, 3),
                       "Mrows_per_s": round(n / med / 1e3, 1), "plan": bn128.scan_plan(n, op), "products_per_row": PRODUCTS_PER_ROW[op],
                       "floor_issue_ms_at_2.4GHz": round(issue_ms, 3), "floor_traffic_ms_at_8TBps": round(traffic_ms, 3),
                       "ratio_to_larger_floor": round(med / max(issue_ms, traffic_ms), 2)}
                lines.append(json.dumps(rec))
                print(lines[-1], flush=True)
            del num, den, out
            torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
