#!/usr/bin/env python3
"""Timing of the BN254 G1 multi-scalar multiplication (csrc/bn_msm.hip) at n = 2^16, 2^20, 2^24: one warm-up, then the median of five runs
timed with device events, all under one time limit.  Bases are 64 multiples of the generator (made on the host by the tests' checker) tiled
over the array, so the gathers of the bucket phase hit cache: the time is that of the arithmetic, not of a real pTau's traffic.  Scalars are
uniform Montgomery words below r, distinct per point.  Beside each time: points per second, the plan, and the floor derived without a run
from the built ISA: mixed additions (n per window) x vector instructions per mixed addition x issue cycles per instruction over the
chip's SIMDs.
  python tools/bench_bn128_msm.py [--limit SECONDS] [--out FILE] [--small]        one JSON line per case"""
import argparse
import ctypes as C
import json
import os
import signal
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "pil2-stark-js_amd", "python"))
sys.path.insert(0, os.path.join(HERE, "..", "tests"))
import numpy as np
import torch
import pil2gl
from pil2gl import bn128
from pil2gl._lib import check, load
import bn128_g1_ref as ref

SIMDS = 256 * 4
# vector instructions of one mixed addition (8M + 2S, its additions and subtractions) in the gfx950 ISA hipcc builds from csrc/bn_msm.hip:
# the accumulate kernel holds the mixed addition and the doubling of its P + P case, 19 Fq products in 7817 vector instructions; 10 of them
FQ_PRODUCTS_MADD, VALU_PER_FQ_PRODUCT = 10, 7817 / 19
ISSUE_CYCLES = 4.8          # per vector instruction per SIMD (profiles/r05_issue_cost_saturated.txt)


def plan(n):
    out = (C.c_uint32 * 4)(); nbytes = C.c_uint64()
    check(load().pil2gl_debug_bn128_msm_plan(n, out, C.byref(nbytes)))
    return {"c": out[0], "nWindows": out[1], "bucketsPerWindow": out[2], "windowsPerPass": out[3], "scratchBytes": nbytes.value}


def timed(fn, runs=5):
    fn(); torch.cuda.synchronize()
    ms = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--limit", type=int, default=240)
    ap.add_argument("--out")
    ap.add_argument("--small", action="store_true", help="n = 2^10, 2^12: a rehearsal of the tool, not a measurement")
    a = ap.parse_args()
    signal.alarm(a.limit)
    assert torch.cuda.is_available(), "this is a measurement: it needs the GPU"
    pil2gl.init(0)
    pts, _ = ref.known_log_bases(64, seed=1)
    tile = torch.from_numpy(ref.point_words(pts).view(np.int64)).cuda()
    lines = []
    for n_bits in ((10, 12) if a.small else (16, 20, 24)):
        n = 1 << n_bits
        bases = tile.repeat(n // 64, 1).contiguous()
        g = torch.Generator(device="cuda"); g.manual_seed(n_bits)
        scalars = torch.randint(0, 1 << 62, (n, 4), dtype=torch.int64, device="cuda", generator=g)
        scalars[:, 3] >>= 2                                 # below 2^252 < r: canonical Montgomery words
        out = torch.empty(8, dtype=torch.int64, device="cuda")
        med, lo, hi = timed(lambda: bn128.g1_msm(bases, scalars, n=n, out=out))
        p = plan(n)
        madds = n * p["nWindows"]
        floor_cycles = madds * FQ_PRODUCTS_MADD * VALU_PER_FQ_PRODUCT / 64 * ISSUE_CYCLES / SIMDS
        rec = {"op": "g1_msm", "n": n, "ms_median": round(med, 3), "ms_min": round(lo, 3), "ms_max": round(hi, 3),
               "Mpoints_per_s": round(n / med / 1e3, 3), "plan": p, "mixed_additions": madds,
               "floor_issue_ms_at_2.4GHz": round(floor_cycles / 2.4e6, 3), "floor_issue_ms_at_2.0GHz": round(floor_cycles / 2.0e6, 3)}
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
        del bases, scalars
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
