#!/usr/bin/env python3
"""Times the stage-2 half of the plookup argument on the device (pil2gl.pilcheck.plookup_prod_dev; csrc/hints.hip over Goldilocks,
csrc/bn_scan.hip over Fr): 2^22 rows of Goldilocks and 2^20 of BN254 Fr; k = 1 without selectors and a base-field h (the range-check
shape), k = 3 with both selectors, and k = 16, over resident matrices, the output a dense column.  Beside them, in the same session, the
yardstick at the parent's code path: gprod (pil2gl.calculateZ / pil2gl.bn128.gprod) on READY num and den columns of the same n, which
is the scan alone; the ratio over it is what the fold costs.  The evaluator pass that would materialise num and den is NOT timed here.

Device events, one warm-up, the median (min, max) of five.  One JSON line per measurement.  The byte floor is what the statement needs
read and written once, from the shapes:  (kF + kT + [selF] + [selT]) n e  (e = 8 elemWords)  +  2 n h  (h1 and h2, h = 8 hDim over
Goldilocks, 32 over Fr)  +  n o  (the column, o = 24 bytes over Goldilocks, 32 over Fr).  The neighbour rows (T' and h1') are other
lanes' rows and count once.  The working memory's traffic is on top of the floor.
    python tools/bench_plookup_prod.py [--out profiles/plookup_prod_bench.txt]
"""
import argparse
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "pil2-stark-js_amd", "python"))
import numpy as np
import torch
import pil2gl
from pil2gl import pilcheck, bn128

SHAPES = (("gl", 1 << 22), ("bn128", 1 << 20))
CASES = (("k = 1, no selectors, base-field h", 1, False, 1), ("k = 3, both selectors", 3, True, 3), ("k = 16", 16, False, 3))


def timed(fn, runs=5):
    fn(); torch.cuda.synchronize()
    ms = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return [round(x, 3) for x in (statistics.median(ms), min(ms), max(ms))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_plookup_prod needs a GPU"
    pil2gl.init(0)
    lines = []
    for field, n in SHAPES:
        words = 1 if field == "gl" else 4
        e, o = 8 * words, 24 if field == "gl" else 32
        rng = np.random.default_rng(n)
        mat = lambda cols: torch.from_numpy(rng.integers(0, 1 << 62, (n, cols) if words == 1 else (n, cols, 4), dtype=np.uint64).view(np.int64)).cuda()   # noqa: E731  below both moduli
        chal = [5, 6, 7] if words == 1 else [5, 6, 7, 8]
        out = torch.zeros((n, 3) if words == 1 else (n, 1, 4), dtype=torch.int64, device="cuda")
        # the yardstick: gprod over ready num and den columns of the same n (extension columns over Goldilocks)
        if words == 1:
            num, den = mat(3), mat(3)
            yard = timed(lambda: pil2gl.calculateZ(num, den, 3, 3, out))
        else:
            num, den = mat(1).reshape(n, 4), mat(1).reshape(n, 4)
            yard = timed(lambda: bn128.gprod(num, den, n, 1, 1, out, 1))
        lines.append(json.dumps({"op": "gprod_dev (ready num and den columns, the scan alone)", "field": field, "rows": n, "call_ms": yard,
                                 "times": "median, min, max of five"}))
        print(lines[-1], flush=True)
        del num, den
        for name, k, sels, h_dim in CASES:
            h_dim = h_dim if words == 1 else 1
            hw = h_dim if words == 1 else 1
            f, t, h = mat(k + 1), mat(k + 1), mat(2 * hw)
            cols = list(range(k))
            sf, st = (f, cols, (f, k) if sels else None), (t, cols, (t, k) if sels else None)
            ms = timed(lambda: pilcheck.plookup_prod_dev(sf, st, (h, 0), (h, hw), chal, chal, chal, chal, (out, 0), n, field, h_dim))
            plan = pilcheck.plookup_plan(n, k, k, field)
            fb = (2 * k + 2 * sels) * n * e + 2 * n * hw * e + n * o
            lines.append(json.dumps({"op": "plookup_prod_dev", "case": name, "field": field, "rows": n, "k": k, "h_dim": h_dim, "launches": plan["launches"],
                                     "work_bytes": plan["workBytes"], "call_ms": ms, "over_gprod_on_ready_columns": round(ms[0] / yard[0], 2), "floor_bytes": fb,
                                     "GBps_of_floor_bytes": round(fb / ms[0] / 1e6, 1), "share_of_8TBps": round(fb / ms[0] / 1e6 / 8000, 3),
                                     "times": "median, min, max of five"}))
            print(lines[-1], flush=True)
            del f, t, h, sf, st
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as fh:                  # one session a file: a second run replaces it
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
