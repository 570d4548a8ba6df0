#!/usr/bin/env python3
"""Times the lookup multiplicities on the device (csrc/lookup_mult.hip; pil2gl.pilcheck.lookup_mult_dev) over both fields: 2^22 rows x 3
columns of Goldilocks and 2^20 x 3 of BN254 Fr, one side of f, resident matrices, m a spare column of t's matrix, the working buffer taken
inside the timed call, which blocks for its report.  Two inputs of the same size, t the same n distinct tuples in both:

  uniform   every row of f draws a row of t at random: n counters, a handful of adds each
  one       every row of f holds ONE tuple of t: n adds to one counter, the case of a range check

Device events, one warm-up, the median (min, max) of five.  One JSON line per measurement; the byte floor is what the statement needs
read and the table written and read, computed from the shapes:  n k e (t in the build, e = 8 elemWords)  +  n k e (f in the count)  +  n k e
(t again in the write)  +  n e (m)  +  8 bytes a slot set by the init  +  per row of t a 4-byte slot claimed and read again, per row of f a
slot read and a 4-byte add.  Key re-reads on probes are on top and depend on the data.
    python tools/bench_lookup_mult.py [--label merged] [--out profiles/lookup_mult_bench.txt]
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
from pil2gl import pilcheck

SHAPES = (("gl", 1 << 22, 3), ("bn128", 1 << 20, 3))


def timed(fn, runs=5):
    fn(); torch.cuda.synchronize()
    ms = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return [round(x, 3) for x in (statistics.median(ms), min(ms), max(ms))]


def matrix(rng, n, k, words):
    """n distinct tuples in k + 1 columns, the last one spare: the row number in the first element's low word, random words below 2^62
    elsewhere (below both moduli)"""
    m = rng.integers(0, 1 << 62, (n, k + 1, words), dtype=np.uint64)
    m[:, 0, 0] = np.arange(n, dtype=np.uint64)
    return m.reshape(n, k + 1) if words == 1 else m


def floor_bytes(n, k, words, cap):
    e = 8 * words
    return 3 * n * k * e + n * e + 8 * cap + 2 * n * 4 + n * 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--label", default="", help="names the build that is measured, e.g. the variant of the count")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_lookup_mult needs a GPU"
    pil2gl.init(0)
    lines = []
    for field, n, k in SHAPES:
        words = 1 if field == "gl" else 4
        rng = np.random.default_rng(n + k)
        t = matrix(rng, n, k, words)
        dt = torch.from_numpy(np.ascontiguousarray(t).view(np.int64)).cuda()
        cols = list(range(k))
        for name, rows in (("uniform", rng.integers(0, n, n)), ("one", np.full(n, 12345))):
            df = torch.from_numpy(np.ascontiguousarray(t[rows]).view(np.int64)).cuda()
            reports = []
            ms = timed(lambda: reports.append(pilcheck.lookup_mult_dev([(df, cols)], (dt, cols), (dt, k), n, field)))
            assert all(r == (0, pilcheck.NONE, pilcheck.NONE, n) for r in reports), reports[-1]
            plan = pilcheck.lookup_mult_plan(n, k, 1, field)
            fb = floor_bytes(n, k, words, 1 << plan["capBits"])
            lines.append(json.dumps({"op": "lookup_mult_dev", "build": args.label, "input": name, "field": field, "rows": n, "cols": k, "sides": 1,
                                     "capBits": plan["capBits"], "launches": plan["launches"], "scratch_bytes": plan["scratchBytes"],
                                     "longest_probe": pilcheck.lookup_mult_probe(), "call_ms": ms, "floor_bytes": fb,
                                     "GBps_of_floor_bytes": round(fb / ms[0] / 1e6, 1), "times": "median, min, max of five; the call blocks for its report"}))
            print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
