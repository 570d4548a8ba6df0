#!/usr/bin/env python3
"""Times the lookup and permutation checks on the device (csrc/tuple_check.hip; pil2gl.pilcheck) over both fields: 2^22 rows x 3 columns
of Goldilocks and 2^20 x 3 of BN254 Fr, resident matrices, the working buffer taken inside the timed call, which blocks for its report.

  perm      f a random permutation of t's rows, all tuples distinct: a clean trace, so every row of both sides is inserted and judged
  lookup    f draws its rows from a table of 2^16 distinct tuples that t repeats: a clean lookup with counters in the tens

Device events, one warm-up, the median (min, max) of five.  One JSON line per measurement; the byte floor is what the statement needs
read and the table written and read, computed from the shapes:  2 n k 8 elemWords (each matrix once in the build)  +  the same again in the
judge (a permutation; a lookup judges f alone)  +  16 bytes a slot set before the build  +  per inserted row a 4-byte slot and an 8-byte
counter touched in the build and read in the judge.  Key re-reads on probes are on top and depend on the data.
    python tools/bench_tuple_check.py [--out profiles/tuple_check_bench.txt]
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
    """n distinct tuples: the row number in the first element's low word, random words below 2^62 elsewhere (below both moduli)"""
    m = rng.integers(0, 1 << 62, (n, k, words), dtype=np.uint64)
    m[:, 0, 0] = np.arange(n, dtype=np.uint64)
    return m.reshape(n, k) if words == 1 else m


def floor_bytes(n, k, words, mode, cap):
    sides = 2 if mode == pilcheck.PERMUTATION else 1
    return 2 * n * k * 8 * words + sides * n * k * 8 * words + 16 * cap + 2 * n * 12 + sides * n * 12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_tuple_check needs a GPU"
    pil2gl.init(0)
    lines = []
    for field, n, k in SHAPES:
        words = 1 if field == "gl" else 4
        rng = np.random.default_rng(n + k)
        t = matrix(rng, n, k, words)
        small = t[: 1 << 16]
        jobs = (("perm", pilcheck.perm_check_dev, pilcheck.PERMUTATION, t[rng.permutation(n)], t),
                ("lookup", pilcheck.lookup_check_dev, pilcheck.LOOKUP, small[rng.integers(0, 1 << 16, n)], small[np.arange(n) % (1 << 16)]))
        for name, fn, mode, f, tt in jobs:
            df, dt = (torch.from_numpy(np.ascontiguousarray(x).view(np.int64)).cuda() for x in (f, tt))
            verdict = []
            ms = timed(lambda: verdict.append(fn(df, list(range(k)), dt, list(range(k)), n, field)))
            assert all(v[0] == 0 for v in verdict), verdict[-1]
            plan = pilcheck.tuple_check_plan(n, k, field, mode)
            fb = floor_bytes(n, k, words, mode, 1 << plan["capBits"])
            lines.append(json.dumps({"op": name + "_check_dev", "field": field, "rows": n, "cols": k, "capBits": plan["capBits"], "launches": plan["launches"],
                                     "scratch_bytes": plan["scratchBytes"], "longest_probe": pilcheck.tuple_check_probe(), "check_ms": ms, "floor_bytes": fb,
                                     "GBps_of_floor_bytes": round(fb / ms[0] / 1e6, 1), "times": "median, min, max of five; the call blocks for its report"}))
            print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("# tools/bench_tuple_check.py, MI355X: the lookup and permutation checks (csrc/tuple_check.hip).  ONE box, ONE run.\n")
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
