#!/usr/bin/env python3
"""Times the lookup grand sum on the device (pil2gl.pilcheck.logup_sum_dev; csrc/hints.hip over Goldilocks, csrc/bn_scan.hip over Fr):
2^22 rows of Goldilocks and 2^20 of BN254 Fr, tuples of k = 3 columns, 2 and 9 terms over resident matrices, every term with a numerator
column, the output a dense column.  Beside it, in the same session, the only existing yardstick: the constant-numerator gsum
(pil2gl.calculateS / pil2gl.bn128.gsum) on a READY denominator column of the same n, which is the scan alone.

Device events, one warm-up, the median (min, max) of five.  One JSON line per measurement.  The byte floor is what the statement needs
read and written once, from the shapes:  nTerms (k + 1) n e  (tuples and numerators, e = 8 elemWords)  +  n o  (the column, o = 24 bytes
over Goldilocks, 32 over Fr).  The working memory's traffic (Goldilocks: tmp written and read, 48 n; Fr: D and N written and read, the
output column rewritten by inversion and scan) is on top of the floor.
    python tools/bench_logup_sum.py [--out profiles/logup_sum_bench.txt]
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
K = 3


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
    assert torch.cuda.is_available(), "bench_logup_sum needs a GPU"
    pil2gl.init(0)
    lines = []
    for field, n in SHAPES:
        words = 1 if field == "gl" else 4
        e, o = 8 * words, 24 if field == "gl" else 32
        rng = np.random.default_rng(n)
        shape = (n, K + 1) if words == 1 else (n, K + 1, 4)
        mats = [torch.from_numpy(rng.integers(0, 1 << 62, shape, dtype=np.uint64).view(np.int64)).cuda() for _ in range(9)]      # below both moduli
        elem = (lambda v: v) if words == 1 else (lambda v: [v, 0, 0, 0])
        chal = [5, 6, 7] if words == 1 else [5, 6, 7, 8]
        out = torch.zeros((n, 3) if words == 1 else (n, 1, 4), dtype=torch.int64, device="cuda")
        for n_terms in (2, 9):
            terms = [(m, list(range(K)), (m, K), elem(1 + u), elem(9)) for u, m in enumerate(mats[:n_terms])]
            ms = timed(lambda: pilcheck.logup_sum_dev(terms, chal, chal, (out, 0), n, field))
            plan = pilcheck.logup_sum_plan(n, n_terms, field)
            fb = n_terms * (K + 1) * n * e + n * o
            lines.append(json.dumps({"op": "logup_sum_dev", "field": field, "rows": n, "k": K, "terms": n_terms, "launches": plan["launches"],
                                     "work_bytes": plan["workBytes"], "call_ms": ms, "floor_bytes": fb, "GBps_of_floor_bytes": round(fb / ms[0] / 1e6, 1), "share_of_8TBps": round(fb / ms[0] / 1e6 / 8000, 3),
                                     "times": "median, min, max of five"}))
            print(lines[-1], flush=True)
        # the yardstick: gsum with ONE numerator element over a ready denominator column of the same n
        if words == 1:
            den = torch.from_numpy(rng.integers(1, 1 << 62, (n, 3), dtype=np.uint64).view(np.int64)).cuda()
            num = torch.tensor([3], dtype=torch.int64, device="cuda")
            ms = timed(lambda: pil2gl.calculateS(num, den, 1, 3, out))
        else:
            den = torch.from_numpy(rng.integers(1, 1 << 62, (n, 4), dtype=np.uint64).view(np.int64)).cuda()
            ms = timed(lambda: bn128.gsum(np.array([3, 0, 0, 0], np.uint64), den, n, 1, out, 1))
        lines.append(json.dumps({"op": "gsum_dev (ready denominator column, the scan alone)", "field": field, "rows": n, "call_ms": ms,
                                 "times": "median, min, max of five"}))
        print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as fh:                  # one session a file: a second run replaces it
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
