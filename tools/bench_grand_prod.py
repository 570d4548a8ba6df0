#!/usr/bin/env python3
"""Times the grand product of a permutation or a connection on the device (pil2gl.pilcheck.grand_prod_dev; csrc/hints.hip over Goldilocks,
csrc/bn_scan.hip over Fr): 2^22 rows of Goldilocks and 2^20 of BN254 Fr; a permutation of two terms with k = 3 and selectors, and
connections of 12 and 18 columns (24 and 36 terms with k = 1 and an id column each), over resident matrices, the output a dense column.
Beside them, in the same session, the yardstick at the parent's code path: gprod (pil2gl.calculateZ / pil2gl.bn128.gprod) on READY num
and den columns of the same n, which is the scan alone; the ratio over it is what the fold costs.  The evaluator pass that would
materialise num and den is NOT timed here.

Device events, one warm-up, the median (min, max) of five.  One JSON line per measurement.  The byte floor is what the statement needs
read and written once, from the shapes:  sum_u (k_u + [sel] + [id]) n e  (e = 8 elemWords)  +  n o  (the column, o = 24 bytes over
Goldilocks, 32 over Fr); a column that several terms read counts once per term.  The working memory's traffic is on top of the floor.
    python tools/bench_grand_prod.py [--out profiles/grand_prod_bench.txt]
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
    assert torch.cuda.is_available(), "bench_grand_prod needs a GPU"
    pil2gl.init(0)
    lines = []
    for field, n in SHAPES:
        words = 1 if field == "gl" else 4
        e, o = 8 * words, 24 if field == "gl" else 32
        rng = np.random.default_rng(n)
        mat = lambda cols: torch.from_numpy(rng.integers(0, 1 << 62, (n, cols) if words == 1 else (n, cols, 4), dtype=np.uint64).view(np.int64)).cuda()   # noqa: E731  below both moduli
        chal = [5, 6, 7] if words == 1 else [5, 6, 7, 8]
        out = torch.zeros((n, 3) if words == 1 else (n, 1, 4), dtype=torch.int64, device="cuda")
        f, t = mat(4), mat(4)
        cases = [("permutation, 2 terms, k = 3, selectors", pilcheck.perm_terms((f, [0, 1, 2], (f, 3)), (t, [0, 1, 2], (t, 3))))]
        for n_cols in (12, 18):
            a, S, x = mat(n_cols), mat(n_cols), mat(1)
            ks = [int(v) for v in rng.integers(2, 1 << 30, n_cols - 1)]
            cases.append(("connection, %d columns" % n_cols, pilcheck.conn_terms([(a, j) for j in range(n_cols)], [(S, j) for j in range(n_cols)], (x, 0), ks, chal, field)))
        for name, terms in cases:
            ms = timed(lambda: pilcheck.grand_prod_dev(terms, chal, chal, chal, (out, 0), n, field))
            sum_k = sum(len(tm[1]) for tm in terms)
            plan = pilcheck.grand_prod_plan(n, len(terms), sum_k, field)
            fb = sum(len(tm[1]) + (tm[2] is not None) + (tm[4] is not None) for tm in terms) * n * e + n * o
            lines.append(json.dumps({"op": "grand_prod_dev", "case": name, "field": field, "rows": n, "terms": len(terms), "sum_k": sum_k, "launches": plan["launches"],
                                     "work_bytes": plan["workBytes"], "call_ms": ms, "floor_bytes": fb, "GBps_of_floor_bytes": round(fb / ms[0] / 1e6, 1),
                                     "share_of_8TBps": round(fb / ms[0] / 1e6 / 8000, 3), "times": "median, min, max of five"}))
            print(lines[-1], flush=True)
            del terms
        # the yardstick: gprod over ready num and den columns of the same n (extension columns over Goldilocks)
        if words == 1:
            num = torch.from_numpy(rng.integers(1, 1 << 62, (n, 3), dtype=np.uint64).view(np.int64)).cuda()
            den = torch.from_numpy(rng.integers(1, 1 << 62, (n, 3), dtype=np.uint64).view(np.int64)).cuda()
            ms = timed(lambda: pil2gl.calculateZ(num, den, 3, 3, out))
        else:
            num = torch.from_numpy(rng.integers(1, 1 << 62, (n, 4), dtype=np.uint64).view(np.int64)).cuda()
            den = torch.from_numpy(rng.integers(1, 1 << 62, (n, 4), dtype=np.uint64).view(np.int64)).cuda()
            ms = timed(lambda: bn128.gprod(num, den, n, 1, 1, out, 1))
        lines.append(json.dumps({"op": "gprod_dev (ready num and den columns, the scan alone)", "field": field, "rows": n, "call_ms": ms,
                                 "times": "median, min, max of five"}))
        print(lines[-1], flush=True)
        del cases, f, t, num, den
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as fh:                  # one session a file: a second run replaces it
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
