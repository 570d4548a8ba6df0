#!/usr/bin/env python3
"""Times the clustered logUp sum on the device (pil2gl.pilcheck.logup_cluster_dev; csrc/hints.hip over Goldilocks, csrc/bn_scan.hip over Fr)
against two yardsticks IN THE SAME RUN:
    (a) one logup_sum_dev / range_sum_dev call on all terms: what the im columns cost on top of s;
    (b) that call plus one such call per cluster: the nearest thing a caller could do before, still without the differencing, so a floor
        on the alternative.
2^22 rows of Goldilocks and 2^20 of BN254 Fr; an f term has k = 3 columns and a numerator column, a range's window is all rows; shapes
(terms, nIm) = (2, 1); (9, 4) with one DIRECT term; (9, 9); nF = 0, nR = 8 in four clusters.  s and the im columns are neighbouring columns of
one matrix; the resident form.

Device events, one warm-up, the median (min, max) of five.  One JSON line per shape.  The byte floor is what the statement needs read and
written once, e = 8 elemWords, o = 24 bytes over Goldilocks and 32 over Fr:  (4 nF + nR) n e + (1 + nIm) n o.  The working memory's traffic
is on top of it.  Not timed: the host forms, short windows, other k, each kernel by itself, counters, more than one session.
    python tools/bench_logup_cluster.py [--out profiles/logup_cluster_bench.txt]
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

SHAPES = (("gl", 1 << 22), ("bn128", 1 << 20))
D = pilcheck.DIRECT
# (nF, nR, the cluster of every term, f terms first)
CASES = ((2, 0, [0, 0]), (8, 1, [0, 0, 1, 1, 2, 2, 3, 3, D]), (8, 1, [0, 1, 2, 3, 4, 5, 6, 7, 8]), (0, 8, [0, 0, 1, 1, 2, 2, 3, 3]))


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
    assert torch.cuda.is_available(), "bench_logup_cluster needs a GPU"
    pil2gl.init(0)
    lines = []
    for field, n in SHAPES:
        words = 1 if field == "gl" else 4
        width = 3 if words == 1 else 1
        e, o = 8 * words, 24 if field == "gl" else 32
        rng = np.random.default_rng(n)
        rand = lambda cols: torch.from_numpy(rng.integers(1, 1 << 62, (n, cols) if words == 1 else (n, cols, 4), dtype=np.uint64).view(np.int64)).cuda()  # noqa: E731  below both moduli
        f, m = rand(32), rand(8)                         # eight f terms' three columns and numerators; eight m columns
        elem = (lambda v: v) if words == 1 else (lambda v: [v, 0, 0, 0])
        chal = [5, 6, 7] if words == 1 else [5, 6, 7, 8]
        outs = torch.zeros((n, 10 * width) if words == 1 else (n, 10, 4), dtype=torch.int64, device="cuda")
        ref = torch.zeros((n, width) if words == 1 else (n, 1, 4), dtype=torch.int64, device="cuda")

        def plain(terms, ranges):
            if ranges:
                pilcheck.range_sum_dev(terms, ranges, chal, chal, (ref, 0), n, field)
            else:
                pilcheck.logup_sum_dev(terms, chal, chal, (ref, 0), n, field)
        for n_f, n_r, cluster in CASES:
            terms = [(f, [4 * u, 4 * u + 1, 4 * u + 2], (f, 4 * u + 3), elem(1 + u), elem(9)) for u in range(n_f)]
            ranges = [((m, r), 1000 * r, n, 0, elem(3 + r), elem(20 + r)) for r in range(n_r)]
            n_im = 1 + max(c for c in cluster if c != D)
            im = [(outs, (1 + c) * width) for c in range(n_im)]
            ms = timed(lambda: pilcheck.logup_cluster_dev(terms, ranges, cluster, im, chal, chal, (outs, 0), n, field))
            yard_a = timed(lambda: plain(terms, ranges))
            torch.cuda.synchronize()
            got = outs.reshape(n, 10, -1)[:, 0].reshape(ref.shape)
            assert torch.equal(got, ref), "logup_cluster_dev's s and the plain call's differ"
            per = []
            for c in range(n_im):
                ct = [t for u, t in enumerate(terms) if cluster[u] == c]
                cr = [r for v, r in enumerate(ranges) if cluster[n_f + v] == c]
                per.append(timed(lambda: plain(ct, cr)))
            yard_b = [round(yard_a[k] + sum(p[k] for p in per), 3) for k in range(3)]
            plan = pilcheck.logup_cluster_plan(n, n_f, n_r, n_im, field)
            fb = (4 * n_f + n_r) * n * e + (1 + n_im) * n * o
            lines.append(json.dumps({"op": "logup_cluster_dev", "field": field, "rows": n, "nF": n_f, "nR": n_r, "nIm": n_im, "direct": sum(c == D for c in cluster),
                                     "launches": plan["launches"], "work_bytes": plan["workBytes"], "call_ms": ms, "plain_sum_ms": yard_a,
                                     "plain_sum_plus_one_per_cluster_ms": yard_b, "median_over_a": round(ms[0] / yard_a[0], 3),
                                     "median_over_b": round(ms[0] / yard_b[0], 3), "at_or_below_b": ms[0] <= yard_b[0], "floor_bytes": fb,
                                     "GBps_of_floor_bytes": round(fb / ms[0] / 1e6, 1), "share_of_8TBps": round(fb / ms[0] / 1e6 / 8000, 3),
                                     "times": "median, min, max of five; (b) adds the medians, minima and maxima of its calls; s compared word for word with (a)'s"}))
            print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as fh:                  # one session a file: a second run replaces it
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
