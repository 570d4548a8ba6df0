#!/usr/bin/env python3
"""Times the range-check grand sum on the device (pil2gl.pilcheck.range_sum_dev; csrc/hints.hip over Goldilocks, csrc/bn_scan.hip over Fr)
against its yardstick IN THE SAME RUN: logup_sum_dev with the same n and terms, each range replaced by a k = 1 term over a materialised
t column and the same m column.  2^22 rows of Goldilocks and 2^20 of BN254 Fr; shapes (nF, nR) = (0, 1), (0, 8), (1, 1), (8, 1); an f
term has one column and a numerator column; every window is all rows; the output a dense column; the resident form.

Device events, one warm-up, the median (min, max) of five.  One JSON line per shape.  The byte floor is what the statement needs read and
written once, from the shapes, e = 8 elemWords, o = 24 bytes over Goldilocks and 32 over Fr:
    logup_sum    (2 nF + 2 nR) n e + n o        (an f term's column and numerator; a range's t and m)
    range_sum    logup_sum's minus n e a range   (no t)
The working memory's traffic is on top of the floor in both.  Not timed: the host forms, strided outputs, each kernel by itself, counters.
    python tools/bench_range_sum.py [--out profiles/range_sum_bench.txt]
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
TERMS = ((0, 1), (0, 8), (1, 1), (8, 1))


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
    assert torch.cuda.is_available(), "bench_range_sum needs a GPU"
    pil2gl.init(0)
    lines = []
    for field, n in SHAPES:
        words = 1 if field == "gl" else 4
        e, o = 8 * words, 24 if field == "gl" else 32
        rng = np.random.default_rng(n)
        rand = lambda cols: torch.from_numpy(rng.integers(1, 1 << 62, (n, cols) if words == 1 else (n, cols, 4), dtype=np.uint64).view(np.int64)).cuda()  # noqa: E731  below both moduli
        f, m = rand(16), rand(8)                         # eight f terms' columns and numerators; eight m columns
        los = [1000 * r for r in range(8)]
        # the materialised t columns of the yardstick: lo_r + i as canonical elements (Montgomery form over Fr, made with the library)
        if words == 1:
            t = torch.stack([torch.arange(n, dtype=torch.int64) + lo for lo in los], 1).contiguous().cuda()
        else:
            plain = np.zeros((n, 8, 4), np.uint64)
            for r, lo in enumerate(los):
                plain[:, r, 0] = np.arange(n, dtype=np.uint64) + np.uint64(lo)
            mont = np.zeros_like(plain)
            pil2gl._lib.call("pil2gl_bn128_convert", pil2gl._ptr(plain), n * 8, 1, pil2gl._ptr(mont))
            t = torch.from_numpy(mont.view(np.int64)).cuda()
        elem = (lambda v: v) if words == 1 else (lambda v: [v, 0, 0, 0])
        chal = [5, 6, 7] if words == 1 else [5, 6, 7, 8]
        out = torch.zeros((n, 3) if words == 1 else (n, 1, 4), dtype=torch.int64, device="cuda")
        ref = torch.zeros_like(out)
        for n_f, n_r in TERMS:
            terms = [(f, [2 * u], (f, 2 * u + 1), elem(1 + u), elem(9)) for u in range(n_f)]
            ranges = [((m, r), los[r], n, 0, elem(3 + r), elem(20 + r)) for r in range(n_r)]
            as_terms = terms + [(t, [r], (m, r), elem(3 + r), elem(20 + r)) for r in range(n_r)]
            ms = timed(lambda: pilcheck.range_sum_dev(terms, ranges, chal, chal, (out, 0), n, field))
            yard = timed(lambda: pilcheck.logup_sum_dev(as_terms, chal, chal, (ref, 0), n, field))
            torch.cuda.synchronize()
            assert torch.equal(out, ref), "range_sum_dev and logup_sum_dev on the materialised columns differ"
            plan = pilcheck.range_sum_plan(n, n_f, n_r, field)
            floor_y = (2 * n_f + 2 * n_r) * n * e + n * o
            fb = floor_y - n_r * n * e
            lines.append(json.dumps({"op": "range_sum_dev", "field": field, "rows": n, "nF": n_f, "nR": n_r, "launches": plan["launches"], "work_bytes": plan["workBytes"],
                                     "call_ms": ms, "logup_sum_dev_ms": yard, "median_over_yardstick_median": round(ms[0] / yard[0], 3),
                                     "median_within_yardstick_max": ms[0] <= yard[2], "floor_bytes": fb, "logup_floor_bytes": floor_y,
                                     "GBps_of_floor_bytes": round(fb / ms[0] / 1e6, 1), "share_of_8TBps": round(fb / ms[0] / 1e6 / 8000, 3),
                                     "times": "median, min, max of five; the two results compared word for word"}))
            print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as fh:                  # one session a file: a second run replaces it
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
