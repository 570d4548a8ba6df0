#!/usr/bin/env python3
"""Times the range-check multiplicities on the device (csrc/range_mult.hip; pil2gl.pilcheck.range_mult_dev) over both fields, by the method
of tools/bench_lookup_mult.py: 2^22 rows of Goldilocks and 2^20 of BN254 Fr, one side of f, a resident column, m a spare column of f's
matrix, the working buffer taken inside the timed call, which blocks for its report.  Two inputs for every size of the range:

  uniform   every row of f draws a value of the range at random
  one       every row of f holds ONE value: n adds to one counter

and beside every line the yardstick, timed in the same run: lookup_mult_dev with k = 1 on the materialised, padded range column of the
same n and the same f.  Every size that the LDS count kernel can take is timed on both count kernels, forced through the debug entry (the
planner's test-only argument), which is what the planner's threshold is read from.

Device events, one warm-up, the median (min, max) of five.  One JSON line per measurement.  The byte floor of the new call per row, from the
shapes: nF e read (e = 8 elemWords), e written (m), 4 bytes a counter (its add), and 4 size set by the init.
    python tools/bench_range_mult.py [--out profiles/range_mult_bench.txt] [--paths 0,1] [--fields gl,bn128]
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

SHAPES = {"gl": 1 << 22, "bn128": 1 << 20}
SIZES = (1 << 8, 1 << 16, 1 << 22)                   # the last one capped at n
LDS_SIZES = (1 << 8, 1 << 10, 1 << 11, 1 << 12, 1 << 13)      # what the LDS count kernel can take: timed on both kernels
R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
MONT = (1 << 256) % R
HBM_GBPS = 8000.0                                    # the figure DESIGN.md section 5 uses


def timed(fn, runs=5):
    fn(); torch.cuda.synchronize()
    ms = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return [round(x, 3) for x in (statistics.median(ms), min(ms), max(ms))]


def elements(field, values):
    """small non-negative integers as a (n, 2) matrix of elements, column 1 spare: words over Goldilocks, Montgomery words over Fr"""
    n = len(values)
    if field == "gl":
        m = np.zeros((n, 2), np.uint64)
        m[:, 0] = values
        return m
    out = np.zeros((n, 2, 4), np.uint64)
    uniq, inverse = np.unique(values, return_inverse=True)
    words = np.zeros((len(uniq), 4), np.uint64)
    for i, v in enumerate(uniq):
        x = int(v) * MONT % R
        words[i] = [(x >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(4)]
    out[:, 0] = words[inverse]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--paths", default="0,1", help="the count kernels timed at the sizes the LDS kernel can take")
    ap.add_argument("--fields", default="gl,bn128")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_range_mult needs a GPU"
    pil2gl.init(0)
    paths = [int(p) for p in args.paths.split(",")]
    lines = []

    def emit(**kw):
        lines.append(json.dumps(kw))
        print(lines[-1], flush=True)
    for field in args.fields.split(","):
        n = SHAPES[field]
        words = 1 if field == "gl" else 4
        e = 8 * words
        rng = np.random.default_rng(n)
        lo = 1000
        for size in sorted(set(min(s, n) for s in SIZES + LDS_SIZES)):
            dt = torch.from_numpy(elements(field, lo + np.minimum(np.arange(n), size - 1)).view(np.int64)).cuda()
            for name, vals in (("uniform", lo + rng.integers(0, size, n)), ("one", np.full(n, lo + size // 2))):
                df = torch.from_numpy(elements(field, vals).view(np.int64)).cuda()
                clean = (0, pilcheck.NONE, pilcheck.NONE, n)
                reps = []
                yard = timed(lambda: reps.append(pilcheck.lookup_mult_dev([(df, [0])], (dt, [0]), (dt, 1), n, field)))
                assert all(r == clean for r in reps), reps[-1]
                want = dt.clone()
                floor = n * e + n * e + 4 * n + 4 * size
                forced = paths if size in LDS_SIZES else []
                for path in [None] + forced:
                    reps = []
                    ms = timed(lambda: reps.append(pilcheck.range_mult_dev([(df, [0])], lo, size, (df, 1), n, field, 0, path)))
                    assert all(r == clean for r in reps), reps[-1]
                    a = df.view(n, 2, words)[:, 1]
                    assert torch.equal(a, want.view(n, 2, words)[:, 1]), "m differs from lookup_mult's"
                    plan = pilcheck.range_mult_plan(n, size, 1, field, path)
                    emit(op="range_mult_dev", input=name, field=field, rows=n, size=size, sides=1, forced=path, path=plan["path"], blocks=plan["blocks"],
                         threads=plan["threads"], call_ms=ms, lookup_mult_dev_ms=yard, ratio_to_lookup_mult=round(ms[0] / yard[0], 3), floor_bytes=floor,
                         GBps_of_floor_bytes=round(floor / ms[0] / 1e6, 1), share_of_8TBps=round(floor / ms[0] / 1e6 / HBM_GBPS, 4),
                         times="median, min, max of five; the call blocks for its report")
    if args.out:
        with open(args.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
