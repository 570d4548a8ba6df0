#!/usr/bin/env python3
"""Timing of the BN254 Fr plookup hint (csrc/bn_h1h2.hip): bn128.h1h2 at n = 2^16, 2^20 and 2^24, stride 1 and stride 8 (columns of a
section 8 elements wide, inputs and outputs alike).  t holds distinct values and f is drawn uniformly from it.  One warm-up, then the
median of five runs timed with device events, all under one time limit.  The time includes the 8-byte readback of the missing cell the
call blocks for.  Beside each time, the traffic floor derived without a run: the bytes the launches must move at the least, against
the HBM rate DESIGN.md section 5 uses (8 TB/s):
  clears   4 cap (table) + 4 n (counts)                                   written
  insert   32 n (t) read, 4 n slots written (a slot per distinct value)
  count    32 n (f) read, 4 n slots read, 4 n counters updated; the key compare reads t[slot] again: 32 n
  scan     4 n read, 4 n written
  expand   4 n starts read, 32 n (t) read, 64 n (h1, h2) written         (the least any expand step reads; the kernel as built loads 1024
           starts for every 512 rows, 8 n, and the probes of one 256-ary search per workgroup: DESIGN.md section 16)
which is 4 cap + 220 n bytes; a strided column moves the same elements (the floor counts elements, not the 64-byte sectors around them).
The table and the t[slot] reads are random accesses, so the floor is far below what they cost; the ratio says how far.
  python tools/bench_bn128_h1h2.py [--limit SECONDS] [--out FILE] [--small]        one JSON line per case"""
import argparse
import json
import os
import signal
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "pil2-stark-js_amd", "python"))
import torch
import pil2gl
from pil2gl import bn128

HBM_BYTES_PER_S = 8e12
BYTES_PER_ROW = 220


def timed(fn, runs=5):
    fn(); torch.cuda.synchronize()
    ms = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def column(elems, stride):
    """(n, 4) elements as a column of a section `stride` wide (the other columns zero), flat"""
    if stride == 1:
        return elems.reshape(-1).contiguous()
    sec = torch.zeros((elems.shape[0], stride, 4), dtype=torch.int64, device="cuda")
    sec[:, 0] = elems
    return sec.reshape(-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--limit", type=int, default=240)
    ap.add_argument("--out")
    ap.add_argument("--small", action="store_true", help="sizes 2^8 times smaller: a rehearsal of the tool, not a measurement")
    a = ap.parse_args()
    signal.alarm(a.limit)
    assert torch.cuda.is_available(), "this is a measurement: it needs the GPU"
    pil2gl.init(0)
    sh = 8 if a.small else 0
    lines = []
    for n_bits in (16 - sh, 20 - sh, 24 - sh):
        n = 1 << n_bits
        g = torch.Generator(device="cuda"); g.manual_seed(n_bits)
        t = torch.randint(0, 1 << 62, (n, 4), dtype=torch.int64, device="cuda", generator=g)
        t[:, 3] >>= 2                                       # below 2^252 < r: canonical words
        t[:, 0] = torch.arange(n, dtype=torch.int64, device="cuda")       # distinct
        f = t[torch.randint(0, n, (n,), device="cuda", generator=g)]      # uniform from t
        for stride in (1, 8):
            cf, ct = column(f, stride), column(t, stride)
            h1 = torch.zeros(n * stride * 4, dtype=torch.int64, device="cuda")
            h2 = torch.zeros(n * stride * 4, dtype=torch.int64, device="cuda")
            fn = lambda: bn128.h1h2(cf, ct, n=n, f_stride=stride, t_stride=stride, h1=h1, h1_stride=stride, h2=h2, h2_stride=stride)      # noqa: E731
            med, lo, hi = timed(fn)
            plan = bn128.h1h2_plan(n)
            floor_bytes = 4 * plan["capacity"] + BYTES_PER_ROW * n
            floor_ms = floor_bytes / HBM_BYTES_PER_S * 1e3
            rec = {"op": "h1h2", "n": n, "stride": stride, "ms_median": round(med, 3), "ms_min": round(lo, 3), "ms_max": round(hi, 3),
                   "Mrows_per_s": round(n / med / 1e3, 1), "plan": plan, "floor_bytes": floor_bytes,
                   "floor_traffic_ms_at_8TBps": round(floor_ms, 4), "ratio_to_floor": round(med / floor_ms, 1)}
            lines.append(json.dumps(rec))
            print(lines[-1], flush=True)
            del cf, ct, h1, h2
            torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f_:
            f_.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
