#!/usr/bin/env python3
"""Timing of the BN254 Fr expression evaluator (csrc/bn_expr.hip): a mul-heavy and an add-heavy synthetic program of about 600 ops, each
in both kernel forms (temporaries in LDS; 40 more values held alive, which sends them to the global working buffer), at 2^20 and 2^24
rows: one warm-up, then the median of five runs timed with device events, all under one time limit.  Beside each time: ops per second
(ops after the host passes x rows) and two floors derived without a run:
  vector issue         products x the vector instructions of the interpreter's product block in the built gfx950 ISA (328, of which 128 are
                       the 64-bit multiply-adds), sums x 80, differences x 40, x 4.8 issue cycles per instruction and SIMD
                       (profiles/r05_issue_cost_saturated.txt) over the chip's 1024 SIMDs
  temporary traffic    global form only: 96 B per op and lane (two 32-byte sources, one destination) against 8 TB/s
  python tools/bench_bn128_expr.py [--limit SECONDS] [--out FILE] [--small]        one JSON line per case"""
import argparse
import ctypes as C
import json
import os
import random
import signal
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "pil2-stark-js_amd", "python"))
import numpy as np
import torch
import pil2gl
from pil2gl import bn128
from pil2gl._lib import call

SIMDS = 256 * 4
VALU = {0: 80, 1: 40, 2: 328, 3: 0}     # add, sub, mul, copy: vector instructions of each op's block in bn_eval_kernel
ISSUE_CYCLES = 4.8
HBM_BYTES_PER_S = 8e12
ADD, SUB, MUL, COPY = 0, 1, 2, 3
WIDTH, N_SCALARS = 2, 4


def tmp(i): return (0, 1, 0, 0, i)
def sec(s, c=0, p=0): return (1, 1, s, p, c)
def scalar(i): return (2, 1, 0, 0, i)


def program(seed, n_ops, mul_share, hold):
    """four interleaved dependent chains over the cells of section 0 and the scalar pool (no two ops alike, so value numbering merges
    nothing but the repeated cell reads), summed into column 0 of section 1; hold products kept alive until the end"""
    rng = random.Random(seed)
    ops, nxt, held = [], 0, []
    for j in range(hold):
        ops.append((MUL, tmp(nxt), sec(0, j % WIDTH, j % 3 - 1), tmp(held[-1]) if held else scalar(0)))
        held.append(nxt); nxt += 1
    chains = []
    for c in range(4):
        ops.append((MUL, tmp(nxt), sec(0, c % WIDTH, c - 1), scalar(c % N_SCALARS)))
        chains.append(nxt); nxt += 1
    while len(ops) < n_ops:
        c = len(ops) % 4
        op = MUL if rng.random() < mul_share else rng.choice((ADD, SUB))
        other = sec(0, rng.randrange(WIDTH), rng.choice((-1, 0, 1))) if rng.random() < 0.5 else (scalar(rng.randrange(N_SCALARS)) if rng.random() < 0.3 else tmp(chains[(c + 1) % 4]))
        ops.append((op, tmp(nxt), tmp(chains[c]), other))
        chains[c] = nxt; nxt += 1
    acc = chains[0]
    for t in chains[1:] + held:
        ops.append((ADD, tmp(nxt), tmp(acc), tmp(t))); acc = nxt; nxt += 1
    ops.append((COPY, sec(1), tmp(acc), None))
    return ops


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
    ap.add_argument("--limit", type=int, default=300)
    ap.add_argument("--out")
    ap.add_argument("--small", action="store_true", help="2^10 and 2^12 rows: a rehearsal of the tool, not a measurement")
    a = ap.parse_args()
    signal.alarm(a.limit)
    assert torch.cuda.is_available(), "this is a measurement: it needs the GPU"
    pil2gl.init(0)
    sc = np.random.default_rng(1).integers(0, 1 << 62, size=(N_SCALARS, 4), dtype=np.uint64)          # below 2^254 < r: canonical
    lines = []
    for n_bits in ((10, 12) if a.small else (20, 24)):
        n = 1 << n_bits
        g = torch.Generator(device="cuda"); g.manual_seed(n_bits)
        src = torch.randint(0, 1 << 62, (n, WIDTH, 4), dtype=torch.int64, device="cuda", generator=g)
        src[:, :, 3] >>= 2                                                                          # below 2^252 < r
        dst = torch.zeros((n, 1, 4), dtype=torch.int64, device="cuda")
        for name, share in (("mul-heavy", 0.9), ("add-heavy", 0.1)):
            for hold in (0, 40):
                ops = program(7, 600, share, hold)
                plan = bn128.plan_program(ops, [WIDTH, 1], sc, n_bits)
                count = {k: sum(1 for o in ops if o[0] == k) for k in VALU}
                prog, ctx = bn128.make_context(ops, None, [src, dst], sc, n_bits, 0)          # encoded once: the timed call is the library's, not Python's
                stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
                med, lo, hi = timed(lambda: call("pil2gl_bn128_eval_program_dev", C.byref(prog), C.byref(ctx), stream))
                issue_cycles = n / 64 * sum(count[k] * VALU[k] for k in VALU) * ISSUE_CYCLES / SIMDS
                rec = {"op": "bn128_eval_program", "program": name, "rows": n, "ops_in": len(ops), "ops_run": plan["ops"], "slots": plan["slots"],
                       "form": "global" if plan["form"] else "lds", "threads": plan["threads"], "mul": count[MUL], "add": count[ADD], "sub": count[SUB],
                       "ms_median": round(med, 3), "ms_min": round(lo, 3), "ms_max": round(hi, 3),
                       "Gops_per_s": round(plan["ops"] * n / med / 1e6, 3),
                       "floor_issue_ms_at_2.4GHz": round(issue_cycles / 2.4e6, 3), "floor_issue_ms_at_2.0GHz": round(issue_cycles / 2.0e6, 3),
                       "floor_tmp_traffic_ms": round(96.0 * plan["ops"] * n / HBM_BYTES_PER_S * 1e3, 3) if plan["form"] else None}
                lines.append(json.dumps(rec))
                print(lines[-1], flush=True)
        del src, dst
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
