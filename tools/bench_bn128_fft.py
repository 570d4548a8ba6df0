#!/usr/bin/env python3
"""Timing of the BN254 Fr transforms (csrc/bn_ntt.hip): fft at 2^20 x 16 and 2^24 x 4, interpolate at 2^20 x 16 with two extension bits.
One warm-up, then the median of five runs timed with device events, all under one time limit.  Beside each time: the sweeps of the plan,
the bytes those sweeps move (64 B per element per sweep) over the time against 8 TB/s, the products (n/2 * nBits * nPols) per second, and
the two floors derived without a run: the traffic of the planned sweeps at 8 TB/s, and the vector issue of the built ISA.
  python tools/bench_bn128_fft.py [--limit SECONDS] [--out FILE] [--small]        one JSON line per case"""
import argparse
import ctypes as C
import json
import os
import signal
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "pil2-stark-js_amd", "python"))
import torch
import pil2gl
from pil2gl import bn128

HBM_BYTES_PER_S = 8e12
SIMDS = 256 * 4
# vector instructions of the kernel's loops in the gfx950 ISA hipcc 7 builds from csrc/bn_ntt.hip (counted in the .s of --save-temps):
# a butterfly with its product / the distance-1 layer's butterfly without / the seam pass per element (two products)
VALU_BUTTERFLY, VALU_BUTTERFLY_PLAIN, VALU_SEAM = 471, 138, 679
ISSUE_CYCLES = 4.8          # per vector instruction per SIMD at >= 2 waves (profiles/r05_issue_cost_saturated.txt: 4.5-5.1 for this mix)


def plan(n_bits):
    layers = (C.c_uint32 * 8)(); n = C.c_uint32()
    pil2gl.check(pil2gl.load().pil2gl_debug_bn128_fft_plan(n_bits, layers, 8, C.byref(n)))
    return list(layers[:n.value])


def model(n_bits, n_pols, inverse=False):
    """(sweeps, bytes moved, lane-level vector instructions) of one transform"""
    layers = plan(n_bits)
    elems = n_pols << n_bits
    valu = elems // 2 * ((n_bits - len(layers)) * VALU_BUTTERFLY + len(layers) * VALU_BUTTERFLY_PLAIN) + elems * (len(layers) - 1) * VALU_SEAM
    if inverse:
        valu += elems * VALU_SEAM // 2
    return len(layers), 64 * elems * len(layers), valu


def words(n_bits, n_pols, seed):
    g = torch.Generator(device="cuda"); g.manual_seed(seed)
    t = torch.randint(0, 1 << 62, (1 << n_bits, n_pols, 4), dtype=torch.int64, device="cuda", generator=g)
    t[:, :, 3] >>= 2                                   # below 2^252 < r: canonical
    return t


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
    ap.add_argument("--limit", type=int, default=240)
    ap.add_argument("--out")
    ap.add_argument("--small", action="store_true", help="2^14 rows: a rehearsal of the tool, not a measurement")
    a = ap.parse_args()
    signal.alarm(a.limit)
    assert torch.cuda.is_available(), "this is a measurement: it needs the GPU"
    pil2gl.init(0)
    cases = [("fft", 20, 16, 0), ("fft", 24, 4, 0), ("interpolate", 20, 16, 2)]
    if a.small:
        cases = [(op, 14, p, e) for op, _, p, e in cases]
    lines, out = [], None
    for op, n_bits, n_pols, ext in cases:
        x = words(n_bits, n_pols, n_bits)
        if op == "fft":
            out = torch.empty_like(x)
            med, lo, hi = timed(lambda: bn128.fft(x, n_pols, n_bits, out=out))
            sweeps, moved, valu = model(n_bits, n_pols)
            muls = (1 << n_bits) // 2 * n_bits * n_pols
        else:
            med, lo, hi = timed(lambda: bn128.interpolate(x, n_pols, n_bits, n_bits + ext))
            s1, m1, v1 = model(n_bits, n_pols, True)
            s2, m2, v2 = model(n_bits + ext, n_pols)
            pad = 32 * (n_pols << (n_bits + ext))              # the coefficient copy (read + write) and the zero rows
            sweeps, moved, valu = s1 + s2, m1 + m2 + pad, v1 + v2
            muls = (1 << n_bits) // 2 * n_bits * n_pols + (1 << (n_bits + ext)) // 2 * (n_bits + ext) * n_pols
            del out
        issue_cycles = valu / 64 * ISSUE_CYCLES / SIMDS
        rec = {"op": op, "nBits": n_bits, "nPols": n_pols, "extBits": ext, "ms_median": round(med, 3), "ms_min": round(lo, 3), "ms_max": round(hi, 3),
               "sweeps": sweeps, "plan_bytes": moved, "TB_per_s": round(moved / med / 1e9, 3), "share_of_8TBps": round(moved / med / 1e9 / 8, 3),
               "fr_mul": muls, "Gmul_per_s": round(muls / med / 1e6, 2),
               "floor_traffic_ms": round(moved / HBM_BYTES_PER_S * 1e3, 3),
               "floor_issue_ms_at_2.4GHz": round(issue_cycles / 2.4e6, 3), "floor_issue_ms_at_2.0GHz": round(issue_cycles / 2.0e6, 3)}
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
        del x
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
