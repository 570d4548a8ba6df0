#!/usr/bin/env python3
"""Timing of the BN254 G1 stage commit (pil2gl_bn128_g1_commit_dev, csrc/bn_msm.hip) against the path a caller had before it, on one device
and one build: K packed polynomials of m = 4 slots and n = m * rows coefficients each, K in {1, 3, 6}, n in {2^16, 2^20, 2^24}, all columns
of one row-major coefficient matrix of K * m columns.
  (a) batched     one g1_commit call on the matrix
  (b) unpacked    per polynomial, m strided column copies into a second buffer (device copy kernels; a caller of the C ABI would use
                  hipMemcpy2DAsync), then one g1_msm call on it: K calls
One warm-up, then the median of five runs timed with device events, min and max beside it, all under one time limit.  Bases are 64
multiples of the generator tiled over the array, so the gathers of the bucket phase hit cache: the times are those of the arithmetic and
the fixed part of a call, not of a real pTau's traffic.  Scalars are uniform Montgomery words below r.  (a) and (b) are compared byte for
byte before they are timed.
  python tools/bench_bn128_commit.py [--limit SECONDS] [--out FILE] [--small]        one JSON line per case"""
import argparse
import ctypes as C
import json
import os
import signal
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "pil2-stark-js_amd", "python"))
sys.path.insert(0, os.path.join(HERE, "..", "tests"))
import numpy as np
import torch
import pil2gl
from pil2gl import bn128
from pil2gl._lib import check, load
import bn128_g1_ref as ref

M = 4


def batch_plan(counts):
    out = (C.c_uint32 * 4)(); nbytes = C.c_uint64()
    check(load().pil2gl_debug_bn128_msm_batch_plan(len(counts), (C.c_uint64 * len(counts))(*counts), out, C.byref(nbytes)))
    return {"c": out[0], "nWindows": out[1], "bucketsPerWindow": out[2], "windowsPerPass": out[3], "scratchBytes": nbytes.value}


def timed(fn, runs=5):
    fn(); torch.cuda.synchronize()
    ms = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return round(statistics.median(ms), 3), round(min(ms), 3), round(max(ms), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--limit", type=int, default=420)
    ap.add_argument("--out")
    ap.add_argument("--small", action="store_true", help="n = 2^10, 2^12: a rehearsal of the tool, not a measurement")
    a = ap.parse_args()
    signal.alarm(a.limit)
    assert torch.cuda.is_available(), "this is a measurement: it needs the GPU"
    pil2gl.init(0)
    pts, _ = ref.known_log_bases(64, seed=1)
    tile = torch.from_numpy(ref.point_words(pts).view(np.int64)).cuda()
    lines = []
    for n_bits in ((10, 12) if a.small else (16, 20, 24)):
        n = 1 << n_bits
        rows = n // M
        bases = tile.repeat(n // 64, 1).contiguous()
        for K in (1, 3, 6):
            cols = K * M
            g = torch.Generator(device="cuda"); g.manual_seed(100 * n_bits + K)
            matrix = torch.randint(0, 1 << 62, (rows, cols, 4), dtype=torch.int64, device="cuda", generator=g)
            matrix[:, :, 3] >>= 2                           # below 2^252 < r: canonical Montgomery words
            polys = [(0, rows, [M * k + j for j in range(M)]) for k in range(K)]
            out_a = torch.empty((K, 8), dtype=torch.int64, device="cuda")
            out_b = torch.empty((K, 8), dtype=torch.int64, device="cuda")
            packed = torch.empty((rows, M, 4), dtype=torch.int64, device="cuda")        # the second buffer, reused per polynomial

            def batched():
                bn128.g1_commit(bases, matrix, polys, cols, out=out_a)

            def unpacked(copy=True, msm=True):
                for k in range(K):
                    if copy:
                        for j in range(M):
                            packed[:, j, :].copy_(matrix[:, M * k + j, :])
                    if msm:
                        bn128.g1_msm(bases, packed, n=n, out=out_b[k])

            batched(); unpacked(); torch.cuda.synchronize()
            assert torch.equal(out_a, out_b), "the batched call and the K single calls differ"
            rec = {"op": "g1_commit", "K": K, "m": M, "n_each": n, "plan": batch_plan([n] * K)}
            for name, fn in (("batched", batched), ("unpacked", unpacked), ("unpacked_copies_only", lambda: unpacked(msm=False)),
                             ("unpacked_msm_only", lambda: unpacked(copy=False))):
                rec["ms_" + name], rec["ms_" + name + "_min"], rec["ms_" + name + "_max"] = timed(fn)
            rec["speedup"] = round(rec["ms_unpacked"] / rec["ms_batched"], 3)
            lines.append(json.dumps(rec))
            print(lines[-1], flush=True)
            del matrix, packed
            torch.cuda.empty_cache()
        del bases
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
