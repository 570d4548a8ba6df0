#!/usr/bin/env python3
"""Timing of the recursion witness expansion (csrc/wtns_exec.hip) beside the thing it replaces, in one run on one box:
  compressor shape   2^22 rows x 12 Goldilocks columns, nWitness 2^22, 2^20 additions in six levels
  final shape        2^20 rows x 6 BN254 Fr columns, nWitness 2^20, 2^18 additions in six levels
Synthetic tables: operands and sMap entries drawn uniformly, a quarter of the cells zero.  Per shape, one warm-up and the median of five
runs timed with device events, of
  adds + gather   pil2gl.wtns.exec_dev on resident tables (what a proof runs after uploading w)
  gather          the fill alone; its traffic floor per cell is sMap 4 B + the cell written + the cell gathered (8 or 32 B each), against
                  the HBM rate DESIGN.md section 5 uses (8 TB/s) -- the gather is a random access, so the floor is far below its cost
  upload w        the pinned asynchronous upload of the witness through the host leg (pil2gl_dev_upload_async + copy_sync)
  upload trace    the same upload of the finished trace: what the host-side *_exec step needs today
and, in a line of its own per shape, of
  conn_pols_dev   the connection polynomials (csrc/conn_pols.hip) from the same resident sMap, N = the rows, unchecked, the working buffer
                  taken from torch's allocator inside the timed call as pil2gl.wtns.conn_pols_dev does for every caller
  conn_check_dev  the connection check (csrc/conn_check.hip) of the gathered trace against those S columns: a clean pair, so every cell is
                  probed and compared; the call blocks for its report, the working buffer is taken inside the timed call as above
  python tools/bench_wtns_exec.py [--limit SECONDS] [--out FILE] [--small]        one JSON line per case"""
import argparse
import ctypes as C
import json
import os
import signal
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "pil2-stark-js_amd", "python"))
import numpy as np
import torch
import pil2gl
from pil2gl import wtns, call

HBM_BYTES_PER_S = 8e12


def timed(fn, runs=5):
    fn(); torch.cuda.synchronize()
    ms = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def timed_upload(dst, n_words, runs=5):
    """host wall time of a pinned asynchronous upload of n_words and the wait for it (the copy stream is the library's own)"""
    pinned = C.c_void_p()
    call("pil2gl_host_alloc", n_words, C.byref(pinned))
    C.memset(pinned, 1, 8 * n_words)
    ms = []
    for k in range(runs + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call("pil2gl_dev_upload_async", C.c_void_p(dst.data_ptr()), pinned, n_words)
        call("pil2gl_copy_sync")
        if k:
            ms.append((time.perf_counter() - t0) * 1e3)
    call("pil2gl_host_free", pinned)
    return statistics.median(ms), min(ms), max(ms)


def synthetic(field, n_rows, n_cols, n_witness, n_adds, seed):
    """six levels: level l draws its operands from the witness and from level l - 1"""
    rng = np.random.default_rng(seed)
    per = n_adds // 6
    a = rng.integers(1, n_witness, n_adds, dtype=np.uint64)
    b = rng.integers(1, n_witness, n_adds, dtype=np.uint64)
    for l in range(1, 6):
        lo = n_witness + (l - 1) * per
        first, last = l * per, (l + 1) * per if l < 5 else n_adds
        b[first:last] = rng.integers(lo, lo + per, last - first, dtype=np.uint64)
    s_map = rng.integers(1, n_witness + n_adds, n_rows * n_cols, dtype=np.uint64)
    s_map[rng.random(s_map.size) < 0.25] = 0
    ex = {"field": field, "nWitness": n_witness, "nAdds": n_adds, "nSMap": n_rows, "nCols": n_cols, "sMap": s_map}
    if field == "gl":
        ex["adds"] = np.stack([a, b, rng.integers(0, 1 << 63, n_adds, dtype=np.uint64), rng.integers(0, 1 << 63, n_adds, dtype=np.uint64)], 1).reshape(-1)
    else:
        ex["addsIdx"] = np.stack([a, b], 1).reshape(-1)
        coef = rng.integers(0, 1 << 62, (2 * n_adds, 4), dtype=np.uint64)
        coef[:, 3] >>= np.uint64(2)
        ex["addsCoef"] = coef
    return ex


def rng_words(seed, n, words):
    """n elements as words below the moduli: uint64 for Goldilocks, (n, 4) for Fr"""
    a = np.random.default_rng(seed).integers(0, 1 << 62, (n, words), dtype=np.uint64)
    a[:, words - 1] >>= np.uint64(2)
    return a.reshape(-1) if words == 1 else a


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--limit", type=int, default=300)
    ap.add_argument("--out")
    ap.add_argument("--small", action="store_true", help="sizes 2^8 times smaller: a rehearsal of the tool, not a measurement")
    a = ap.parse_args()
    signal.alarm(a.limit)
    assert torch.cuda.is_available(), "this is a measurement: it needs the GPU"
    pil2gl.init(0)
    sh = 8 if a.small else 0
    lines = []
    for name, field, bits, n_cols, add_bits in (("compressor12", "gl", 22 - sh, 12, 20 - sh), ("final", "bn128", 20 - sh, 6, 18 - sh)):
        words = 1 if field == "gl" else 4
        n_rows = n_witness = 1 << bits
        n_adds = 1 << add_bits
        ex = synthetic(field, n_rows, n_cols, n_witness, n_adds, bits)
        prep = wtns.prepare(ex)
        assert prep["nLevels"] == 6, prep["nLevels"]
        n_w = prep["nW"]
        g = torch.Generator(device="cuda"); g.manual_seed(bits)
        w = torch.randint(0, 1 << 62, (n_w, words), dtype=torch.int64, device="cuda", generator=g)
        dst = torch.empty(n_rows * n_cols * words, dtype=torch.int64, device="cuda")
        cells = n_rows * n_cols
        both = timed(lambda: wtns.exec_dev(prep, w, dst))
        fill = timed(lambda: wtns.gather_dev(prep, w, dst))
        up_w = timed_upload(w, n_witness * words)
        up_t = timed_upload(dst, cells * words)
        floor_bytes = cells * (4 + 16 * words)
        floor_ms = floor_bytes / HBM_BYTES_PER_S * 1e3
        rec = {"op": "wtns_exec", "shape": name, "field": field, "rows": n_rows, "cols": n_cols, "nWitness": n_witness, "nAdds": n_adds, "levels": prep["nLevels"],
               "adds_gather_ms": [round(x, 3) for x in both], "gather_ms": [round(x, 3) for x in fill],
               "gather_floor_bytes": floor_bytes, "gather_GBps_of_floor_bytes": round(floor_bytes / fill[0] / 1e6, 1),
               "gather_floor_ms_at_8TBps": round(floor_ms, 4), "gather_ratio_to_floor": round(fill[0] / floor_ms, 1),
               "upload_w_ms": [round(x, 3) for x in up_w], "upload_w_GBps": round(8 * n_witness * words / up_w[0] / 1e6, 1),
               "upload_trace_ms": [round(x, 3) for x in up_t], "upload_trace_GBps": round(8 * cells * words / up_t[0] / 1e6, 1),
               "expand_plus_upload_w_ms": round(both[0] + up_w[0], 3), "trace_upload_over_expand_plus_upload_w": round(up_t[0] / (both[0] + up_w[0]), 2),
               "times": "median, min, max of five"}
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
        del dst
        # the connection polynomials from the same resident sMap (csrc/conn_pols.hip), N = the rows; w and ks' are multiplied as given, so any words do
        cw = rng_words(bits, 1, words)
        ks = rng_words(bits + 1, n_cols - 1, words)
        plan = wtns.conn_plan(n_rows, n_cols, n_w, n_rows, field)
        s_cols = torch.empty(n_rows * n_cols * words, dtype=torch.int64, device="cuda")
        conn = timed(lambda: wtns.conn_pols_dev(prep, n_rows, cw, ks, dst=s_cols))
        rec = {"op": "conn_pols_dev", "shape": name, "field": field, "rows": n_rows, "cols": n_cols, "nW": n_w, "passes": plan["passes"],
               "launches": plan["launches"], "scratch_bytes": plan["scratchBytes"], "conn_ms": [round(x, 3) for x in conn], "times": "median, min, max of five"}
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
        # the connection check (csrc/conn_check.hip) of the trace against those columns: clean, so every cell is probed and compared
        trace = wtns.gather_dev(prep, w)
        cplan = wtns.conn_check_plan(n_rows, n_cols, field)
        verdict = []
        chk = timed(lambda: verdict.append(wtns.conn_check_dev(trace, s_cols, n_cols, n_rows, cw, ks, field=field)))
        assert all(v is None for v in verdict), verdict[0]
        floor_bytes = cells * (8 + 24 * words)         # a slot written and read, S, a and the partner's a read
        rec = {"op": "conn_check_dev", "shape": name, "field": field, "rows": n_rows, "cols": n_cols, "capBits": cplan["capBits"],
               "launches": cplan["launches"], "scratch_bytes": cplan["scratchBytes"], "longest_probe": wtns.conn_check_probe(),
               "check_ms": [round(x, 3) for x in chk], "floor_bytes": floor_bytes, "GBps_of_floor_bytes": round(floor_bytes / chk[0] / 1e6, 1),
               "times": "median, min, max of five; the call blocks for its report"}
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
        del s_cols, prep, trace, w
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f_:
            f_.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
