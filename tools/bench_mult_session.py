#!/usr/bin/env python3
"""Times the multiplicity sessions on the device (csrc/mult_session.hip; pil2gl.pilcheck.LookupSession / RangeSession) beside the one-shot
entries they were cut from, in ONE run: 2^22 rows a side of Goldilocks and of BN254 Fr, resident matrices, two inputs

  uniform   every row of f draws a value of the table at random
  one       every row of f holds ONE value: every add goes to one counter

and for each the session's open, an add of 1 side and of 8 sides (one matrix serves all eight), and write, then the yardstick on the same
rows: range_mult_dev / lookup_mult_dev with 1 and with 8 sides (their working buffer comes from torch's caching allocator inside the timed
call, as in tools/bench_range_mult.py), the call blocking for its report as an add does.
The range table is timed at a size on each count path (2^8: LDS, 2^16: global) with m of `size` rows (the table's own AIR) and of n rows
(the one-shot's shape); the lookup table at 2^16 rows and padded to n rows (the one-shot's shape, t[i] = min(i, 2^16 - 1)).

Device events around each call, one warm-up of every call, then five rounds that take every call of a configuration once, so that session
and yardstick alternate; the median (min, max) of the five.  One JSON line per configuration.  `add1_over_oneshot1`: an add of the same
rows over the WHOLE one-shot call (init, count, write): above 1 by more than the spread of the repeats means the add's own kernel is slower.
    python tools/bench_mult_session.py [--out profiles/mult_session_bench.txt] [--fields gl,bn128] [--rows 22]
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

R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
MONT = (1 << 256) % R
TABLE = 1 << 16


def timed_together(calls, rounds=5):
    """calls: name -> function.  One warm-up each, then `rounds` rounds of every call once -> name -> [median, min, max] in ms"""
    for fn in calls.values():
        fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in calls}
    for _ in range(rounds):
        for name, fn in calls.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); fn(); b.record(); torch.cuda.synchronize()
            ms[name].append(a.elapsed_time(b))
    return {name: [round(x, 3) for x in (statistics.median(v), min(v), max(v))] for name, v in ms.items()}


def elements(field, values):
    """small non-negative integers as a (n, 2) matrix of elements on the device, column 1 spare"""
    n = len(values)
    if field == "gl":
        m = np.zeros((n, 2), np.uint64)
        m[:, 0] = values
    else:
        m = np.zeros((n, 2, 4), np.uint64)
        uniq, inverse = np.unique(values, return_inverse=True)
        words = np.zeros((len(uniq), 4), np.uint64)
        for i, v in enumerate(uniq):
            x = int(v) * MONT % R
            words[i] = [(x >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(4)]
        m[:, 0] = words[inverse]
    return torch.from_numpy(m.view(np.int64)).cuda()


def column(t, col, n, words):
    return t.view(n, 2, words)[:, col]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--fields", default="gl,bn128")
    ap.add_argument("--rows", type=int, default=22, help="log2 of the rows a side")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_mult_session needs a GPU"
    pil2gl.init(0)
    n = 1 << args.rows
    lines = []

    def emit(**kw):
        ratio = lambda a, b: round(kw[a][0] / kw[b][0], 3)                       # noqa: E731
        kw.update(add1_over_oneshot1=ratio("add1_ms", "oneshot1_ms"), add8_over_oneshot8=ratio("add8_ms", "oneshot8_ms"),
                  times="ms: median, min, max of five alternating rounds; adds and one-shot calls block for their report, write for its total")
        lines.append(json.dumps(kw))
        print(lines[-1], flush=True)
    for field in args.fields.split(","):
        words = 1 if field == "gl" else 4
        rng = np.random.default_rng(n)
        lo = 1000
        scratch = lambda nbytes: torch.empty(max(nbytes // 8, 2), dtype=torch.int64, device="cuda")      # noqa: E731
        # ---- range sessions ----
        for size in (1 << 8, TABLE):
            dm_n, dm_size = elements(field, np.zeros(n, np.int64)), elements(field, np.zeros(size, np.int64))
            for name, vals in (("uniform", lo + rng.integers(0, size, n)), ("one", np.full(n, lo + size // 2))):
                df = elements(field, vals)
                side = (df, [0])
                s = pilcheck.RangeSession(lo, size, field)
                reopen = lambda: pilcheck.call("pil2gl_range_session_open_dev", size, pilcheck._ptr(s.work), s.bytes, pilcheck._stream())    # noqa: E731
                # the session against the one-shot call once: the same m, the same report
                want = pilcheck.range_mult_dev([side], lo, size, (dm_n, 1), n, field)
                assert s.add([side], [n]) == want and s.write((dm_n, 0), n) == n == want[3]
                assert torch.equal(column(dm_n, 0, n, words), column(dm_n, 1, n, words)), "the session's m differs from range_mult_dev's"
                got = timed_together({
                    "open_ms": reopen,
                    "add1_ms": lambda: s.add([side], [n]),
                    "oneshot1_ms": lambda: pilcheck.range_mult_dev([side], lo, size, (dm_n, 1), n, field),
                    "add8_ms": lambda: s.add([side] * 8, [n] * 8),
                    "oneshot8_ms": lambda: pilcheck.range_mult_dev([side] * 8, lo, size, (dm_n, 1), n, field),
                    "write_table_ms": lambda: s.write((dm_size, 0), size),
                    "write_n_ms": lambda: s.write((dm_n, 0), n),
                })
                emit(kind="range", field=field, input=name, rows_a_side=n, size=size, path=s.plan["path"], counter_bytes=s.plan["counterBytes"],
                     scratch_bytes=s.bytes, oneshot_scratch_bytes=pilcheck.range_mult_plan(n, size, 1, field)["scratchBytes"], **got)
                del df, s
        # ---- lookup sessions ----
        for n_t in (TABLE, n):
            dt = elements(field, np.minimum(np.arange(n_t), TABLE - 1))
            dt_n = dt if n_t == n else elements(field, np.minimum(np.arange(n), TABLE - 1))
            for name, vals in (("uniform", rng.integers(0, TABLE, n)), ("one", np.full(n, TABLE // 2))):
                df = elements(field, vals)
                side, t = (df, [0]), (dt, [0])
                s = pilcheck.LookupSession(t, n_t, field)
                reopen = lambda: pilcheck.call(s._name % "open", s.T, n_t, 1, pilcheck._ptr(s.work), s.bytes, pilcheck._stream())                # noqa: E731
                want = pilcheck.lookup_mult_dev([side], (dt_n, [0]), (df, 1), n, field)
                assert s.add([side], [n]) == want and s.write((dt, 1)) == n == want[3]
                assert torch.equal(column(dt, 1, n_t, words), column(df, 1, n, words)[:n_t]), "the session's m differs from lookup_mult_dev's"
                got = timed_together({
                    "open_ms": reopen,
                    "add1_ms": lambda: s.add([side], [n]),
                    "oneshot1_ms": lambda: pilcheck.lookup_mult_dev([side], (dt_n, [0]), (dt_n, 1), n, field),
                    "add8_ms": lambda: s.add([side] * 8, [n] * 8),
                    "oneshot8_ms": lambda: pilcheck.lookup_mult_dev([side] * 8, (dt_n, [0]), (dt_n, 1), n, field),
                    "write_table_ms": lambda: s.write((dt, 1)),
                })
                emit(kind="lookup", field=field, input=name, rows_a_side=n, table_rows=n_t, cap_bits=s.plan["capBits"], slot_bytes=s.plan["slotBytes"],
                     scratch_bytes=s.bytes, oneshot_scratch_bytes=pilcheck.lookup_mult_plan(n, 1, 1, field)["scratchBytes"], **got)
                del df, s
    if args.out:
        with open(args.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
