"""Which kernel an expression-evaluator call ran, and real programs at circuit size against the oracle.

pil2gl_eval_program_dev (csrc/expr.hip) has three device forms:
  * "jit": the straight-line kernel hiprtc builds for the program (temporaries in registers).  With PIL2GL_JIT_INFO=1 every
    launch prints `pil2gl jit_eval: N ops, regs R, lds L, scratch S, max threads T` to stderr; nothing else prints that line.
  * "interp" / "lds": eval_kernel<true>, temporaries in LDS, when slots * 3 * 64 * 8 bytes fit 60 KiB;
  * "interp" / "global": eval_kernel<false>, temporaries in a global [slot][lane] array.
Both interpreter forms use persistent lanes: the grid is capped, and rows beyond it are taken by a second turn of the row loop.
The two interpreter forms print nothing; which one ran follows from the slot count, taken from pil2gl_debug_plan_program
(the optimiser exactly as the evaluator runs it) and the rule of expr.hip restated below.  The helpers set PIL2GL_JIT_INFO and
read stderr through pytest's capfd: they never change how a program is routed."""
import ctypes as C
import re

import numpy as np

P = 0xFFFFFFFF00000001
JIT_LINE = re.compile(r"pil2gl jit_eval: (\d+) ops, regs (\d+), lds (\d+), scratch (\d+), max threads (\d+)")
FALLBACK = "run-time compilation unavailable"
SLOT_CAP = 200                      # expr.hip: the compiled kernel only takes programs of at most 200 slots
LDS_LIMIT = 60 * 1024               # expr.hip: the LDS form when slots * 3 * 64 * 8 bytes fit
LDS_MAX_BLOCKS = 256 * 64           # expr.hip: grid cap of the LDS form (16384 blocks of 256 >> k threads)
GLOBAL_LANES = 256 * 8 * 256        # expr.hip: grid cap of the global form (2048 blocks of 256 threads)


def _c_program(ops, n_tmp, widths, scalars, n_bits, prime_shift):
    import gl_oracle
    from pil2gl import _lib
    prog = gl_oracle.make_program(ops, n_tmp, struct_op=_lib.GlxOp, struct_prog=_lib.GlxProgram)
    cs = (_lib.GlxSection * len(widths))()
    for i, w in enumerate(widths):
        cs[i].ptr = 0; cs[i].width = w
    scalars = np.ascontiguousarray(scalars, dtype=np.uint64)
    ctx = _lib.GlxCtx(n_bits, prime_shift, len(widths), scalars.size, cs, scalars.ctypes.data_as(_lib.u64p))
    ctx._keep = (cs, scalars)
    return prog, ctx


def plan(ops, n_tmp, widths, scalars, n_bits=16, prime_shift=0):
    """(slots, ops, fused Horner terms) of the program as the evaluator optimises it (host only)"""
    from pil2gl import _lib
    prog, ctx = _c_program(ops, n_tmp, widths, scalars, n_bits, prime_shift)
    info = (C.c_uint32 * 3)()
    assert _lib.load().pil2gl_debug_plan_program(C.byref(prog), C.byref(ctx), info) == 0, _lib.load().pil2gl_last_error()
    return info[0], info[1], info[2]


def compact(ops, n_tmp):
    """(slots, ops) after value numbering and slot allocation, without Horner fusion (pil2gl_debug_compact_program, host only)"""
    import gl_oracle
    from pil2gl import _lib
    prog = gl_oracle.make_program(ops, n_tmp, struct_op=_lib.GlxOp, struct_prog=_lib.GlxProgram)
    out = (_lib.GlxOp * (2 * len(ops) + 16))(); info = (C.c_uint32 * 2)()
    assert _lib.load().pil2gl_debug_compact_program(C.byref(prog), out, info) == 0, _lib.load().pil2gl_last_error()
    return info[0], info[1]


def interp_form(slots):
    """the interpreter form a program of `slots` slots takes and the lanes its grid launches (expr.hip, `interpreter:`)"""
    slots = max(slots, 1)
    if slots * 3 * 64 * 8 <= LDS_LIMIT:
        threads = 256
        while slots * 3 * threads * 8 > LDS_LIMIT:
            threads //= 2
        return "lds", LDS_MAX_BLOCKS * threads
    return "global", GLOBAL_LANES


def jit_launches(capfd, monkeypatch, run):
    """run() with PIL2GL_JIT_INFO=1: the compiled-kernel launches it made, as dicts.  A hiprtc fallback fails the test."""
    monkeypatch.setenv("PIL2GL_JIT_INFO", "1")
    capfd.readouterr()
    try:
        run()
    finally:
        _, err = capfd.readouterr()
        monkeypatch.delenv("PIL2GL_JIT_INFO")
    assert FALLBACK not in err, err[-2000:]
    return [dict(zip(("ops", "regs", "lds", "scratch", "max_threads"), map(int, m.groups()))) for m in JIT_LINE.finditer(err)]


def eval_path(capfd, monkeypatch, run, ops, n_tmp, widths, scalars, n_bits, prime_shift):
    """run() evaluates the program (ops, n_tmp) once on sections of `widths` columns.  Returns ("jit", {ops, regs, lds, scratch,
    max_threads}) if the compiled kernel ran, ("interp", {form: "lds" | "global", slots, lanes}) if an interpreter kernel did."""
    launches = jit_launches(capfd, monkeypatch, run)
    assert len(launches) <= 1, launches
    slots, n_ops, _ = plan(ops, n_tmp, widths, scalars, n_bits, prime_shift)
    if launches:
        assert launches[0]["ops"] == n_ops and slots <= SLOT_CAP, (launches[0], slots, n_ops)
        return "jit", launches[0]
    form, lanes = interp_form(slots)
    return "interp", {"form": form, "slots": slots, "lanes": lanes}


# ---------------------------------------------------------------------------------------------------------------------------
# circuit-size runs
EDGE_PAIR = ((1 << 32) + 1, (1 << 32) - 1)          # (2^32 + 1)(2^32 - 1) = 2^64 - 1: a lazy product's non-canonical output


def edge_rows(width):
    """the four edge rows: all zero, all p - 1, and the two arrangements of the (2^32 + 1, 2^32 - 1) column pairs"""
    pair = [EDGE_PAIR[c & 1] for c in range(width)]
    swap = [EDGE_PAIR[1 - (c & 1)] for c in range(width)]
    return np.array([[0] * width, [P - 1] * width, pair, swap], dtype=np.uint64)


def fill_section(rng, n_rows, width, prime_shift):
    """random canonical values; rows 0-3 are the edge rows, and so are the last 2^prime_shift rows (where a `prime` offset wraps
    through the mask to row 0), cycling through them.  Every column gets them, so the three components of extension values do."""
    a = rng.integers(0, P, size=(n_rows, width), dtype=np.uint64)
    e = edge_rows(width)
    a[:4] = e
    tail = 1 << prime_shift
    a[n_rows - tail:] = e[(np.arange(tail) + 1) % 4]
    return a


def windows(n_rows, lanes, w=4096):
    """[0, w), w rows centred on each multiple of the launched lane count inside the domain, [N - w, N)"""
    out = [(0, w)]
    for m in range(lanes, n_rows, lanes):
        out.append((m - w // 2, m + w // 2))
    out.append((n_rows - w, n_rows))
    return out


def run_device(ops, n_tmp, secs, scalars, n_bits, prime_shift, dest):
    """the program on the device; secs: list of host arrays (rows, width); returns the destination section after the run.
    The destination starts as all-ones words, which no canonical result equals: a row the kernel skips cannot pass."""
    import torch
    from pil2gl import _lib
    prog, ctx = _c_program(ops, n_tmp, [s.shape[1] for s in secs], scalars, n_bits, prime_shift)
    dev = []
    for i, s in enumerate(secs):
        t = torch.full(s.shape, -1, dtype=torch.int64, device="cuda") if i == dest else torch.from_numpy(s.view(np.int64)).cuda()
        dev.append(t)
        ctx._keep[0][i].ptr = t.data_ptr()
    _lib.call("pil2gl_eval_program_dev", C.byref(prog), C.byref(ctx), None)
    torch.cuda.synchronize()
    got = dev[dest].cpu().numpy().view(np.uint64)
    del dev
    return got


def run_oracle(oracle, ops, n_tmp, secs, scalars, n_bits, prime_shift, dest, wins=None):
    """the oracle's destination section on the whole domain, or on the row windows `wins` only (other rows stay zero)"""
    out = list(secs)
    out[dest] = np.zeros_like(secs[dest])
    for b, e in (wins or [(0, 1 << n_bits)]):
        oracle.eval_program(ops, n_tmp, out, scalars, n_bits, prime_shift, b, e)
    return out[dest]


def bigint_row(code, secs_by_name, info, ctx, row, n_bits, prime_shift):
    """tests/stark_ref.py's big-integer exec_code on one row of a prover op-list (leaves resolved from the sections by their meaning,
    not through the encoder): the value its last op writes"""
    import stark_ref
    mask = (1 << n_bits) - 1

    def cell(name, col, dim, prime=0):
        r = secs_by_name[name][(row + (prime << prime_shift)) & mask]
        return int(r[col]) if dim == 1 else [int(v) for v in r[col:col + 3]]

    def resolve(r):
        t = r["type"]
        if t == "number": return int(r["value"], 0) % P
        if t == "public": return int(ctx["publics"][r["id"]]) % P
        if t == "challenge": return [int(v) for v in ctx["challenges"][r["stage"] - 1][r["stageId"]]]
        if t == "eval": return [int(v) for v in ctx["evals"][r["id"]]]
        if t == "cm":
            p = info["cmPolsMap"][r["id"]]
            return cell("cm%d_ext" % p["stage"], p["stagePos"], p["dim"], r.get("prime", 0))
        if t == "const": return cell("const_ext", r["id"], 1, r.get("prime", 0))
        if t == "Zi": return cell("Zi_ext#%d" % r["boundaryId"], 0, 1)
        if t == "xDivXSubXi": return cell("xDivXSubXi_ext", 3 * r["id"], 3)
        raise ValueError(t)
    v = stark_ref.exec_code(code, resolve)
    return [int(c) % P for c in (v if isinstance(v, list) else [v, 0, 0])]


FIB_WIDTHS = {"const_ext": 2, "cm2_ext": 6, "q_ext": 3, "Zi_ext#0": 1, "xDivXSubXi_ext": 6, "f_ext": 3}


def fibonacci_program(k, which, n_bits, prime_shift, seed):
    """expressionsCode[which] of stark.fibonacci_air(k) -- 0 the constraint program, 1 the FRI program -- encoded as the prover
    encodes it, with random challenges / evaluations / publics and every section it reads filled by fill_section"""
    from pil2gl import stark
    rng = np.random.default_rng(seed)
    info, exprs, _ = stark.fibonacci_air(k, {"nBits": n_bits - 3, "nBitsExt": n_bits, "nQueries": 8, "steps": [{"nBits": n_bits}]})
    r3 = lambda: [int(v) for v in rng.integers(0, P, 3, dtype=np.uint64)]
    ctx = {"pilInfo": info, "publics": [int(v) for v in rng.integers(0, P, 3, dtype=np.uint64)],
           "challenges": [[], [r3()], [r3()], [r3(), r3()]], "evals": [r3() for _ in info["evMap"]]}
    code = exprs["expressionsCode"][which]["code"]["code"]
    ops, n_tmp, names, scalars = stark.encode_code(code, "ext", ctx)
    widths = [2 * k if n == "cm1_ext" else FIB_WIDTHS[n] for n in names]
    dest = names.index("q_ext" if which == 0 else "f_ext")
    secs = [np.zeros((1 << n_bits, w), np.uint64) if i == dest else fill_section(rng, 1 << n_bits, w, prime_shift)
            for i, w in enumerate(widths)]
    return {"code": code, "ops": ops, "n_tmp": n_tmp, "names": names, "secs": secs, "scalars": scalars, "info": info, "ctx": ctx,
            "dest": dest, "n_bits": n_bits, "prime_shift": prime_shift}


def check_at_size(oracle, capfd, monkeypatch, pr, wins=None, bigint=True):
    """pr (as fibonacci_program returns it) on the device, bit-exact against the oracle on every row (wins None) or on the row windows
    `wins`; the first, middle and last rows also against the big-integer interpreter.  Returns eval_path's (path, info)."""
    ops, n_tmp, secs, sc, nb, ps, d = pr["ops"], pr["n_tmp"], pr["secs"], pr["scalars"], pr["n_bits"], pr["prime_shift"], pr["dest"]
    box = {}
    path = eval_path(capfd, monkeypatch, lambda: box.update(got=run_device(ops, n_tmp, secs, sc, nb, ps, d)),
                     ops, n_tmp, [s.shape[1] for s in secs], sc, nb, ps)
    got = box["got"].reshape(secs[d].shape)
    want = run_oracle(oracle, ops, n_tmp, secs, sc, nb, ps, d, wins)
    rows = np.concatenate([np.arange(b, e) for b, e in wins]) if wins else slice(None)
    bad = np.nonzero((got[rows] != want[rows]).any(axis=1))[0]
    assert bad.size == 0, ("rows differ", (np.arange(1 << nb)[rows])[bad[:8]].tolist(), path)
    if bigint:
        named = dict(zip(pr["names"], secs))
        for r in (0, (1 << nb) // 2, (1 << nb) - 1):
            v = bigint_row(pr["code"], named, pr["info"], pr["ctx"], r, nb, ps)
            assert [int(x) for x in got[r]] == v[:secs[d].shape[1]], r
    return path
