"""CPU-side checks of the C-ABI library: it loads, exports every symbol include/pil2gl.h declares,
and refuses to compute without a GPU (no silent fallback)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT

pil2gl = pytest.importorskip("pil2gl")
from pil2gl import _lib  # noqa: E402


def _declared():
    src = open(os.path.join(ROOT, "include", "pil2gl.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(pil2gl_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_every_declared_symbol():
    lib = _lib.load()
    names = _declared()
    assert len(names) >= 40
    for n in names:
        assert hasattr(lib, n), "libpil2gl.so does not export " + n
    # the Python binding binds exactly the declared set
    assert sorted(_lib.SIGNATURES) == names


def test_expr_struct_layout_matches_header():
    # include/pil2gl_expr.h: glx_ref 16 bytes, glx_op 56 bytes
    assert C.sizeof(_lib.GlxRef) == 16 and C.sizeof(_lib.GlxOp) == 56
    assert C.sizeof(_lib.GlxSection) == 16


def test_merkle_num_nodes_host_only(oracle):
    lib = _lib.load()
    for h in list(range(1, 70)) + [255, 256, 257, 1 << 20, (1 << 20) + 3]:
        assert lib.pil2gl_merkle_num_nodes(h) == oracle.merkle_num_nodes(h)


def test_scalar_field_exports_against_the_references_vectors():
    """pil2gl_add / _mul / _square = the WASM module's scalar exports (glwasm.js:47-96,1269-1275): host arithmetic, against the products
    and sums the reference's f3g.js wrote into tests/golden/field.json; operands above p are reduced first"""
    from conftest import golden, H, P
    lib = _lib.load()
    g = golden("field.json")
    for a, b, m, s, d in H(g["mul"]):
        assert lib.pil2gl_mul(a, b) == m and lib.pil2gl_add(a, b) == s and lib.pil2gl_square(a) == a * a % P
    assert lib.pil2gl_mul(P + 5, 3) == 15 and lib.pil2gl_add(2 ** 64 - 1, 1) == (2 ** 64) % P and lib.pil2gl_square(P - 1) == 1


def _have_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


@pytest.mark.skipif(_have_gpu(), reason="only meaningful on a machine without a GPU")
def test_no_cpu_fallback_without_gpu():
    a = np.arange(8, dtype=np.uint64)
    out = np.zeros(16, np.uint64)
    with pytest.raises(pil2gl.Pil2glError) as e:
        pil2gl.interpolate(a, 1, 3, out, 4)
    assert "-2" in str(e.value) or "no HIP device" in str(e.value)
    with pytest.raises(pil2gl.Pil2glError):
        pil2gl.buildMerkleHash(False).merkelize(a, 1, 8)


_PLAN_HOOKS = {"-": {}, "G1": {"PIL2GL_NTT_GENERIC": "1"}, "W0": {"PIL2GL_LDE_WIDEFWD": "0"},
               "K4": {"PIL2GL_NTT_KMAX": "4"}, "K6": {"PIL2GL_NTT_KMAX": "6"}, "K9": {"PIL2GL_NTT_KMAX": "9"}, "K10": {"PIL2GL_NTT_KMAX": "10"}}


def test_transform_plans_are_the_recorded_ones(monkeypatch):
    """every launch of fft / ifft / interpolate / the extension from coefficients -- kernel instance, tile geometry, workgroup, grid, LDS
    bytes, flags -- equals the table in tests/golden/transform_plans.txt.gz, one line per call: `hooks op nBits columns extBits cosets :
    launch ; launch ...` (fields of a launch: include/pil2gl.h, pil2gl_debug_plan_transform; cosets 0 = the whole extension).
    The table was recorded from the code BEFORE plan_ntt / plan_lde existed, whose launch sites wrote their parameters instead of
    launching: 2^0..2^18, 2^20, 2^21, 2^24, 2^27, 2^30 rows x 20 widths from 1 to 200 columns x extensions by 0..3 bits and slices of 1..3
    cosets of 8, with the test hooks unset and at each value the tests use.  Equal plans are equal kernels, grids and LDS: a change of
    the planner that means to move a launch updates the table with it and says so."""
    import gzip
    import transform_plan as tp
    with gzip.open(os.path.join(ROOT, "tests", "golden", "transform_plans.txt.gz"), "rt") as f:
        lines = f.read().splitlines()
    assert len(lines) == 7 * 24 * 20 * (2 + 2 * 7)
    seen, hooks = set(), None
    for ln in lines:
        head, want = ln.split(" :")
        hook, op, nb, c, eb, cc = head.split()
        if hook != hooks:
            for k in ("PIL2GL_NTT_KMAX", "PIL2GL_NTT_GENERIC", "PIL2GL_LDE_WIDEFWD"):
                monkeypatch.delenv(k, raising=False)
            for k, v in _PLAN_HOOKS[hook].items():
                monkeypatch.setenv(k, v)
            hooks = hook
        seen.add(head)
        assert tp.line(tp.plan(op, int(nb), int(c), int(eb), int(cc))) == want.strip(), head
    assert len(seen) == len(lines) and {h.split()[0] for h in seen} == set(_PLAN_HOOKS)


def test_transform_plan_reaches_what_the_gpu_tests_claim(monkeypatch):
    """the kernel families and pass sizes the GPU tests name, from the host-only plan: which shapes run fixed-geometry instances, that
    no default plan takes a 15-slot PASS instance (rows of 15 columns are under 128 bytes: 7-stage passes) while PIL2GL_NTT_KMAX=9
    does, and that the mid kernel only ever needs 2, 4, 8 or 16 rows per lane"""
    import gzip
    import transform_plan as tp
    for k in ("PIL2GL_NTT_KMAX", "PIL2GL_NTT_GENERIC", "PIL2GL_LDE_WIDEFWD"):
        monkeypatch.delenv(k, raising=False)
    assert [(l.kind, l.k, l.fixed) for l in tp.plan("interpolate", 17, 100, 1)] == [("i", 5, 0), ("i", 4, 0), ("m", 8, 16), ("d", 5, 0), ("d", 4, 0)]
    assert [(l.kind, l.k, l.fixed) for l in tp.plan("interpolate", 14, 15, 3)] == [("i", 6, 0), ("m", 8, 15), ("d", 6, 0)]
    assert [(l.k, l.fixed, l.scatter, l.canon) for l in tp.plan("fft", 20, 100)] == [(8, 16, 0, 0), (8, 16, 0, 0), (4, 0, 1, 1)]
    assert tp.plan("fft", 0, 5) == [] and tp.plan("interpolate", 9, 0, 1) == []
    with gzip.open(os.path.join(ROOT, "tests", "golden", "transform_plans.txt.gz"), "rt") as f:
        table = [ln.split(" :") for ln in f.read().splitlines()]
    ept, pass15 = set(), set()
    for head, launches in table:
        for l in filter(None, launches.strip().split(" ; ")):
            v = l.split()
            if v[0] == "m":
                ept.add(int(v[9]))
            elif v[8] == "15":
                pass15.add(head.split()[0])
    assert ept == {2, 4, 8, 16} and pass15 == {"K9", "K10"}
    monkeypatch.setenv("PIL2GL_NTT_KMAX", "9")
    assert [(l.kind, l.k, l.fixed) for l in tp.plan("fft", 8, 15)] == [("f", 8, 15)]
    assert [(l.kind, l.k, l.fixed) for l in tp.plan("interpolate", 16, 15, 0)] == [("i", 8, 15), ("m", 8, 15), ("d", 8, 15)]
    lib = _lib.load()
    n = C.c_uint32()
    assert lib.pil2gl_debug_plan_transform(0, 31, 1, 31, 0, None, 0, C.byref(n)) != 0       # beyond the largest domain
    assert lib.pil2gl_debug_plan_transform(2, 9, 1, 8, 0, None, 0, C.byref(n)) != 0         # nBitsExt < nBits
    assert lib.pil2gl_debug_plan_transform(4, 9, 1, 9, 0, None, 0, C.byref(n)) != 0         # no such transform


def test_tmp_compaction_preserves_program(oracle):
    """host-side live-range renumbering of temporaries (expr.hip) must not change what the program computes"""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_gpu_parity import _random_program
    from conftest import rand_field
    lib = _lib.load()
    for n_ops in (5, 20, 300, 1500):
        rng = np.random.default_rng(n_ops)
        n_bits = 5
        widths = [5, 9, 1, 3]
        secs = [rand_field(rng, (1 << n_bits, w)) for w in widths]
        secs[-1][:] = 0
        scalars = rand_field(rng, 40)
        ops, n_tmp = _random_program(rng, n_ops, widths, scalars.size, len(widths) - 1)
        ref = [s.copy() for s in secs]
        oracle.eval_program(ops, n_tmp, ref, scalars, n_bits, 0)
        prog = oracle.make_program(ops, n_tmp, struct_op=_lib.GlxOp, struct_prog=_lib.GlxProgram)
        out = (_lib.GlxOp * (2 * len(ops) + 16))(); info = (C.c_uint32 * 2)()
        assert lib.pil2gl_debug_compact_program(C.byref(prog), out, info) == 0
        n_slots = C.c_uint32(info[0])
        assert n_slots.value <= n_tmp + 64 and (n_ops < 100 or n_slots.value < n_tmp // 2)
        ops2 = []
        for o in list(out)[:info[1]]:
            def ref_(r):
                return (r.kind, r.dim, r.section, r.prime, r.index)
            ops2.append((o.op, ref_(o.dest), ref_(o.src[0]), ref_(o.src[1]) if o.op != 3 else None))
        got = [s.copy() for s in secs]
        oracle.eval_program(ops2, max(1, n_slots.value), got, scalars, n_bits, 0)
        for a, b in zip(got, ref):
            assert (a == b).all(), n_ops


def test_evaluator_routing_of_the_reference_programs(oracle):
    """why each evaluator test takes the kernel it takes: (ops as encoded, slots after compaction) of the programs the GPU tests run,
    from pil2gl_debug_compact_program, and the slots the evaluator's own choice reads (pil2gl_debug_plan_program: Horner fusion
    included, which moves some counts by one).  The compiled kernel takes programs of at most 200 slots: the two long programs the
    reference wrote are over that cap and run in the global-memory interpreter; the FRI program of fibonacci_air(k) (2k + 2 slots)
    crosses it between k = 99 and k = 100; 40 slots (k = 19) is the largest that keeps its temporaries in LDS.  Fails when
    compaction or fusion changes, so that the routing the GPU tests assert is revisited."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import bn128_oracle as bn
    import evalpath as ep
    from conftest import rand_field
    from pil2gl import stark
    from test_gpu_parity import _random_program
    import test_ref_oplist
    import test_reference_proof
    W = {"x_ext": 3, "f_ext": 3, "Zi_ext#0": 1, "const_ext": 64, "cm1_ext": 1024, "cm2_ext": 6, "cm3_ext": 64, "cm4_ext": 64,
         "q_ext": 3, "xDivXSubXi_ext": 6}

    def counts(ops, n_tmp, secs, scalars):
        slots, _ = ep.compact(ops, n_tmp)
        return len(ops), slots, ep.plan(ops, n_tmp, [W[s] for s in secs], scalars)[0]
    # verifyEvals verifierCode + its store
    inp = test_ref_oplist._inputs(4)
    ctx = {"pilInfo": {}, "publics": inp["publics"], "evals": inp["evals"], "challengesFlat": inp["challengesFlat"], "challenges": []}
    assert counts(*stark.encode_code(test_ref_oplist._load(), "ext", ctx)) == (3258, 330, 331)
    # test/final qVerifier (muladd expanded) and queryVerifier
    info, vinfo, _, z = test_reference_proof._final()
    tr = test_reference_proof._final_transcript(bn.TranscriptBN128(16), z, info)
    ctx = {"pilInfo": info, "publics": [int(v) for v in z["publics"]], "evals": [[int(v) for v in e] for e in z["evals"]], "challenges": tr["challenges"]}
    assert counts(*stark.encode_code(vinfo["qVerifier"]["code"], "ext", ctx)) == (2697, 309, 310)
    assert counts(*stark.encode_code(vinfo["queryVerifier"]["code"], "ext", ctx)) == (317, 37, 36)
    # fibonacci_air(k): constraint program (expressionsCode[0]) and FRI program ([1])
    fib = {}
    for k in (19, 20, 50, 99, 100, 150, 400):
        pr = [ep.fibonacci_program(k, e, 8, 0, seed=k) for e in (0, 1)]
        fib[k] = [counts(p["ops"], p["n_tmp"], p["names"], p["scalars"]) for p in pr]
    assert [fib[k][0] for k in (50, 150, 400)] == [(661, 7, 6), (1961, 7, 6), (5211, 7, 7)]
    for k in fib:
        assert fib[k][1] == (12 * k + 12, 2 * k + 2, 2 * k + 2), k
    cap = ep.SLOT_CAP
    assert fib[99][1][2] <= cap < fib[100][1][2]
    assert max(fib[k][0][2] for k in (50, 150, 400)) <= cap < min(331, 310)
    assert (ep.interp_form(fib[19][1][2]), ep.interp_form(fib[20][1][2])) == (("lds", 1 << 20), ("global", 1 << 19))
    # _random_program(300) of test_expression_evaluator_interpreter_and_jit_agree (the table counts its ops after compaction: 340)
    rng = np.random.default_rng(1300)
    widths = [5, 9, 1, 3]
    for w in widths:
        rand_field(rng, (1 << 10, w))
    scalars = rand_field(rng, 40)
    ops, n_tmp = _random_program(rng, 300, widths, scalars.size, 3)
    assert ep.compact(ops, n_tmp) == (77, 340)
    assert ep.plan(ops, n_tmp, widths, scalars)[0] == 77


def test_constraint_program_compiles_with_hiprtc_and_fuses_horner():
    """the run-time compiled evaluator path: optimiser + source generator + hiprtc, on the synthetic AIR's cExp (no GPU)"""
    import time
    from pil2gl import stark
    lib = _lib.load()
    ss = {"nBits": 16, "nBitsExt": 19, "nQueries": 8, "steps": [{"nBits": 19}, {"nBits": 14}, {"nBits": 9}]}
    info, exprs, _ = stark.fibonacci_air(10, ss)
    ctx = {"pilInfo": info, "publics": [1, 2, 3], "challenges": [[], [[5, 6, 7]], [[1, 1, 1]], [[2, 2, 2], [3, 3, 3]]], "evals": [[i, i + 1, i + 2] for i in range(len(info["evMap"]))]}
    ops, n_tmp, secs, scalars = stark.encode_code(exprs["expressionsCode"][0]["code"]["code"], "ext", ctx)
    prog = stark.make_c_program(ops, n_tmp)
    widths = {"const_ext": 2, "cm1_ext": 20, "q_ext": 3, "Zi_ext#0": 1}
    cs = (_lib.GlxSection * len(secs))()
    for i, name in enumerate(secs):
        cs[i].ptr = 0; cs[i].width = widths[name]
    c = _lib.GlxCtx(19, 3, len(secs), scalars.size, cs, scalars.ctypes.data_as(_lib.u64p))
    nbytes = C.c_uint64(); fused = C.c_uint32()
    t0 = time.time()
    rc = lib.pil2gl_debug_jit_compile(C.byref(prog), C.byref(c), C.byref(nbytes), C.byref(fused))
    assert rc == 0, lib.pil2gl_last_error()
    assert nbytes.value > 1000
    assert fused.value == 2 * 10 + 3          # every constraint became one lazy multiply-accumulate term
    assert time.time() - t0 < 120
    # the form long programs take (modular multiplications called, not inlined: the kernel must fit the instruction cache)
    inlined = nbytes.value
    os.environ["PIL2GL_EXPR_MULCALL"] = "1"
    try:
        rc = lib.pil2gl_debug_jit_compile(C.byref(prog), C.byref(c), C.byref(nbytes), C.byref(fused))
    finally:
        del os.environ["PIL2GL_EXPR_MULCALL"]
    assert rc == 0, lib.pil2gl_last_error()
    assert 1000 < nbytes.value < inlined


def test_no_early_clobber_overlap_in_bn128_isa(tmp_path):
    """hipcc's coalescer has been seen (round 5) to give an early-clobber asm output the register of an input it is later selected
    against -- `v_cndmask_b32 v8, v8, v8, vcc` in the earlier bn::cond_sub_r when its result was copied back over its input inside a loop: both
    outcomes of the select are then the difference, silently wrong for every value below r.  bn::cond_sub_r works in place since round 6
    (no select is left in it); this scan stays as a backstop for any select whose two sources are the same register, in the ISA of the
    files that carry such asm statements (no GPU needed: hipcc cross-compiles).
    The same ISA carries bnm::mfma_first's two hand-written v_mfma_i32_32x32x32_i8 (accumulators started at 2.0), which the compiler cannot
    see to pad: the s_nop after each pair must give at least the wait states hipcc itself puts between that instruction and a vector
    read of its result -- read here from a one-instruction kernel compiled by the same hipcc, not written down."""
    import re
    import shutil
    import subprocess
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    probe = tmp_path / "one_mfma.hip"
    probe.write_text("#include <hip/hip_runtime.h>\n"
                     "typedef int v4i __attribute__((ext_vector_type(4)));\n"
                     "typedef int v16i __attribute__((ext_vector_type(16)));\n"
                     "__global__ void one_mfma(const v4i *a, const v4i *b, int *out) {\n"
                     "    const v4i x = a[threadIdx.x], y = b[threadIdx.x];\n"
                     "    const v16i c = __builtin_amdgcn_mfma_i32_32x32x32_i8(x, y, v16i{}, 0, 0, 0);\n"
                     "    out[threadIdx.x] = c[0] ^ 0x55;\n"
                     "}\n")
    subprocess.check_call([hipcc, "-O3", "--offload-arch=gfx950", "-S", "--cuda-device-only", str(probe), "-o", str(tmp_path / "one_mfma.s")],
                          stderr=subprocess.DEVNULL)
    lines = [l.split(";")[0].strip() for l in (tmp_path / "one_mfma.s").read_text().splitlines()]
    lines = [l for l in lines if l and not l.startswith(".") and not l.endswith(":")]
    at = next(i for i, l in enumerate(lines) if l.startswith("v_mfma_i32_32x32x32_i8 "))
    lo, hi = map(int, re.match(r"v_mfma_i32_32x32x32_i8 v\[(\d+):(\d+)\]", lines[at]).groups())
    need = 0                                         # wait states from the result's write to its first reader
    for l in lines[at + 1:]:
        nop = re.match(r"s_nop (\d+)$", l)
        regs = [(int(m[0] or m[2]), int(m[1] or m[2])) for m in re.findall(r"\bv(?:\[(\d+):(\d+)\]|(\d+)\b)", l)]
        if nop:
            need += int(nop.group(1)) + 1
        elif any(a <= hi and b >= lo for a, b in regs):
            break
        else:
            need += 1
    assert need >= 1, "no pad found after the probe's matrix instruction"
    pkg = os.path.join(ROOT, "pil2-stark-js_amd")
    for src in ("bn128.hip",):
        out = tmp_path / (src + ".s")
        subprocess.check_call([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "-Wno-unused-function", "-ffp-contract=off", "-I" + os.path.join(pkg, "build"),
                               "-S", "--cuda-device-only", os.path.join(pkg, "csrc", src), "-o", str(out)], stderr=subprocess.DEVNULL)
        isa = out.read_text()
        bad = re.findall(r"v_cndmask_b32(?:_e32|_e64)? v\d+, (v\d+), \1, (?:vcc|s\[\d+:\d+\])", isa)     # ANY select whose two sources are one register
        assert not bad, "%s: a select between a register and itself (%d sites)" % (src, len(bad))
        pads = re.findall(r"v_mfma_i32_32x32x32_i8 [^\n]*, 2\.0\n\s*v_mfma_i32_32x32x32_i8 [^\n]*, 2\.0\n\s*s_nop (\d+)", isa)
        n_inline = len(re.findall(r"v_mfma_i32_32x32x32_i8 [^\n]*, 2\.0\n", isa))
        assert pads and 2 * len(pads) == n_inline, "%s: %d matrix instructions on the inline bias, %d padded pairs" % (src, n_inline, len(pads))
        short = [int(n) for n in pads if int(n) + 1 < need]
        assert not short, "%s: %d pairs padded with s_nop %d, hipcc pads %d wait states" % (src, len(short), min(short), need)


def test_bn254_sbox_columns_model_and_generated_file():
    """the S-box's seventeen columns per product (csrc/bn_field29_columns.inc): the generator's integer model of exactly those columns -- every
    column sum below 2^64, result = a b / 2^261 mod r below 2^252 + r -- on random and edge operands, and the checked-in file is what the
    generator writes (build() runs the same check)"""
    import subprocess
    import sys
    subprocess.check_call([sys.executable, os.path.join(ROOT, "pil2-stark-js_amd", "csrc", "gen_bn29_columns.py"), "--check"])

