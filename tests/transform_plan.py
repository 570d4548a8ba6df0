"""Which kernels a transform launches, for tests that claim one: pil2gl_debug_plan_transform (csrc/ntt.hip) returns the launches
fft / ifft / interpolate / the extension from coefficients make for a shape -- the planner exactly as ntt_launch / lde_launch run it,
under whatever test hooks (PIL2GL_NTT_KMAX, PIL2GL_NTT_GENERIC, PIL2GL_LDE_WIDEFWD) the environment holds.  Host only: no device."""
import collections
import ctypes as C

OPS = ("fft", "ifft", "interpolate", "extend_coefs")        # PIL2GL_PLAN_* of include/pil2gl.h
KINDS = "ifdm"                                              # inverse DIF pass, forward DIF pass, DIT pass, mid kernel
WORDS = 14                                                  # PIL2GL_PLAN_LAUNCH_WORDS
Launch = collections.namedtuple("Launch", "kind lo k cols groups chunks bx by fixed ept lds blocks scatter canon")


def plan(op, n_bits, n_pols, ext_bits=0, coset_count=0):
    """the launches of one call, in order; coset_count 0 = the whole extension"""
    from pil2gl import _lib
    lib = _lib.load()
    buf = (C.c_uint32 * (WORDS * 64))()
    n = C.c_uint32()
    rc = lib.pil2gl_debug_plan_transform(OPS.index(op), n_bits, n_pols, n_bits + ext_bits, coset_count, buf, 64, C.byref(n))
    assert rc == 0, lib.pil2gl_last_error()
    return [Launch(KINDS[buf[WORDS * i]], *buf[WORDS * i + 1:WORDS * (i + 1)]) for i in range(n.value)]


def line(launches):
    """a plan as tests/golden/transform_plans.txt.gz writes it"""
    return " ; ".join("%s %s" % (l.kind, " ".join(str(v) for v in l[1:])) for l in launches)


def fixed_instances(launches):
    """the launches that run a fixed-geometry instance (ntt_pass_kernel<.., 8, 15|16>, lde_mid_kernel<16, 15|16>)"""
    return [l for l in launches if l.fixed]


def balanced(n_bits, kmax):
    """the largest pass of n_bits index bits cut into ceil(n_bits / kmax) nearly equal passes: the planner balances, so a forced
    maximum of kmax stages is reached exactly only where kmax divides n_bits or n_bits <= kmax"""
    passes = -(-n_bits // kmax)
    return -(-n_bits // passes)


def check_hooks(env, ops, n_bits, n_pols, ext_bits=0, coset_count=0):
    """what a test that sets one of the hooks claims, read from the plans of `ops` under the CURRENT environment (env: the hooks the
    test has just set, name -> value):
      PIL2GL_NTT_GENERIC=1: no fixed-geometry instance; =0: an extension holds one (its mid kernel at least), and so does fft / ifft
        where its balanced split has 8-stage passes (2^16 rows; 2^17 x 100 runs 6, 6, 5 on the any-geometry instances);
      PIL2GL_NTT_KMAX=K: the largest planned pass is the balanced split's, balanced(n_bits, K) <= K;
      PIL2GL_LDE_WIDEFWD: a narrow matrix (under 15 columns) whose extension is wide (16 columns and more) plans its forward side -- mid
        kernel and DIT passes -- within 8 stages with 1 and within 7 with 0: the largest is balanced(n_bits, 8), e.g. 8 at 2^15 and 2^16
        rows, against balanced(n_bits, 7), 5 and 6 there (2^17 rows: 6 either way); a narrow extension stays within 7 either way."""
    for op in ops:
        eb, cc = (ext_bits, coset_count) if op in ("interpolate", "extend_coefs") else (0, 0)
        p = plan(op, n_bits, n_pols, eb, cc)
        assert p or n_bits == 0
        if "PIL2GL_NTT_GENERIC" in env:
            if env["PIL2GL_NTT_GENERIC"] == "1":
                assert not fixed_instances(p), (op, p)
            elif eb or op in ("interpolate", "extend_coefs") or balanced(n_bits, 8) == 8:
                assert fixed_instances(p), (op, p)
        if "PIL2GL_NTT_KMAX" in env and p:
            assert max(l.k for l in p) == balanced(n_bits, int(env["PIL2GL_NTT_KMAX"])), (op, p)
        if "PIL2GL_LDE_WIDEFWD" in env and eb:
            fwd = max(l.k for l in p if l.kind in "md")
            cosets = coset_count or 1 << eb
            if n_pols < 15:
                assert fwd == balanced(n_bits, 8 if env["PIL2GL_LDE_WIDEFWD"] == "1" and n_pols * cosets >= 16 else 7), (op, p)
