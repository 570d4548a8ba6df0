// Stand-alone driver of the BN254 Fr evaluator's host-only half (csrc/bn_expr_plan.h: the checks made before any device call and the
// launch geometry), built by tests/test_bn128_expr_cpu.py with -fsanitize=address,undefined.  Prints one JSON object.
#include <stdio.h>
#include <string.h>
#include <vector>
#include "bn_expr_plan.h"

static glx_ref ref(int kind, uint32_t index, uint16_t section = 0, int32_t prime = 0, uint8_t dim = 1) {
    glx_ref r; memset(&r, 0, sizeof r); r.kind = (uint8_t)kind; r.dim = dim; r.section = section; r.prime = prime; r.index = index; return r;
}
static glx_op op(uint32_t o, glx_ref d, glx_ref a, glx_ref b) { glx_op x; memset(&x, 0, sizeof x); x.op = o; x.dest = d; x.src[0] = a; x.src[1] = b; return x; }

static void verdict(const char *name, std::vector<glx_op> ops, uint32_t nBits, uint32_t primeShift, bool nullFirst, bool last) {
    std::vector<uint64_t> a(4 * 2 * 8), b(4 * 8), sc(4);
    bnx_section secs[2] = { { nullFirst ? nullptr : a.data(), 2 }, { b.data(), 1 } };
    bnx_ctx ctx = { nBits, primeShift, 2, 1, secs, sc.data() };
    glx_program prog = { (uint32_t)ops.size(), 1, ops.data() };
    char err[160] = "";
    const bool ok = bnx::validate(&prog, &ctx, err, sizeof err);
    printf("\"%s\": \"%s\"%s", name, ok ? "" : err, last ? "" : ", ");
}

int main() {
    printf("{\"geometry\": {");
    const uint32_t bits[3] = { 0, 8, 20 };
    bool first = true;
    for (uint32_t nb : bits)
        for (uint32_t k = 0; k <= 40; k++) {
            const bnx::Geometry g = bnx::geometry(k, nb);
            printf("%s\"%u/%u\": [%u, %u, %u, %u, %llu, %llu]", first ? "" : ", ", k, nb, g.form, g.threads, g.blocks, g.ldsBytes,
                   (unsigned long long)g.lanesPerLaunch, (unsigned long long)g.tmpBytes);
            first = false;
        }
    printf("}, \"verdicts\": {");
    const glx_ref t0 = ref(GLX_TMP, 0), s0 = ref(GLX_SCALAR, 0);
    verdict("good", { op(GLX_OP_MUL, t0, ref(GLX_SEC, 0, 0, 1), s0), op(GLX_OP_ADD, ref(GLX_SEC, 0, 1), t0, ref(GLX_SEC, 1, 0)) }, 3, 0, false, false);
    verdict("in place", { op(GLX_OP_MUL, ref(GLX_SEC, 1, 0), ref(GLX_SEC, 1, 0), ref(GLX_SEC, 1, 0)) }, 3, 0, false, false);
    verdict("dim", { op(GLX_OP_COPY, t0, ref(GLX_SEC, 0, 0, 0, 3), s0) }, 3, 0, false, false);
    verdict("race", { op(GLX_OP_MUL, ref(GLX_SEC, 1, 0), ref(GLX_SEC, 1, 0, -1), s0) }, 3, 0, false, false);
    verdict("two offsets", { op(GLX_OP_COPY, ref(GLX_SEC, 0, 1, 1), s0, s0), op(GLX_OP_COPY, ref(GLX_SEC, 0, 1, 2), s0, s0) }, 3, 0, false, false);
    verdict("overflow", { op(GLX_OP_COPY, t0, ref(GLX_SEC, 0, 0, 1 << 20), s0) }, 28, 12, false, false);
    verdict("null", { op(GLX_OP_COPY, t0, ref(GLX_SEC, 0, 0), s0) }, 3, 0, true, true);
    printf("}}\n");
    return 0;
}
