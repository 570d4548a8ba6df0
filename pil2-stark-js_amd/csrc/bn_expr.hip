// Expression evaluator over the BN254 scalar field Fr, gfx950: the device twin of the row loop the fflonk final prover runs between its
// commitments (src/prover/prover.js:212-219 -> prover_helpers.js:31-72 calculateExps, :83-107 compileCode, :109-259 setRef / getRef /
// evalMap, fflonk_prover_worker.js:5-41) with ctx.F = curve.Fr.  Op-list encoding: include/pil2gl_expr.h; elements and context:
// include/pil2gl_bn_expr.h.  With it a stage runs ifft -> blind -> evaluate -> fft -> msm without a copy to the host.
//
// One lane evaluates one row; the program is wave-uniform.  An element is 32 bytes of Montgomery words and stays in that form: add, sub
// and mul are bn_field.cuh's fr_add / fr_sub / fr_mul, canonical in and out.  The host value-numbers the temporaries and renumbers them
// by live range (expr.hip's passes 1 and 3, through pil2gl_debug_compact_program; its Horner fusion is the Goldilocks lazy form and has
// no meaning here).  The temporaries live in a [slot][half][lane] array of 16-byte halves, as bn_ntt.hip moves elements, so that slot
// numbers -- data of the program -- index memory and a wave's access to a slot is contiguous: in LDS when the slots fit a workgroup of
// 256, 128 or 64 lanes, in a global working buffer (SCR_BN_EXPR) otherwise.  bnx::geometry (bn_expr_plan.h) decides, and
// pil2gl_debug_bn128_plan_program reports what it decided.
#include "common.h"
#include "bn_elem.cuh"
#include "bn_expr_plan.h"
#include <vector>
#include <string.h>

using namespace pil2gl;

namespace {

struct DevRef { u32 kind, section; int32_t rowOff; u32 index; };      // rowOff: prime << primeShift, already scaled
struct DevOp { u32 op, pad_; DevRef dest, src[2]; };                  // 56 bytes

struct DevCtx {
    const DevOp *__restrict__ ops; u32 nOps;
    u32 nBits;
    const uint4 *__restrict__ scalars;
    uint4 *secPtr[PIL2GL_BNX_MAX_SECTIONS];
    u32 secWidth[PIL2GL_BNX_MAX_SECTIONS];
};

constexpr u64 HEADER_WORDS = 8;                      // SCR_BN_EXPR starts with the first-non-zero search's cell

// element (row + rowOff) mod 2^nBits, column index of a section   (prover_helpers.js:220-233)
__device__ __forceinline__ uint4 *cell(const DevRef &r, const DevCtx &c, u64 row) {
    const u64 rr = (row + (u64)(int64_t)r.rowOff) & ((1ull << c.nBits) - 1);
    return c.secPtr[r.section] + 2 * (rr * c.secWidth[r.section] + r.index);
}
// Temporaries: slot s, half h of a lane at T[(2 s + h) * stride].  In the LDS form T is an LDS pointer by its type, so that hipcc keeps
// these accesses apart from the sections' (it otherwise folds the three operand classes into flat dword loads through one pointer).
typedef u32 v4u __attribute__((ext_vector_type(4)));             // a plain vector: HIP's uint4 class has no members for a qualified address space
typedef __attribute__((address_space(3))) v4u lds_v4u;
template <bool LDS_TMP> struct TmpPtr { typedef v4u *type; };
template <> struct TmpPtr<true> { typedef lds_v4u *type; };

template <bool LDS_TMP>
__device__ __forceinline__ void load_ref(const DevRef &r, const DevCtx &c, u64 row, typename TmpPtr<LDS_TMP>::type T, u32 stride, u32 x[8]) {
    if (r.kind == GLX_TMP) {
        const size_t e = (size_t)(2 * r.index) * stride;
        const v4u a = T[e], b = T[e + stride];
        x[0] = a.x; x[1] = a.y; x[2] = a.z; x[3] = a.w; x[4] = b.x; x[5] = b.y; x[6] = b.z; x[7] = b.w;
        return;
    }
    const uint4 *p = r.kind == GLX_SCALAR ? c.scalars + 2 * (size_t)r.index : cell(r, c, row);
    bn::ld_elem(p, x);
}

template <bool LDS_TMP>
__global__ void __launch_bounds__(256) bn_eval_kernel(DevCtx c, uint4 *gtmp) {
    extern __shared__ __attribute__((aligned(16))) v4u lds_tmp[];
    typename TmpPtr<LDS_TMP>::type T; u32 stride;
    if constexpr (LDS_TMP) { T = (lds_v4u *)lds_tmp + threadIdx.x; stride = blockDim.x; }
    else { T = (v4u *)gtmp + (size_t)blockIdx.x * blockDim.x + threadIdx.x; stride = gridDim.x * blockDim.x; }
    const u64 nRows = 1ull << c.nBits;
    for (u64 row = (u64)blockIdx.x * blockDim.x + threadIdx.x; row < nRows; row += (u64)gridDim.x * blockDim.x) {
        for (u32 k = 0; k < c.nOps; k++) {
            const DevOp op = c.ops[k];
            u32 a[8], b[8];
            load_ref<LDS_TMP>(op.src[0], c, row, T, stride, a);
            if (op.op != GLX_OP_COPY) load_ref<LDS_TMP>(op.src[1], c, row, T, stride, b);
            if (op.op == GLX_OP_ADD) bn::fr_add(a, b);
            else if (op.op == GLX_OP_SUB) bn::fr_sub(a, b);
            else if (op.op == GLX_OP_MUL) bn::fr_mul(a, a, b);
            if (op.dest.kind == GLX_TMP) {
                const size_t e = (size_t)(2 * op.dest.index) * stride;
                T[e] = (v4u){ a[0], a[1], a[2], a[3] }; T[e + stride] = (v4u){ a[4], a[5], a[6], a[7] };
            } else {
                bn::st_elem(cell(op.dest, c, row), a);
            }
        }
    }
}

// the smallest row of [first, last) whose element is not zero: one atomic minimum per wave that saw one
__global__ void __launch_bounds__(256) bn_first_nonzero_kernel(const uint4 *__restrict__ col, u64 width, u64 first, u64 last,
                                                               unsigned long long *__restrict__ best) {
    const u64 r = first + (u64)blockIdx.x * blockDim.x + threadIdx.x;
    bool nz = false;
    if (r < last) {
        const uint4 a = col[2 * r * width], b = col[2 * r * width + 1];
        nz = !bn::is_zero(a, b);
    }
    const u64 mask = __ballot(nz);
    if (mask && (threadIdx.x & 63) == 0) atomicMin(best, (unsigned long long)(r + __builtin_ctzll(mask)));
}

struct Plan {
    std::vector<glx_op> ops;                         // after value numbering and slot allocation
    u32 nSlots = 0;
    bnx::Geometry geo;
};

// the program as the kernel runs it, with every check that needs no device
int plan_program(const glx_program *prog, const bnx_ctx *ctx, Plan &plan) {
    char err[160];
    if (!bnx::validate(prog, ctx, err, sizeof err)) return fail(PIL2GL_EINVAL, "%s", err);
    plan.ops.clear();
    if (prog->nOps) {
        plan.ops.resize(2ull * prog->nOps + 16);
        u32 info[2] = { 0, 0 };
        P2_TRY(pil2gl_debug_compact_program(prog, plan.ops.data(), info));
        plan.nSlots = info[0];
        plan.ops.resize(info[1]);
    }
    if (plan.nSlots > bnx::MAX_SLOTS) return fail(PIL2GL_EINVAL, "%u live temporaries: at most %u", plan.nSlots, bnx::MAX_SLOTS);
    plan.geo = bnx::geometry(plan.nSlots, ctx->nBits);
    return PIL2GL_OK;
}

int launch(const Plan &plan, const bnx_ctx *ctx, const bnx_section *sections, hipStream_t st) {
    if (plan.ops.empty()) return PIL2GL_OK;
    const bnx::Geometry &g = plan.geo;
    // device form of the program and the scalar pool, one host buffer and one copy
    const u64 opsWords = ((u64)plan.ops.size() * sizeof(DevOp) + 15) / 16 * 2, scalarWords = 4ull * ctx->nScalars;
    std::vector<u64> host(opsWords + scalarWords);
    DevOp *dops = (DevOp *)host.data();
    for (size_t k = 0; k < plan.ops.size(); k++) {
        auto cv = [&](const glx_ref &r) { DevRef d; d.kind = r.kind; d.section = r.section; d.rowOff = (int32_t)((int64_t)r.prime * ((int64_t)1 << ctx->primeShift)); d.index = r.index; return d; };
        dops[k].op = plan.ops[k].op; dops[k].pad_ = 0;
        dops[k].dest = cv(plan.ops[k].dest); dops[k].src[0] = cv(plan.ops[k].src[0]); dops[k].src[1] = cv(plan.ops[k].src[1]);
    }
    if (scalarWords) memcpy(host.data() + opsWords, ctx->scalars, scalarWords * 8);
    const u64 tmpWords = g.tmpBytes / 8;
    u64 *d;
    P2_TRY(scratch(SCR_BN_EXPR, HEADER_WORDS + host.size() + tmpWords, &d));
    // a pageable-host async copy is staged by the runtime before it returns, so `host` may go out of scope; the kernel is only enqueued
    HIP_TRY(hipMemcpyAsync(d + HEADER_WORDS, host.data(), host.size() * 8, hipMemcpyHostToDevice, st));
    DevCtx c;
    c.ops = (const DevOp *)(d + HEADER_WORDS); c.nOps = (u32)plan.ops.size();
    c.nBits = ctx->nBits;
    c.scalars = (const uint4 *)(d + HEADER_WORDS + opsWords);
    for (u32 i = 0; i < PIL2GL_BNX_MAX_SECTIONS; i++) {
        c.secPtr[i] = i < ctx->nSections ? (uint4 *)sections[i].ptr : nullptr;
        c.secWidth[i] = i < ctx->nSections ? (u32)sections[i].width : 0;
    }
    if (g.form == 0) {
        bn_eval_kernel<true><<<g.blocks, g.threads, g.ldsBytes, st>>>(c, nullptr);
    } else {
        bn_eval_kernel<false><<<g.blocks, g.threads, 0, st>>>(c, (uint4 *)(d + HEADER_WORDS + host.size()));
    }
    KERNEL_CHECK();
    return PIL2GL_OK;
}

}  // namespace

extern "C" {

int pil2gl_debug_bn128_plan_program(const glx_program *prog, const bnx_ctx *ctx, uint32_t *outInfo) {
    if (!outInfo) return fail(PIL2GL_EINVAL, "null argument");
    Plan plan;
    P2_TRY(plan_program(prog, ctx, plan));
    outInfo[0] = plan.nSlots; outInfo[1] = (uint32_t)plan.ops.size(); outInfo[2] = plan.geo.form;
    outInfo[3] = bnx::LDS_SLOT_LIMIT; outInfo[4] = (uint32_t)plan.geo.lanesPerLaunch; outInfo[5] = plan.geo.threads;
    return PIL2GL_OK;
}

int pil2gl_bn128_eval_program_dev(const glx_program *prog, const bnx_ctx *ctx, void *stream) {
    Plan plan;
    P2_TRY(plan_program(prog, ctx, plan));
    for (u32 i = 0; i < ctx->nSections; i++)
        if ((uintptr_t)ctx->sections[i].ptr & 15) return fail(PIL2GL_EINVAL, "section %u must be 16-byte aligned", i);
    P2_TRY(ensure_init());
    return launch(plan, ctx, ctx->sections, as_stream(stream));
}

int pil2gl_bn128_eval_program(const glx_program *prog, const bnx_ctx *ctx) {
    Plan plan;
    P2_TRY(plan_program(prog, ctx, plan));
    if (plan.ops.empty()) return PIL2GL_OK;
    // only the sections the program names travel; the ones it writes come back
    std::vector<char> used(ctx->nSections, 0), written(ctx->nSections, 0);
    for (u32 k = 0; k < prog->nOps; k++) {
        const glx_op &o = prog->ops[k];
        for (int s = 0; s < (o.op == GLX_OP_COPY ? 1 : 2); s++) if (o.src[s].kind == GLX_SEC) used[o.src[s].section] = 1;
        if (o.dest.kind == GLX_SEC) used[o.dest.section] = written[o.dest.section] = 1;
    }
    const u64 rows = 1ull << ctx->nBits;
    u64 total = 0;
    for (u32 i = 0; i < ctx->nSections; i++) if (used[i]) total += rows * ctx->sections[i].width * 4;
    Stage s(total);
    P2_TRY(s.rc());
    std::vector<bnx_section> dev(ctx->nSections);
    for (u32 i = 0; i < ctx->nSections; i++) {
        dev[i].width = ctx->sections[i].width;
        dev[i].ptr = used[i] ? const_cast<u64 *>(s.put(ctx->sections[i].ptr, rows * dev[i].width * 4)) : nullptr;
    }
    P2_TRY(s.rc());
    P2_TRY(launch(plan, ctx, dev.data(), 0));
    for (u32 i = 0; i < ctx->nSections; i++) if (written[i]) P2_TRY(s.get(ctx->sections[i].ptr, dev[i].ptr, rows * dev[i].width * 4));
    return PIL2GL_OK;
}

int pil2gl_bn128_first_nonzero_row_dev(const uint64_t *col, uint64_t width, uint64_t column, uint64_t first, uint64_t last,
                                       uint64_t *hostRow, uint64_t *hostVal, void *stream) {
    if (!hostRow || !hostVal) return fail(PIL2GL_EINVAL, "null buffer");
    if (width == 0 || width >> 32 || column >= width) return fail(PIL2GL_EINVAL, "column %llu of a section %llu wide", (unsigned long long)column, (unsigned long long)width);
    if (last < first) return fail(PIL2GL_EINVAL, "empty range [%llu, %llu)", (unsigned long long)first, (unsigned long long)last);
    if (last > (1ull << bnx::MAX_BITS)) return fail(PIL2GL_EINVAL, "row %llu beyond 2^%u", (unsigned long long)last, bnx::MAX_BITS);
    if (last > first && !col) return fail(PIL2GL_EINVAL, "null buffer");
    if ((uintptr_t)col & 15) return fail(PIL2GL_EINVAL, "the section must be 16-byte aligned");
    *hostRow = ~0ull;
    for (int k = 0; k < 4; k++) hostVal[k] = 0;
    if (last == first) return PIL2GL_OK;
    P2_TRY(ensure_init());
    hipStream_t st = as_stream(stream);
    u64 *d;
    P2_TRY(scratch(SCR_BN_EXPR, HEADER_WORDS, &d));
    HIP_TRY(hipMemsetAsync(d, 0xff, 8, st));
    const u64 blocks = (last - first + 255) / 256;
    bn_first_nonzero_kernel<<<(unsigned)blocks, 256, 0, st>>>((const uint4 *)col + 2 * column, width, first, last, (unsigned long long *)d);
    KERNEL_CHECK();
    HIP_TRY(hipMemcpyAsync(hostRow, d, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (*hostRow != ~0ull) HIP_TRY(hipMemcpy(hostVal, col + 4 * (*hostRow * width + column), 32, hipMemcpyDeviceToHost));
    return PIL2GL_OK;
}

}  // extern "C"
