// Host-side shared declarations of libpil2gl (not part of the public ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <mutex>
#include "../../include/pil2gl.h"

namespace pil2gl {

typedef uint64_t u64;
typedef uint32_t u32;

// largest transform (rows = 2^this) the NTT / LDE / FRI-fold entry points accept on one device
#define PIL2GL_MAX_NTT_BITS 30

// error plumbing ------------------------------------------------------------
int  fail(int code, const char *fmt, ...);          // records the message, returns code
int  hip_fail(hipError_t e, const char *what);      // -> PIL2GL_EHIP
#define HIP_TRY(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return ::pil2gl::hip_fail(e_, #expr); } while (0)
#define P2_TRY(expr)  do { int rc_ = (expr); if (rc_ != PIL2GL_OK) return rc_; } while (0)
#define KERNEL_CHECK() HIP_TRY(hipGetLastError())

int ensure_init();                                   // pil2gl_init(current device) on first use
std::recursive_mutex &runtime_lock();                // guards the process-global runtime state (tables, scratch, kernel cache)
void jit_clear();                                    // unloads the run-time compiled expression kernels (expr.hip)
void hostleg_shutdown();                             // destroys the copy stream, its events and the pinned file chunks (hostleg.hip)

// host-side Goldilocks (table construction and scalar parameters only) ---------
u64 h_mul(u64 a, u64 b);
u64 h_add(u64 a, u64 b);
u64 h_sub(u64 a, u64 b);
u64 h_pow(u64 a, u64 e);
u64 h_inv(u64 a);
u64 h_root(u32 bits);                                // F.w[bits]
void h_e3_mul(const u64 a[3], const u64 b[3], u64 r[3]);

// device tables -------------------------------------------------------------------
// pow256 layout: T[t*256 + i] = g^(i << (8t)), t = 0..3  (any 32-bit exponent in 3 multiplications)
struct Tables {
    const u64 *powW;      // g = w[32]   (forward roots of unity)
    const u64 *powWi;     // g = w[32]^-1
    const u64 *pow7;      // g = 7       (coset shift)
    const u64 *pow7i;     // g = 7^-1
    const u64 *tw1024;    // tw1024[j] = w[10]^j, j < 1024 (tile twiddles of the NTT passes)
    const u64 *tw1024i;   // w[10]^-j
};
const Tables &tables();

// scratch (grown on demand, kept across calls): one slot per owner, so that no two buffers that are live at once share one
enum ScratchSlot : u32 {
    SCR_NTT_TMP = 0,          // ntt.hip: the second buffer of a transform of more than one pass
    SCR_FRI_COEF = 1,         // fri.hip: a fold's coefficients (fri_fold, fri_verify_fold); the FRI polynomial on its coset before the extension
    SCR_FRI_TABLE = 2,        // fri.hip upload_small: the small host-made table of one helper call (zerofiers, shifts, Lagrange powers)
    SCR_EVALS = 3,            // fri.hip compute_evals: the blocks' partial sums
    SCR_EXPR_PROGRAM = 4,     // expr.hip: the device form of a program (ops, scalar pool, limbs)
    SCR_EXPR_TMP = 5,         // expr.hip: the interpreter's temporaries when they do not fit LDS
    SCR_GROUP_PROOFS = 6,     // merkle.hip, bn128.hip: the openings group_proofs gathers / roots_from_group_proofs walks -- shared: none of them calls another
    SCR_DOT = 7,              // dot.hip: tables and partial sums of the extension-weighted sums
    SCR_HINT_TMP = 8,         // hints.hip: the running sums / products' per-element work
    SCR_HINT_TOTALS = 9,      // hints.hip: their blocks' totals
    SCR_HINT_WORK = 10,       // hints.hip h1h2: hash table, counts, starts, totals
    SCR_STAGE = 11,           // Stage below: device copies of the small host-pointer calls
    SCR_HOST_NTT_IN = 12,     // ntt.hip host_wrap: device copies of the host-pointer transforms (a size policy of its own, documented there)
    SCR_HOST_NTT_OUT = 13,
    SCR_Q_A = 14,             // fri.hip: the quotient stage (q, then its coefficients in SCR_Q_B) and the FRI polynomial (x / (x - xi) tables, accumulators)
    SCR_Q_B = 15,
    SCR_CLOCK_PROBE = 16,     // merkle.hip pil2gl_selftest_clock
    SCR_BN_NTT_TMP = 17,      // bn_ntt.hip: the working buffer of a BN254 transform of more than one sweep
    SCR_BN_MSM = 18,          // bn_msm.hip: histogram, cursors, point lists, buckets and reduction levels of a G1 MSM (layout: bnp::bn_msm_plan)
    SCR_BN_EXPR = 19,         // bn_expr.hip: the first-non-zero search's cell, the device form of a program (ops, scalar pool), the temporaries that do not fit LDS
    SCR_BN_POLY = 20,         // bn_poly.hip: the levels' multipliers, then the segment values of every level and point (layout: bnpoly::plan)
    SCR_BN_SCAN = 21,         // bn_scan.hip: the levels' segment totals and prefixes, then the level-0 prefixes of an inversion in place (layout: bnscan::plan)
    SCR_BN_H1H2 = 22,         // bn_h1h2.hip: hash table, counts / group starts, chunk totals, the missing cell (layout: bnh1h2::plan)
    SCR_BN_POLYMUL = 23,      // bn_polymul.hip: the cell of poly_degree's atomic maximum (poly_fma has no working buffer)
    SCR_WTNS = 24,            // wtns_exec.hip: the cell of a checked gather's atomic minimum, the first sMap index that names no signal
    N_SCRATCH
};
int scratch(ScratchSlot slot, u64 nWords, u64 **out);

// Device staging for the host-pointer entry points: reserves nWords, hands out consecutive sub-ranges (filled from host memory or left for
// the kernels to write), copies results back and releases on scope exit.  Small requests (<= 16 MB) come from a persistent slot -- a
// hipMalloc / hipFree pair per call costs a device synchronisation each, which dominated the transcript's single permutations -- larger ones
// are allocated and released per call.  The first failure (initialisation, allocation, a copy) stays in rc(); after it put / take return
// nullptr and get returns it.
class Stage {
public:
    explicit Stage(u64 nWords);                       // includes ensure_init()
    ~Stage();
    Stage(const Stage &) = delete; Stage &operator=(const Stage &) = delete;
    int rc() const { return rc_; }
    u64 *take(u64 n);                                 // the next n words, as they are
    const u64 *put(const u64 *host, u64 n);           // the next n words, copied from host; n == 0: nullptr (an absent input)
    int get(u64 *host, const u64 *dev, u64 n);        // device -> host
private:
    u64 *d_ = nullptr, used_ = 0, cap_ = 0;
    bool owned_ = false;
    int rc_;
};

hipStream_t as_stream(void *s);

// internal launchers shared between translation units --------------------------------------
int ntt_launch(const u64 *src, u64 nPols, u32 nBits, u64 *dst, bool inverse, hipStream_t st);
int lde_launch(const u64 *src, u64 nPols, u32 nBits, u64 *dst, u32 nBitsExt, hipStream_t st, u32 cosetBegin, u32 cosetCount, u64 *work, bool unitShift, bool coefIn = false);

}  // namespace pil2gl
