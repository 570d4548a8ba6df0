// The host -> HBM leg of libpil2gl: pinned host memory, asynchronous copies on a library-owned copy stream ordered against
// compute streams by events, the landing pass a freshly copied chunk gets (canonicity check, row widening), and the
// `.commit` / `.const` / `.consttree` file loaders that stream a file through two pinned chunks
// (src/witness/witnessCalculator.js:145-214, src/helpers/hash/merklehash/merklehash_p.js:228-278 of the reference).
#include "common.h"
#include <errno.h>
#include <fcntl.h>
#include <string.h>
#include <sys/stat.h>
#include <unistd.h>

namespace pil2gl {

static const u64 GL_P = 0xFFFFFFFF00000001ull;
static const u64 NO_BAD = ~0ull;
static const u64 DEFAULT_CHUNK_WORDS = 1ull << 25;      // 256 MB, the reference's MaxBuffSize (witnessCalculator.js:148)

// ---- the landing kernel ---------------------------------------------------------------------------------------------
// One read of every source word: the smallest flat SOURCE index (plus idxBase) of a word >= p goes to *firstBad, and the
// word goes to its place in dst (nowhere when the copy engine already put it there).  Forms, chosen by the host:
//   LAND_CHECK   srcCols == dstCols, src == dst: check only.  16-byte loads; the host peels a leading word when src is only
//                8-byte aligned and the odd last word, thread 0 takes both.
//   LAND_COPY    srcCols == dstCols, src != dst, both congruent mod 16: the same with 16-byte stores.
//   LAND_WIDE2   both widths even, both pointers 16-byte aligned: a row is a whole number of 16-byte pairs; pair j of dst row r
//                is pair j of src row r, or zeros from srcCols / 2 on.
//   LAND_WORD    anything else, one word at a time (odd widths, pointers of different alignment).
// (row, column) of a thread's element comes from one division before the loop; the grid stride then advances it by a
// precomputed (rows, columns) step, so the loop body has no division and every index is 64 bits wide.
enum { LAND_CHECK = 0, LAND_COPY = 1, LAND_WIDE2 = 2, LAND_WORD = 3 };

__device__ __forceinline__ u64 bad_at(u64 v, u64 idx, u64 best) { return (v >= GL_P && idx < best) ? idx : best; }

template <int MODE>
__global__ void __launch_bounds__(256) land_rows_kernel(const u64 *__restrict__ src, u64 srcCols, u64 *__restrict__ dst, u64 dstCols,
                                                        u64 nRows, u64 idxBase, u64 *firstBad) {
    const u64 tid = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    const u64 stride = (u64)gridDim.x * blockDim.x;
    u64 best = NO_BAD;
    if (MODE == LAND_CHECK || MODE == LAND_COPY) {
        const u64 nWords = nRows * srcCols;
        const u64 head = (nWords && ((uintptr_t)src & 8)) ? 1 : 0;
        const u64 nPairs = (nWords - head) >> 1;
        const ulonglong2 *s2 = (const ulonglong2 *)(src + head);
        ulonglong2 *d2 = (ulonglong2 *)(dst + head);
        for (u64 i = tid; i < nPairs; i += stride) {
            const ulonglong2 v = s2[i];
            best = bad_at(v.y, idxBase + head + 2 * i + 1, best);
            best = bad_at(v.x, idxBase + head + 2 * i, best);
            if (MODE == LAND_COPY) d2[i] = v;
        }
        if (tid == 0) {
            const u64 last = head + 2 * nPairs;
            if (last < nWords) { const u64 v = src[last]; best = bad_at(v, idxBase + last, best); if (MODE == LAND_COPY) dst[last] = v; }
            if (head) { const u64 v = src[0]; best = bad_at(v, idxBase, best); if (MODE == LAND_COPY) dst[0] = v; }
        }
    } else {
        // per: elements of a dst row (pairs or words); live: those that come from src
        const u64 unit = (MODE == LAND_WIDE2) ? 2 : 1;
        const u64 per = dstCols / unit, live = srcCols / unit;
        const u64 stepRows = stride / per, stepCols = stride % per;
        u64 r = tid / per, j = tid % per;
        while (r < nRows) {
            if (MODE == LAND_WIDE2) {
                ulonglong2 v = make_ulonglong2(0, 0);
                if (j < live) {
                    const u64 at = r * srcCols + 2 * j;
                    v = *(const ulonglong2 *)(src + at);
                    best = bad_at(v.y, idxBase + at + 1, best);
                    best = bad_at(v.x, idxBase + at, best);
                }
                *(ulonglong2 *)(dst + r * dstCols + 2 * j) = v;
            } else {
                u64 v = 0;
                if (j < live) { const u64 at = r * srcCols + j; v = src[at]; best = bad_at(v, idxBase + at, best); }
                dst[r * dstCols + j] = v;
            }
            r += stepRows; j += stepCols;
            if (j >= per) { j -= per; r++; }
        }
    }
    if (!firstBad) return;
    // one atomic per workgroup that saw a bad word: lanes -> wave by shuffles, the four waves through 32 bytes of LDS
    for (int o = 32; o > 0; o >>= 1) { const u64 other = __shfl_xor(best, o, 64); best = other < best ? other : best; }
    __shared__ u64 waveBest[4];
    if ((threadIdx.x & 63) == 0) waveBest[threadIdx.x >> 6] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; w++) best = waveBest[w] < best ? waveBest[w] : best;
        if (best != NO_BAD) atomicMin((unsigned long long *)firstBad, (unsigned long long)best);
    }
}

// ---- copy stream, events, pinned chunks (created on first use, destroyed by pil2gl_shutdown) ---------------------------
static hipStream_t g_copy = nullptr;
static hipEvent_t g_ev_after = nullptr, g_ev_fence = nullptr, g_ev_chunk[2] = { nullptr, nullptr };
static u64 *g_pinned[2] = { nullptr, nullptr };        // the two host chunks a file streams through
static u64 *g_stage[2] = { nullptr, nullptr };         // their device twins, for rows that are widened on the way
static u64 g_pinned_words = 0, g_stage_words = 0;
static u64 *g_bad_dev = nullptr, *g_bad_host = nullptr;
static int g_cus = 0;

static int copy_ready() {
    P2_TRY(ensure_init());
    if (g_copy) return PIL2GL_OK;
    // non-blocking: a blocking stream would serialise with the NULL stream every host-pointer entry point and Node use
    HIP_TRY(hipStreamCreateWithFlags(&g_copy, hipStreamNonBlocking));
    HIP_TRY(hipEventCreateWithFlags(&g_ev_after, hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&g_ev_fence, hipEventDisableTiming));
    for (int k = 0; k < 2; k++) HIP_TRY(hipEventCreateWithFlags(&g_ev_chunk[k], hipEventDisableTiming));
    HIP_TRY(hipMalloc((void **)&g_bad_dev, 8));
    HIP_TRY(hipHostMalloc((void **)&g_bad_host, 8, hipHostMallocDefault));
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    HIP_TRY(hipDeviceGetAttribute(&g_cus, hipDeviceAttributeMultiprocessorCount, dev));
    if (g_cus <= 0) g_cus = 256;
    return PIL2GL_OK;
}

static void free_chunks() {
    for (int k = 0; k < 2; k++) {
        if (g_pinned[k]) (void)hipHostFree(g_pinned[k]);
        if (g_stage[k]) (void)hipFree(g_stage[k]);
        g_pinned[k] = g_stage[k] = nullptr;
    }
    g_pinned_words = g_stage_words = 0;
}

void hostleg_shutdown() {
    if (g_copy) (void)hipStreamSynchronize(g_copy);
    free_chunks();
    if (g_bad_dev) (void)hipFree(g_bad_dev);
    if (g_bad_host) (void)hipHostFree(g_bad_host);
    g_bad_dev = g_bad_host = nullptr;
    for (hipEvent_t *e : { &g_ev_after, &g_ev_fence, &g_ev_chunk[0], &g_ev_chunk[1] }) { if (*e) (void)hipEventDestroy(*e); *e = nullptr; }
    if (g_copy) (void)hipStreamDestroy(g_copy);
    g_copy = nullptr;
}

static int chunks_ready(u64 chunkWords, bool withStage) {
    if (g_pinned_words != chunkWords) {
        if (g_copy) HIP_TRY(hipStreamSynchronize(g_copy));
        free_chunks();
        for (int k = 0; k < 2; k++) HIP_TRY(hipHostMalloc((void **)&g_pinned[k], chunkWords * 8, hipHostMallocDefault));
        g_pinned_words = chunkWords;
    }
    if (withStage && g_stage_words != chunkWords) {
        for (int k = 0; k < 2; k++) HIP_TRY(hipMalloc((void **)&g_stage[k], chunkWords * 8));
        g_stage_words = chunkWords;
    }
    return PIL2GL_OK;
}

// pinned (hipHostMalloc) or registered (hipHostRegister) at both ends of the range; pageable memory would turn the copy into
// a synchronous staged one without a word.  The runtime reports no extent for registered memory, so the two ends are what is
// checked (the header says so): a range that leaves one pinned block and ends in another is the caller's error.
static bool is_pinned(const void *p, u64 nBytes) {
    const char *ends[2] = { (const char *)p, (const char *)p + (nBytes ? nBytes - 1 : 0) };
    for (const char *q : ends) {
        hipPointerAttribute_t a;
        memset(&a, 0, sizeof a);
        if (hipPointerGetAttributes(&a, q) != hipSuccess) { (void)hipGetLastError(); return false; }
        if (a.type != hipMemoryTypeHost) return false;
    }
    return true;
}

static int land_launch(const u64 *src, u64 srcCols, u64 *dst, u64 dstCols, u64 nRows, u64 idxBase, u64 *firstBad, hipStream_t st) {
    if (dstCols < srcCols) return fail(PIL2GL_EINVAL, "land_rows: dstCols %llu < srcCols %llu", (unsigned long long)dstCols, (unsigned long long)srcCols);
    if (!nRows || !dstCols) return PIL2GL_OK;
    if (!src || !dst) return fail(PIL2GL_EINVAL, "null buffer");
    if (((uintptr_t)src | (uintptr_t)dst) & 7) return fail(PIL2GL_EINVAL, "land_rows: buffers must be 8-byte aligned");
    if (nRows > NO_BAD / 8 / dstCols) return fail(PIL2GL_EINVAL, "land_rows: size overflows");
    const bool same = srcCols == dstCols;
    if (!same || src != dst) {
        const u64 *dEnd = dst + nRows * dstCols, *sEnd = src + nRows * srcCols;
        if (src < dEnd && dst < sEnd) return fail(PIL2GL_EINVAL, "land_rows: src and dst overlap (only src == dst with equal widths lands in place)");
    }
    int mode; u64 elems;
    if (same && src == dst) { mode = LAND_CHECK; elems = nRows * srcCols / 2 + 1; }
    else if (same && !(((uintptr_t)src ^ (uintptr_t)dst) & 15)) { mode = LAND_COPY; elems = nRows * srcCols / 2 + 1; }
    else if (!((srcCols | dstCols) & 1) && !(((uintptr_t)src | (uintptr_t)dst) & 15)) { mode = LAND_WIDE2; elems = nRows * (dstCols / 2); }
    else { mode = LAND_WORD; elems = nRows * dstCols; }
    const u64 want = (elems + 255) / 256, cap = (u64)g_cus * 8;       // a grid sized to the chip; the stride loop takes the rest
    const unsigned grid = (unsigned)(want < cap ? want : cap);
    switch (mode) {
        case LAND_CHECK: land_rows_kernel<LAND_CHECK><<<grid, 256, 0, st>>>(src, srcCols, dst, dstCols, nRows, idxBase, firstBad); break;
        case LAND_COPY:  land_rows_kernel<LAND_COPY><<<grid, 256, 0, st>>>(src, srcCols, dst, dstCols, nRows, idxBase, firstBad); break;
        case LAND_WIDE2: land_rows_kernel<LAND_WIDE2><<<grid, 256, 0, st>>>(src, srcCols, dst, dstCols, nRows, idxBase, firstBad); break;
        default:         land_rows_kernel<LAND_WORD><<<grid, 256, 0, st>>>(src, srcCols, dst, dstCols, nRows, idxBase, firstBad); break;
    }
    KERNEL_CHECK();
    return PIL2GL_OK;
}

static int bad_reset(hipStream_t st) { HIP_TRY(hipMemsetAsync(g_bad_dev, 0xFF, 8, st)); return PIL2GL_OK; }
static int bad_fetch(hipStream_t st, u64 *out) {
    HIP_TRY(hipMemcpyAsync(g_bad_host, g_bad_dev, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    *out = *g_bad_host;
    return PIL2GL_OK;
}

struct Fd { int fd; ~Fd() { if (fd >= 0) close(fd); } };

static int read_fully(int fd, const char *name, void *buf, u64 nBytes, u64 at) {
    char *p = (char *)buf;
    while (nBytes) {
        const ssize_t got = pread(fd, p, nBytes, (off_t)at);
        if (got < 0) { if (errno == EINTR) continue; return fail(PIL2GL_EINVAL, "%s: read at byte %llu failed: %s", name, (unsigned long long)at, strerror(errno)); }
        if (got == 0) return fail(PIL2GL_EINVAL, "%s: ends at byte %llu, %llu more expected", name, (unsigned long long)at, (unsigned long long)nBytes);
        p += got; at += (u64)got; nBytes -= (u64)got;
    }
    return PIL2GL_OK;
}
static int write_fully(int fd, const char *name, const void *buf, u64 nBytes, u64 at) {
    const char *p = (const char *)buf;
    while (nBytes) {
        const ssize_t put = pwrite(fd, p, nBytes, (off_t)at);
        if (put < 0) { if (errno == EINTR) continue; return fail(PIL2GL_EINVAL, "%s: write at byte %llu failed: %s", name, (unsigned long long)at, strerror(errno)); }
        p += put; at += (u64)put; nBytes -= (u64)put;
    }
    return PIL2GL_OK;
}

}  // namespace pil2gl

using namespace pil2gl;

// the copy stream, its events and the chunks are process-global state like the tables and scratch slots: same lock (common.h)
#define HOSTLEG_LOCK() std::lock_guard<std::recursive_mutex> lk_(runtime_lock())

extern "C" {

int pil2gl_host_alloc(uint64_t nWords, uint64_t **out) {
    HOSTLEG_LOCK();
    P2_TRY(ensure_init());
    if (!out) return fail(PIL2GL_EINVAL, "null out pointer");
    HIP_TRY(hipHostMalloc((void **)out, (nWords ? nWords : 1) * 8, hipHostMallocDefault));
    return PIL2GL_OK;
}
int pil2gl_host_free(uint64_t *p) { if (p) HIP_TRY(hipHostFree(p)); return PIL2GL_OK; }
int pil2gl_host_register(uint64_t *p, uint64_t nWords) {
    HOSTLEG_LOCK();
    P2_TRY(ensure_init());
    if (!p || !nWords) return fail(PIL2GL_EINVAL, "host_register: null or empty buffer");
    HIP_TRY(hipHostRegister(p, nWords * 8, hipHostRegisterDefault));
    return PIL2GL_OK;
}
int pil2gl_host_unregister(uint64_t *p) { if (!p) return fail(PIL2GL_EINVAL, "null buffer"); HIP_TRY(hipHostUnregister(p)); return PIL2GL_OK; }

int pil2gl_dev_upload_async(uint64_t *dst, const uint64_t *hostSrc, uint64_t nWords) {
    HOSTLEG_LOCK();
    P2_TRY(copy_ready());
    if (!nWords) return PIL2GL_OK;
    if (!dst || !hostSrc) return fail(PIL2GL_EINVAL, "null buffer");
    if (!is_pinned(hostSrc, nWords * 8)) return fail(PIL2GL_EINVAL, "dev_upload_async: host memory is neither pinned (pil2gl_host_alloc) nor registered (pil2gl_host_register)");
    HIP_TRY(hipMemcpyAsync(dst, hostSrc, nWords * 8, hipMemcpyHostToDevice, g_copy));
    return PIL2GL_OK;
}
int pil2gl_dev_download_async(uint64_t *hostDst, const uint64_t *src, uint64_t nWords) {
    HOSTLEG_LOCK();
    P2_TRY(copy_ready());
    if (!nWords) return PIL2GL_OK;
    if (!hostDst || !src) return fail(PIL2GL_EINVAL, "null buffer");
    if (!is_pinned(hostDst, nWords * 8)) return fail(PIL2GL_EINVAL, "dev_download_async: host memory is neither pinned (pil2gl_host_alloc) nor registered (pil2gl_host_register)");
    HIP_TRY(hipMemcpyAsync(hostDst, src, nWords * 8, hipMemcpyDeviceToHost, g_copy));
    return PIL2GL_OK;
}
int pil2gl_copy_after(void *stream) {
    HOSTLEG_LOCK();
    P2_TRY(copy_ready());
    HIP_TRY(hipEventRecord(g_ev_after, as_stream(stream)));
    HIP_TRY(hipStreamWaitEvent(g_copy, g_ev_after, 0));
    return PIL2GL_OK;
}
int pil2gl_copy_fence(void *stream) {
    HOSTLEG_LOCK();
    P2_TRY(copy_ready());
    HIP_TRY(hipEventRecord(g_ev_fence, g_copy));
    HIP_TRY(hipStreamWaitEvent(as_stream(stream), g_ev_fence, 0));
    return PIL2GL_OK;
}
int pil2gl_copy_sync(void) {
    HOSTLEG_LOCK();
    P2_TRY(copy_ready());
    HIP_TRY(hipStreamSynchronize(g_copy));
    return PIL2GL_OK;
}

int pil2gl_land_rows_dev(const uint64_t *src, uint64_t srcCols, uint64_t *dst, uint64_t dstCols, uint64_t nRows,
                         uint64_t *hostFirstBad, void *stream) {
    HOSTLEG_LOCK();
    P2_TRY(copy_ready());
    hipStream_t st = as_stream(stream);
    if (!hostFirstBad) return land_launch(src, srcCols, dst, dstCols, nRows, 0, nullptr, st);
    P2_TRY(bad_reset(st));
    P2_TRY(land_launch(src, srcCols, dst, dstCols, nRows, 0, g_bad_dev, st));
    return bad_fetch(st, hostFirstBad);
}

int pil2gl_dev_load_file(const char *fileName, uint64_t byteOffset, uint64_t nRows, uint64_t srcCols,
                         uint64_t *dst, uint64_t dstCols, uint64_t chunkWords, uint64_t *hostFirstBad) {
    HOSTLEG_LOCK();
    P2_TRY(copy_ready());
    if (!fileName) return fail(PIL2GL_EINVAL, "null file name");
    if (dstCols < srcCols) return fail(PIL2GL_EINVAL, "dev_load_file: dstCols %llu < srcCols %llu", (unsigned long long)dstCols, (unsigned long long)srcCols);
    if (srcCols && nRows > NO_BAD / 8 / dstCols) return fail(PIL2GL_EINVAL, "dev_load_file: size overflows");
    if (!chunkWords) chunkWords = DEFAULT_CHUNK_WORDS;
    const u64 total = nRows * srcCols;
    const bool widen = dstCols != srcCols;
    if (widen && chunkWords < srcCols) return fail(PIL2GL_EINVAL, "dev_load_file: chunkWords %llu holds no whole row of %llu words", (unsigned long long)chunkWords, (unsigned long long)srcCols);
    if (total && (!dst || ((uintptr_t)dst & 7))) return fail(PIL2GL_EINVAL, "dev_load_file: dst must be an 8-byte aligned device buffer");
    Fd f = { open(fileName, O_RDONLY) };
    if (f.fd < 0) return fail(PIL2GL_EINVAL, "%s: %s", fileName, strerror(errno));
    struct stat sb;
    if (fstat(f.fd, &sb) != 0) return fail(PIL2GL_EINVAL, "%s: %s", fileName, strerror(errno));
    if (byteOffset > NO_BAD - 8 * total) return fail(PIL2GL_EINVAL, "dev_load_file: byteOffset %llu + %llu bytes overflows", (unsigned long long)byteOffset, (unsigned long long)(8 * total));
    if ((u64)sb.st_size < byteOffset + 8 * total)
        return fail(PIL2GL_EINVAL, "%s holds %llu bytes, expected %llu (%llu rows x %llu words from byte %llu)", fileName, (unsigned long long)sb.st_size,
                    (unsigned long long)(byteOffset + 8 * total), (unsigned long long)nRows, (unsigned long long)srcCols, (unsigned long long)byteOffset);
    if (hostFirstBad) { *hostFirstBad = NO_BAD; P2_TRY(bad_reset(g_copy)); }
    if (total) {
        P2_TRY(chunks_ready(chunkWords, widen));
        const u64 step = widen ? (chunkWords / srcCols) * srcCols : chunkWords;      // whole rows when rows change shape
        u64 *bad = hostFirstBad ? g_bad_dev : nullptr;
        int k = 0;
        for (u64 o = 0; o < total; o += step, k ^= 1) {
            const u64 m = total - o < step ? total - o : step;
            HIP_TRY(hipEventSynchronize(g_ev_chunk[k]));                             // the copy that last read this pinned chunk is done
            P2_TRY(read_fully(f.fd, fileName, g_pinned[k], m * 8, byteOffset + o * 8));
            if (!widen) {
                HIP_TRY(hipMemcpyAsync(dst + o, g_pinned[k], m * 8, hipMemcpyHostToDevice, g_copy));
                HIP_TRY(hipEventRecord(g_ev_chunk[k], g_copy));
                if (bad) P2_TRY(land_launch(dst + o, m, dst + o, m, 1, o, bad, g_copy));
            } else {
                // stream order keeps the landing pass that last read this staging chunk ahead of the copy that refills it
                HIP_TRY(hipMemcpyAsync(g_stage[k], g_pinned[k], m * 8, hipMemcpyHostToDevice, g_copy));
                HIP_TRY(hipEventRecord(g_ev_chunk[k], g_copy));
                P2_TRY(land_launch(g_stage[k], srcCols, dst + (o / srcCols) * dstCols, dstCols, m / srcCols, o, bad, g_copy));
            }
        }
    }
    if (hostFirstBad) return bad_fetch(g_copy, hostFirstBad);
    HIP_TRY(hipStreamSynchronize(g_copy));
    return PIL2GL_OK;
}

int pil2gl_dev_save_file(const char *fileName, uint64_t byteOffset, const uint64_t *src, uint64_t nWords, uint64_t chunkWords) {
    HOSTLEG_LOCK();
    P2_TRY(copy_ready());
    if (!fileName) return fail(PIL2GL_EINVAL, "null file name");
    if (nWords && !src) return fail(PIL2GL_EINVAL, "null buffer");
    if (!chunkWords) chunkWords = DEFAULT_CHUNK_WORDS;
    Fd f = { open(fileName, O_WRONLY | O_CREAT, 0666) };
    if (f.fd < 0) return fail(PIL2GL_EINVAL, "%s: %s", fileName, strerror(errno));
    struct stat sb;
    if (fstat(f.fd, &sb) != 0) return fail(PIL2GL_EINVAL, "%s: %s", fileName, strerror(errno));
    if ((u64)sb.st_size < byteOffset) return fail(PIL2GL_EINVAL, "%s holds %llu bytes, byteOffset %llu is beyond its end", fileName, (unsigned long long)sb.st_size, (unsigned long long)byteOffset);
    if (nWords > (NO_BAD >> 5) || byteOffset > (NO_BAD >> 1) - 8 * nWords) return fail(PIL2GL_EINVAL, "dev_save_file: byteOffset %llu overflows", (unsigned long long)byteOffset);
    if (ftruncate(f.fd, (off_t)byteOffset) != 0) return fail(PIL2GL_EINVAL, "%s: %s", fileName, strerror(errno));   // the words are the file's end
    if (!nWords) return PIL2GL_OK;
    P2_TRY(chunks_ready(chunkWords, false));
    // chunk k comes down into one pinned chunk while chunk k - 1 is written from the other
    u64 prevO = 0, prevM = 0; int k = 0;
    for (u64 o = 0; o < nWords; o += chunkWords, k ^= 1) {
        const u64 m = nWords - o < chunkWords ? nWords - o : chunkWords;
        HIP_TRY(hipMemcpyAsync(g_pinned[k], src + o, m * 8, hipMemcpyDeviceToHost, g_copy));
        HIP_TRY(hipEventRecord(g_ev_chunk[k], g_copy));
        if (prevM) { HIP_TRY(hipEventSynchronize(g_ev_chunk[k ^ 1])); P2_TRY(write_fully(f.fd, fileName, g_pinned[k ^ 1], prevM * 8, byteOffset + prevO * 8)); }
        prevO = o; prevM = m;
    }
    HIP_TRY(hipEventSynchronize(g_ev_chunk[k ^ 1]));
    return write_fully(f.fd, fileName, g_pinned[k ^ 1], prevM * 8, byteOffset + prevO * 8);
}

}  // extern "C"
