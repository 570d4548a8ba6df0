// N-API binding of the libpil2gl C ABI (include/pil2gl.h) for Node.js >= 12.17 (N-API 6: BigUint64Array).
//
// Thin by design: every export is one C-ABI call on raw pointers.  Host buffers are BigUint64Array
// (what the reference hands to its workers: fft_p.js:246, merklehash_p.js:70); device buffers are
// addresses carried as BigInt.  The CommonJS modules in ../js give these the reference's own
// function names and signatures.  Calls are synchronous (the reference awaits each one anyway).
#include <node_api.h>
#include <stdint.h>
#include <stddef.h>
#include <string.h>
#include <string>
#include <vector>
#include <unordered_map>
#include "pil2gl.h"

#define NAPI_CALL(env, call)                                                         \
    do { if ((call) != napi_ok) { napi_throw_error(env, nullptr, "N-API call failed: " #call); return nullptr; } } while (0)

static napi_value throw_rc(napi_env env, int rc) {
    std::string m = "pil2gl error " + std::to_string(rc) + ": " + pil2gl_last_error();
    napi_throw_error(env, nullptr, m.c_str());
    return nullptr;
}
#define P2(env, call) do { int rc_ = (call); if (rc_ != PIL2GL_OK) return throw_rc(env, rc_); } while (0)

struct Args {
    napi_env env; size_t argc; napi_value argv[12]; bool ok;
    Args(napi_env e, napi_callback_info info) : env(e), argc(12), ok(true) {
        if (napi_get_cb_info(e, info, &argc, argv, nullptr, nullptr) != napi_ok) ok = false;
    }
    bool fail(const char *m) { if (ok) napi_throw_type_error(env, nullptr, m); ok = false; return false; }
    uint64_t u64(size_t i) {                       // Number or BigInt
        if (!ok || i >= argc) { fail("missing argument"); return 0; }
        napi_valuetype t; napi_typeof(env, argv[i], &t);
        if (t == napi_bigint) { uint64_t v = 0; bool lossless; napi_get_value_bigint_uint64(env, argv[i], &v, &lossless); return v; }
        if (t == napi_number) { double d; napi_get_value_double(env, argv[i], &d); if (d < 0) { fail("negative size"); return 0; } return (uint64_t)d; }
        if (t == napi_boolean) { bool b; napi_get_value_bool(env, argv[i], &b); return b; }
        fail("expected a number or BigInt"); return 0;
    }
    bool is_nullish(size_t i) {
        if (i >= argc) return true;
        napi_valuetype t; napi_typeof(env, argv[i], &t);
        return t == napi_undefined || t == napi_null;
    }
    uint64_t *arr(size_t i, uint64_t minWords, uint64_t *len = nullptr) {   // BigUint64Array
        if (!ok || i >= argc) { fail("missing buffer argument"); return nullptr; }
        bool is; napi_is_typedarray(env, argv[i], &is);
        if (!is) { fail("expected a BigUint64Array"); return nullptr; }
        napi_typedarray_type ty; size_t n; void *data; napi_value ab; size_t off;
        napi_get_typedarray_info(env, argv[i], &ty, &n, &data, &ab, &off);
        if (ty != napi_biguint64_array && ty != napi_bigint64_array) { fail("expected a BigUint64Array"); return nullptr; }
        if (n < minWords) { fail("buffer too small"); return nullptr; }
        if (len) *len = n;
        return (uint64_t *)data;
    }
    void *stream(size_t i) { return is_nullish(i) ? nullptr : (void *)(uintptr_t)u64(i); }
};

static napi_value mk_undefined(napi_env env) { napi_value v; napi_get_undefined(env, &v); return v; }
static napi_value mk_bigint(napi_env env, uint64_t x) { napi_value v; napi_create_bigint_uint64(env, x, &v); return v; }

#define FN(name) static napi_value name(napi_env env, napi_callback_info info)
#define DP(i) ((uint64_t *)(uintptr_t)a.u64(i))      // a device address carried as BigInt

FN(Init) { Args a(env, info); int dev = a.is_nullish(0) ? 0 : (int)a.u64(0); if (!a.ok) return nullptr; P2(env, pil2gl_init(dev)); return mk_undefined(env); }
FN(Shutdown) { pil2gl_shutdown(); return mk_undefined(env); }
FN(DeviceInfo) {
    char name[64]; uint32_t cus; uint64_t mem;
    P2(env, pil2gl_device_info(name, sizeof name, &cus, &mem));
    napi_value o, v; napi_create_object(env, &o);
    napi_create_string_utf8(env, name, NAPI_AUTO_LENGTH, &v); napi_set_named_property(env, o, "name", v);
    napi_create_uint32(env, cus, &v); napi_set_named_property(env, o, "computeUnits", v);
    napi_set_named_property(env, o, "totalMem", mk_bigint(env, mem));
    return o;
}

// ---- device buffers ----
FN(DevAlloc) { Args a(env, info); uint64_t n = a.u64(0); if (!a.ok) return nullptr; uint64_t *p; P2(env, pil2gl_dev_alloc(n, &p)); return mk_bigint(env, (uint64_t)(uintptr_t)p); }
FN(DevFree) { Args a(env, info); uint64_t p = a.u64(0); if (!a.ok) return nullptr; P2(env, pil2gl_dev_free((uint64_t *)(uintptr_t)p)); return mk_undefined(env); }
FN(DevZero) { Args a(env, info); uint64_t p = a.u64(0), off = a.u64(1), n = a.u64(2); if (!a.ok) return nullptr; P2(env, pil2gl_dev_zero((uint64_t *)(uintptr_t)p + off, n, nullptr)); return mk_undefined(env); }
FN(DevUpload) {      // (devPtr, offsetWords, BigUint64Array)
    Args a(env, info); uint64_t p = a.u64(0), off = a.u64(1), n = 0; uint64_t *h = a.arr(2, 0, &n); if (!a.ok) return nullptr;
    P2(env, pil2gl_dev_upload((uint64_t *)(uintptr_t)p + off, h, n)); return mk_undefined(env);
}
FN(DevDownload) {    // (BigUint64Array, devPtr, offsetWords)
    Args a(env, info); uint64_t n = 0; uint64_t *h = a.arr(0, 0, &n); uint64_t p = a.u64(1), off = a.u64(2); if (!a.ok) return nullptr;
    P2(env, pil2gl_dev_download(h, (uint64_t *)(uintptr_t)p + off, n)); return mk_undefined(env);
}
FN(Sync) { P2(env, pil2gl_sync(nullptr)); return mk_undefined(env); }

// ---- the host <-> HBM leg (csrc/hostleg.hip): pinned memory, asynchronous copies on the library's copy stream, file loaders ----
// hostAlloc(nWords) -> BigUint64Array over pinned memory (an external ArrayBuffer); the memory goes back when the ArrayBuffer is
// collected, or at hostFree(array) -- after which the array must not be touched (js/native.js PinnedBuffer drops it).
// Liveness is kept PER ALLOCATION: each ArrayBuffer's finalizer carries its own record.  An address comes back from the allocator
// once it is freed, so the finalizer of an array freed by hand must never take the address's word for it.
struct PinnedRec { uint64_t *p; bool freed; };
static std::unordered_map<void *, PinnedRec *> &pinned_live() { static std::unordered_map<void *, PinnedRec *> m; return m; }     // address -> its LIVE allocation
static void pinned_finalize(napi_env, void *, void *hint) {
    PinnedRec *rec = (PinnedRec *)hint;
    if (!rec->freed) { pinned_live().erase(rec->p); (void)pil2gl_host_free(rec->p); }
    delete rec;
}
FN(HostAlloc) {
    Args a(env, info); uint64_t n = a.u64(0); if (!a.ok) return nullptr;
    uint64_t *p; P2(env, pil2gl_host_alloc(n, &p));
    PinnedRec *rec = new PinnedRec{ p, false };
    napi_value ab, ta;
    if (napi_create_external_arraybuffer(env, p, n * 8, pinned_finalize, rec, &ab) != napi_ok) {
        delete rec; (void)pil2gl_host_free(p); napi_throw_error(env, nullptr, "pinned memory cannot be wrapped in an ArrayBuffer of this length"); return nullptr; }
    pinned_live()[p] = rec;                 // from here on the ArrayBuffer's finalizer owns rec
    if (napi_create_typedarray(env, napi_biguint64_array, n, ab, 0, &ta) != napi_ok) { napi_throw_error(env, nullptr, "pinned memory cannot be wrapped in a BigUint64Array of this length"); return nullptr; }
    return ta;
}
FN(HostFree) {       // (BigUint64Array from hostAlloc)
    Args a(env, info); uint64_t *h = a.arr(0, 0); if (!a.ok) return nullptr;
    auto &m = pinned_live(); auto it = m.find(h);
    if (it == m.end()) { napi_throw_error(env, nullptr, "hostFree: not a live hostAlloc array"); return nullptr; }
    it->second->freed = true;               // its finalizer will find nothing left to do, whoever holds the address by then
    m.erase(it);
    P2(env, pil2gl_host_free(h)); return mk_undefined(env);
}
FN(HostRegister) { Args a(env, info); uint64_t n = 0; uint64_t *h = a.arr(0, 1, &n); if (!a.ok) return nullptr; P2(env, pil2gl_host_register(h, n)); return mk_undefined(env); }
FN(HostUnregister) { Args a(env, info); uint64_t *h = a.arr(0, 1); if (!a.ok) return nullptr; P2(env, pil2gl_host_unregister(h)); return mk_undefined(env); }
FN(DevUploadAsync) {   // (devPtr, offsetWords, pinned BigUint64Array): enqueues on the copy stream; keep the array alive until copySync / a fenced stream is done
    Args a(env, info); uint64_t p = a.u64(0), off = a.u64(1), n = 0; uint64_t *h = a.arr(2, 0, &n); if (!a.ok) return nullptr;
    P2(env, pil2gl_dev_upload_async((uint64_t *)(uintptr_t)p + off, h, n)); return mk_undefined(env);
}
FN(DevDownloadAsync) { // (pinned BigUint64Array, devPtr, offsetWords)
    Args a(env, info); uint64_t n = 0; uint64_t *h = a.arr(0, 0, &n); uint64_t p = a.u64(1), off = a.u64(2); if (!a.ok) return nullptr;
    P2(env, pil2gl_dev_download_async(h, (uint64_t *)(uintptr_t)p + off, n)); return mk_undefined(env);
}
FN(CopyAfter) { Args a(env, info); P2(env, pil2gl_copy_after(a.stream(0))); return mk_undefined(env); }
FN(CopyFence) { Args a(env, info); P2(env, pil2gl_copy_fence(a.stream(0))); return mk_undefined(env); }
FN(CopySync) { P2(env, pil2gl_copy_sync()); return mk_undefined(env); }
FN(LandRowsDev) {      // (dSrc, srcCols, dDst, dstCols, nRows, check[, stream]) -> first non-canonical index as BigInt (2^64-1: none), undefined without check
    Args a(env, info); uint64_t *s = DP(0); uint64_t sc = a.u64(1); uint64_t *d = DP(2); uint64_t dc = a.u64(3), nRows = a.u64(4); bool check = a.u64(5) != 0; if (!a.ok) return nullptr;
    uint64_t bad = ~0ull;
    P2(env, pil2gl_land_rows_dev(s, sc, d, dc, nRows, check ? &bad : nullptr, a.stream(6)));
    return check ? mk_bigint(env, bad) : mk_undefined(env);
}
static bool get_string(Args &a, size_t i, std::string &out) {
    size_t len = 0;
    if (i >= a.argc || napi_get_value_string_utf8(a.env, a.argv[i], nullptr, 0, &len) != napi_ok) return a.fail("expected a file name");
    out.resize(len + 1);
    napi_get_value_string_utf8(a.env, a.argv[i], &out[0], len + 1, &len);
    out.resize(len);
    return true;
}
FN(DevLoadFile) {      // (fileName, byteOffset, nRows, srcCols, dDst, dstCols, chunkWords, check) -> first non-canonical index as BigInt / undefined
    Args a(env, info); std::string name; get_string(a, 0, name);
    uint64_t off = a.u64(1), nRows = a.u64(2), sc = a.u64(3); uint64_t *d = DP(4); uint64_t dc = a.u64(5), chunk = a.u64(6); bool check = a.u64(7) != 0; if (!a.ok) return nullptr;
    uint64_t bad = ~0ull;
    P2(env, pil2gl_dev_load_file(name.c_str(), off, nRows, sc, d, dc, chunk, check ? &bad : nullptr));
    return check ? mk_bigint(env, bad) : mk_undefined(env);
}
FN(DevSaveFile) {      // (fileName, byteOffset, dSrc, nWords, chunkWords)
    Args a(env, info); std::string name; get_string(a, 0, name);
    uint64_t off = a.u64(1); uint64_t *s = DP(2); uint64_t n = a.u64(3), chunk = a.u64(4); if (!a.ok) return nullptr;
    P2(env, pil2gl_dev_save_file(name.c_str(), off, s, n, chunk)); return mk_undefined(env);
}

// ---- NTT ----
FN(Interpolate) {    // (src, nPols, nBits, dst, nBitsExt)  fft_p.js:187
    Args a(env, info); uint64_t nPols = a.u64(1); uint32_t nBits = (uint32_t)a.u64(2), nBitsExt = (uint32_t)a.u64(4);
    if (nBits > 40 || nBitsExt > 40) a.fail("bad size");
    uint64_t *s = a.arr(0, a.ok ? nPols << nBits : 0), *d = a.arr(3, a.ok ? nPols << nBitsExt : 0); if (!a.ok) return nullptr;
    P2(env, pil2gl_interpolate(s, nPols, nBits, d, nBitsExt)); return mk_undefined(env);
}
static napi_value fft_common(napi_env env, napi_callback_info info, bool inverse) {
    Args a(env, info); uint64_t nPols = a.u64(1); uint32_t nBits = (uint32_t)a.u64(2);
    if (nBits > 40) a.fail("bad size");
    uint64_t *s = a.arr(0, a.ok ? nPols << nBits : 0), *d = a.arr(3, a.ok ? nPols << nBits : 0); if (!a.ok) return nullptr;
    P2(env, inverse ? pil2gl_ifft(s, nPols, nBits, d) : pil2gl_fft(s, nPols, nBits, d)); return mk_undefined(env);
}
FN(Fft) { return fft_common(env, info, false); }
FN(Ifft) { return fft_common(env, info, true); }
FN(InterpolateDev) {
    Args a(env, info); uint64_t s = a.u64(0), nPols = a.u64(1), nBits = a.u64(2), d = a.u64(3), nBitsExt = a.u64(4); if (!a.ok) return nullptr;
    P2(env, pil2gl_interpolate_dev((const uint64_t *)(uintptr_t)s, nPols, (uint32_t)nBits, (uint64_t *)(uintptr_t)d, (uint32_t)nBitsExt, a.stream(5))); return mk_undefined(env);
}
FN(FftDev) {
    Args a(env, info); uint64_t s = a.u64(0), nPols = a.u64(1), nBits = a.u64(2), d = a.u64(3); if (!a.ok) return nullptr;
    P2(env, pil2gl_fft_dev((const uint64_t *)(uintptr_t)s, nPols, (uint32_t)nBits, (uint64_t *)(uintptr_t)d, a.stream(4))); return mk_undefined(env);
}
FN(IfftDev) {
    Args a(env, info); uint64_t s = a.u64(0), nPols = a.u64(1), nBits = a.u64(2), d = a.u64(3); if (!a.ok) return nullptr;
    P2(env, pil2gl_ifft_dev((const uint64_t *)(uintptr_t)s, nPols, (uint32_t)nBits, (uint64_t *)(uintptr_t)d, a.stream(4))); return mk_undefined(env);
}

// ---- BN254 Fr transforms (fft_p.bn128.js:178-285): 4 words per element, Montgomery form ----
static napi_value bn128_fft_common(napi_env env, napi_callback_info info, bool inverse) {      // (src, nPols, nBits, dst)
    Args a(env, info); uint64_t nPols = a.u64(1); uint32_t nBits = (uint32_t)a.u64(2);
    if (nBits > 40) a.fail("bad size");
    uint64_t *s = a.arr(0, a.ok ? (nPols << nBits) * 4 : 0), *d = a.arr(3, a.ok ? (nPols << nBits) * 4 : 0); if (!a.ok) return nullptr;
    P2(env, inverse ? pil2gl_bn128_ifft(s, nPols, nBits, d) : pil2gl_bn128_fft(s, nPols, nBits, d)); return mk_undefined(env);
}
FN(Bn128Fft) { return bn128_fft_common(env, info, false); }
FN(Bn128Ifft) { return bn128_fft_common(env, info, true); }
FN(Bn128Interpolate) {   // (src, nPols, nBits, dstCoefs | null, dst, nBitsExt)  fft_p.bn128.js:225
    Args a(env, info); uint64_t nPols = a.u64(1); uint32_t nBits = (uint32_t)a.u64(2), nBitsExt = (uint32_t)a.u64(5);
    if (nBits > 40 || nBitsExt > 40) a.fail("bad size");
    uint64_t *s = a.arr(0, a.ok ? (nPols << nBits) * 4 : 0), *c = a.is_nullish(3) ? nullptr : a.arr(3, a.ok ? (nPols << nBits) * 4 : 0);
    uint64_t *d = a.arr(4, a.ok ? (nPols << nBitsExt) * 4 : 0); if (!a.ok) return nullptr;
    P2(env, pil2gl_bn128_interpolate(s, nPols, nBits, c, d, nBitsExt)); return mk_undefined(env);
}
FN(Bn128FftDev) {        // (dSrc, nPols, nBits, dDst[, stream])
    Args a(env, info); uint64_t *s = DP(0); uint64_t nPols = a.u64(1), nBits = a.u64(2); uint64_t *d = DP(3); if (!a.ok) return nullptr;
    P2(env, pil2gl_bn128_fft_dev(s, nPols, (uint32_t)nBits, d, a.stream(4))); return mk_undefined(env);
}
FN(Bn128IfftDev) {
    Args a(env, info); uint64_t *s = DP(0); uint64_t nPols = a.u64(1), nBits = a.u64(2); uint64_t *d = DP(3); if (!a.ok) return nullptr;
    P2(env, pil2gl_bn128_ifft_dev(s, nPols, (uint32_t)nBits, d, a.stream(4))); return mk_undefined(env);
}
FN(Bn128InterpolateDev) { // (dSrc, nPols, nBits, dDstCoefs | null, dDst, nBitsExt[, stream])
    Args a(env, info); uint64_t *s = DP(0); uint64_t nPols = a.u64(1), nBits = a.u64(2); uint64_t *c = a.is_nullish(3) ? nullptr : DP(3); uint64_t *d = DP(4); uint64_t nBitsExt = a.u64(5);
    if (!a.ok) return nullptr;
    P2(env, pil2gl_bn128_interpolate_dev(s, nPols, (uint32_t)nBits, c, d, (uint32_t)nBitsExt, a.stream(6))); return mk_undefined(env);
}

// ---- BN254 G1 multi-scalar multiplication (G1.multiExpAffine + toAffine): device pointers, the 64 bytes written on the device ----
FN(Bn128G1MsmDev) {      // (dBases, dScalars, n, scalarStride, scalarsMontgomery, dOut[, stream])
    Args a(env, info); uint64_t *b = DP(0), *s = DP(1); uint64_t n = a.u64(2), stride = a.u64(3), mont = a.u64(4); uint64_t *o = DP(5); if (!a.ok) return nullptr;
    P2(env, pil2gl_bn128_g1_msm_dev(b, s, n, stride, (uint32_t)mont, o, a.stream(6))); return mk_undefined(env);
}

// K packed polynomials over the same bases, K * 8 words written on the device
// (dBases, nBases, dScalars, rowStride, scalarsMontgomery, polys BigUint64Array of (first, rows, m) per polynomial, slots BigUint64Array of one
//  column index or 0xFFFFFFFF per slot, dOut[, stream])
FN(Bn128G1CommitDev) {
    Args a(env, info); uint64_t *b = DP(0); uint64_t nBases = a.u64(1); uint64_t *s = DP(2); uint64_t stride = a.u64(3), mont = a.u64(4);
    uint64_t nDesc = 0, nSlots = 0;
    uint64_t *desc = a.arr(5, 0, &nDesc), *slotWords = a.arr(6, 0, &nSlots); uint64_t *o = DP(7);
    if (a.ok && (nDesc % 3 || nDesc > 3 * 64)) a.fail("polys must hold (first, rows, m) per polynomial");
    if (a.ok && nSlots > 4096) a.fail("too many slots");
    if (!a.ok) return nullptr;
    std::vector<pil2gl_g1_poly> polys(nDesc / 3 + 1);
    std::vector<uint32_t> slots(nSlots + 1);
    uint64_t need = 0;
    for (uint64_t k = 0; k < nDesc / 3; k++) {
        polys[k].first = desc[3 * k]; polys[k].rows = desc[3 * k + 1]; polys[k].reserved = 0;
        polys[k].m = desc[3 * k + 2] > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)desc[3 * k + 2];
        need += polys[k].m;
    }
    if (need > nSlots) { a.fail("slots hold fewer entries than the polynomials name"); return nullptr; }
    for (uint64_t j = 0; j < nSlots; j++) slots[j] = slotWords[j] > 0xFFFFFFFFull ? 0xFFFFFFFEu : (uint32_t)slotWords[j];      // too large: refused by the library as a column
    P2(env, pil2gl_bn128_g1_commit_dev(b, nBases, s, stride, (uint32_t)mont, polys.data(), (uint32_t)(nDesc / 3), slots.data(), o, a.stream(8)));
    return mk_undefined(env);
}

// ---- BN254 Fr expression evaluator (calculateExps over curve.Fr): device sections, Montgomery scalars ----
// (opsBuf BigUint64Array = packed glx_op[], nOps, nTmp, nBits, primeShift, sectionPtrs BigUint64Array, sectionWidths BigUint64Array in elements,
//  scalars BigUint64Array of 4 words per element[, stream])
FN(Bn128EvalProgramDev) {
    Args a(env, info); uint64_t nOps = a.u64(1), nTmp = a.u64(2), nBits = a.u64(3), ps = a.u64(4);
    uint64_t nSec = 0, nSec2 = 0, nSc = 0;
    uint64_t *ops = a.arr(0, nOps * (sizeof(glx_op) / 8)), *ptrs = a.arr(5, 0, &nSec), *widths = a.arr(6, 0, &nSec2), *scal = a.arr(7, 0, &nSc);
    if (a.ok && nSec != nSec2) a.fail("section arrays differ in length");
    if (a.ok && nSc % 4) a.fail("scalars must hold 4 words per element");
    if (!a.ok) return nullptr;
    std::vector<bnx_section> secs(nSec);
    for (uint64_t i = 0; i < nSec; i++) { secs[i].ptr = (uint64_t *)(uintptr_t)ptrs[i]; secs[i].width = widths[i]; }
    glx_program prog = { (uint32_t)nOps, (uint32_t)nTmp, (const glx_op *)ops };
    bnx_ctx ctx = { (uint32_t)nBits, (uint32_t)ps, (uint32_t)nSec, (uint32_t)(nSc / 4), secs.data(), scal };
    P2(env, pil2gl_bn128_eval_program_dev(&prog, &ctx, a.stream(8))); return mk_undefined(env);
}
// (devSection, width, column, first, last) -> [row, w0, w1, w2, w3] as BigInt, row = 2^64-1 when the column is zero on [first, last)
FN(Bn128FirstNonzeroRowDev) {
    Args a(env, info); uint64_t col = a.u64(0), width = a.u64(1), column = a.u64(2), first = a.u64(3), last = a.u64(4);
    if (!a.ok) return nullptr;
    uint64_t out[5] = { 0, 0, 0, 0, 0 };
    P2(env, pil2gl_bn128_first_nonzero_row_dev((const uint64_t *)(uintptr_t)col, width, column, first, last, &out[0], &out[1], nullptr));
    napi_value arr; NAPI_CALL(env, napi_create_array_with_length(env, 5, &arr));
    for (uint32_t i = 0; i < 5; i++) { napi_value v; NAPI_CALL(env, napi_create_bigint_uint64(env, out[i], &v)); NAPI_CALL(env, napi_set_element(env, arr, i, v)); }
    return arr;
}

// ---- BN254 Fr polynomial division by x^k - beta and evaluation: device coefficients, beta / points as host Montgomery words ----
FN(Bn128PolyDivDev) {    // (dSrc, n, stride, k, beta BigUint64Array(4), dDst[, stream])
    Args a(env, info); uint64_t *s = DP(0); uint64_t n = a.u64(1), stride = a.u64(2), k = a.u64(3); uint64_t *beta = a.arr(4, 4); uint64_t *d = DP(5);
    if (!a.ok) return nullptr;
    P2(env, pil2gl_bn128_poly_div_xk_sub_dev(s, n, stride, k, beta, d, a.stream(6))); return mk_undefined(env);
}
FN(Bn128PolyEvalDev) {   // (dSrc, n, stride, points BigUint64Array(4 * nPoints), dOut[, stream])
    Args a(env, info); uint64_t *s = DP(0); uint64_t n = a.u64(1), stride = a.u64(2), len = 0; uint64_t *pts = a.arr(3, 4, &len); uint64_t *o = DP(4);
    if (a.ok && (len % 4 || len / 4 > 64)) a.fail("points must hold 4 words per point, at most 64 points");
    if (!a.ok) return nullptr;
    P2(env, pil2gl_bn128_poly_eval_dev(s, n, stride, pts, (uint32_t)(len / 4), o, a.stream(5))); return mk_undefined(env);
}

// ---- BN254 Fr products with a sparse polynomial, scaled sums and the degree (shplonkjs open): device columns, host scale / terms ----
FN(Bn128PolyFmaDev) {    // (dAcc, nAcc, accStride, scale BigUint64Array(4) | null, dSrc, nSrc, srcStride, coefs BigUint64Array(4 t), exps BigUint64Array(t)[, stream])
    Args a(env, info); uint64_t *acc = DP(0); uint64_t nAcc = a.u64(1), as = a.u64(2); uint64_t *scale = a.is_nullish(3) ? nullptr : a.arr(3, 4);
    uint64_t *src = DP(4); uint64_t nSrc = a.u64(5), ss = a.u64(6), nc = 0, ne = 0; uint64_t *coefs = a.arr(7, 0, &nc), *exps = a.arr(8, 0, &ne);
    if (a.ok && (nc != 4 * ne || ne > 0xFFFFFFFFull)) a.fail("coefs must hold 4 words per exponent");
    if (!a.ok) return nullptr;
    P2(env, pil2gl_bn128_poly_fma_dev(acc, nAcc, as, scale, src, nSrc, ss, coefs, exps, (uint32_t)ne, a.stream(9))); return mk_undefined(env);
}
FN(Bn128PolyDegreeDev) { // (dSrc, n, stride[, stream]) -> the degree as a BigInt, 2^64-1 for the zero polynomial
    Args a(env, info); uint64_t *s = DP(0); uint64_t n = a.u64(1), stride = a.u64(2);
    if (!a.ok) return nullptr;
    uint64_t deg = UINT64_MAX;
    P2(env, pil2gl_bn128_poly_degree_dev(s, n, stride, &deg, a.stream(3))); return mk_bigint(env, deg);
}

// ---- BN254 Fr batch inverse, grand product and grand sum (the gprod / gsum hints over curve.Fr): device columns, each with its stride ----
FN(Bn128BatchInverseDev) {   // (dSrc, srcStride, n, dDst, dstStride[, stream])
    Args a(env, info); uint64_t *s = DP(0); uint64_t ss = a.u64(1), n = a.u64(2); uint64_t *d = DP(3); uint64_t ds = a.u64(4);
    if (!a.ok) return nullptr;
    P2(env, pil2gl_bn128_batch_inverse_dev(s, ss, n, d, ds, a.stream(5))); return mk_undefined(env);
}
FN(Bn128GprodDev) {          // (dNum, numStride, dDen, denStride, n, dOut, outStride[, stream])
    Args a(env, info); uint64_t *nu = DP(0); uint64_t ns = a.u64(1); uint64_t *de = DP(2); uint64_t ds = a.u64(3), n = a.u64(4); uint64_t *o = DP(5); uint64_t os = a.u64(6);
    if (!a.ok) return nullptr;
    P2(env, pil2gl_bn128_gprod_dev(nu, ns, de, ds, n, o, os, a.stream(7))); return mk_undefined(env);
}
FN(Bn128GsumDev) {           // (num BigUint64Array(4), dDen, denStride, n, dOut, outStride[, stream])
    Args a(env, info); uint64_t *nu = a.arr(0, 4); uint64_t *de = DP(1); uint64_t ds = a.u64(2), n = a.u64(3); uint64_t *o = DP(4); uint64_t os = a.u64(5);
    if (!a.ok) return nullptr;
    P2(env, pil2gl_bn128_gsum_dev(nu, de, ds, n, o, os, a.stream(6))); return mk_undefined(env);
}
FN(Bn128GsumColDev) {        // (dNum, numStride, dDen, denStride, n, dOut, outStride[, stream]): gsum with a column numerator
    Args a(env, info); uint64_t *nu = DP(0); uint64_t ns = a.u64(1); uint64_t *de = DP(2); uint64_t ds = a.u64(3), n = a.u64(4); uint64_t *o = DP(5); uint64_t os = a.u64(6);
    if (!a.ok) return nullptr;
    P2(env, pil2gl_bn128_gsum_col_dev(nu, ns, de, ds, n, o, os, a.stream(7))); return mk_undefined(env);
}
// the plookup hint over curve.Fr (calculateH1H2).  A value of f that is not in t is no exception here: the row comes back, and
// js/polutils_bn128.js throws the reference's full message, which needs the element
FN(Bn128H1h2Dev) {           // (dF, fStride, dT, tStride, n, dH1, h1Stride, dH2, h2Stride[, stream]) -> undefined, or the lowest missing row as a BigInt
    Args a(env, info); uint64_t *f = DP(0); uint64_t fs = a.u64(1); uint64_t *t = DP(2); uint64_t ts = a.u64(3), n = a.u64(4);
    uint64_t *h1 = DP(5); uint64_t s1 = a.u64(6); uint64_t *h2 = DP(7); uint64_t s2 = a.u64(8);
    if (!a.ok) return nullptr;
    uint64_t miss = UINT64_MAX;
    const int rc = pil2gl_bn128_h1h2_dev(f, fs, t, ts, n, h1, s1, h2, s2, &miss, a.stream(9));
    if (rc == PIL2GL_EINVAL && miss != UINT64_MAX) return mk_bigint(env, miss);
    P2(env, rc); return mk_undefined(env);
}

// ---- hashing ----
FN(Poseidon) {      // (in BigUint64Array(8*count), cap BigUint64Array(4*count)|null, count, nOut, out)
    Args a(env, info); uint64_t count = a.u64(2); uint32_t nOut = (uint32_t)a.u64(3);
    uint64_t *in = a.arr(0, 8 * count), *cap = a.is_nullish(1) ? nullptr : a.arr(1, 4 * count), *out = a.arr(4, (uint64_t)nOut * count); if (!a.ok) return nullptr;
    P2(env, pil2gl_poseidon(in, cap, count, nOut, out)); return mk_undefined(env);
}
FN(LinearHashRows) { // (in, width, height, split, out)  merklehash_worker.js:37
    Args a(env, info); uint64_t w = a.u64(1), h = a.u64(2); int split = (int)a.u64(3);
    uint64_t *in = a.arr(0, w * h), *out = a.arr(4, 4 * h); if (!a.ok) return nullptr;
    P2(env, pil2gl_linear_hash_rows(in, w, h, split, out)); return mk_undefined(env);
}
FN(MerkelizeLevel) { // (in, nOps, out)  merklehash_worker.js:86
    Args a(env, info); uint64_t n = a.u64(1); uint64_t *in = a.arr(0, 8 * n), *out = a.arr(2, 4 * n); if (!a.ok) return nullptr;
    P2(env, pil2gl_merkelize_level(in, n, out)); return mk_undefined(env);
}
FN(MerkleNumNodes) { Args a(env, info); uint64_t h = a.u64(0); if (!a.ok) return nullptr; napi_value v; napi_create_double(env, (double)pil2gl_merkle_num_nodes(h), &v); return v; }
FN(Merkelize) {      // (elems, width, height, split, nodes)  merklehash_p.js:44
    Args a(env, info); uint64_t w = a.u64(1), h = a.u64(2); int split = (int)a.u64(3);
    uint64_t *el = a.arr(0, w * h), *nodes = a.arr(4, pil2gl_merkle_num_nodes(h)); if (!a.ok) return nullptr;
    P2(env, pil2gl_merkelize(el, w, h, split, nodes)); return mk_undefined(env);
}
FN(MerkelizeDev) {   // (devElems, width, height, split, devNodes)
    Args a(env, info); uint64_t el = a.u64(0), w = a.u64(1), h = a.u64(2); int split = (int)a.u64(3); uint64_t nodes = a.u64(4); if (!a.ok) return nullptr;
    P2(env, pil2gl_merkelize_dev((const uint64_t *)(uintptr_t)el, w, h, split, (uint64_t *)(uintptr_t)nodes, a.stream(5))); return mk_undefined(env);
}
FN(GroupProofDev) {  // (devElems, devNodes, width, height, idx, vals BigUint64Array(width), siblings BigUint64Array(4*64)) -> nLevels
    Args a(env, info); uint64_t el = a.u64(0), nodes = a.u64(1), w = a.u64(2), h = a.u64(3), idx = a.u64(4);
    uint64_t *vals = a.arr(5, w), *sib = a.arr(6, 4 * 64); if (!a.ok) return nullptr;
    uint32_t nl = 0;
    P2(env, pil2gl_group_proof_dev((const uint64_t *)(uintptr_t)el, (const uint64_t *)(uintptr_t)nodes, w, h, idx, vals, sib, &nl));
    napi_value v; napi_create_uint32(env, nl, &v); return v;
}

FN(GroupProofsDev) { // (devElems, devNodes, width, height, idxs BigUint64Array(n), out BigUint64Array(n*(width+4*levels))) -> nLevels: every query of a tree in one gather
    Args a(env, info); uint64_t el = a.u64(0), nodes = a.u64(1), w = a.u64(2), h = a.u64(3);
    uint64_t n = 0; uint64_t *idxs = a.arr(4, 1, &n); uint64_t *out = a.arr(5, n * w); if (!a.ok) return nullptr;
    uint32_t nl = 0;
    for (uint64_t m = h * 4; m > 4; m = ((m - 1) / 8 + 1) * 4) nl++;
    uint64_t outLen = 0; a.arr(5, n * (w + 4ull * nl), &outLen); if (!a.ok) return nullptr;
    P2(env, pil2gl_group_proofs_dev((const uint64_t *)(uintptr_t)el, (const uint64_t *)(uintptr_t)nodes, w, h, idxs, (uint32_t)n, out, &nl));
    napi_value v; napi_create_uint32(env, nl, &v); return v;
}

FN(SpongeAbsorb) {  // (blocks BigUint64Array(8*n), n, cap BigUint64Array(4), out BigUint64Array(12))  transcript.js:49-66 for a list
    Args a(env, info); uint64_t n = a.u64(1);
    uint64_t *blocks = a.arr(0, 8 * n), *cap = a.arr(2, 4), *out = a.arr(3, 12); if (!a.ok) return nullptr;
    P2(env, pil2gl_sponge_absorb(blocks, n, cap, out)); return mk_undefined(env);
}
FN(RootsFromGroupProofs) {  // (packed BigUint64Array(n*(width+4*levels)), width, levels, idxs BigUint64Array(n), n, split, roots BigUint64Array(4n))
    Args a(env, info); uint64_t w = a.u64(1), lv = a.u64(2), n = a.u64(4); int split = (int)a.u64(5);
    uint64_t *packed = a.arr(0, n * (w + 4 * lv)), *idx = a.arr(3, n), *roots = a.arr(6, 4 * n); if (!a.ok) return nullptr;
    P2(env, pil2gl_roots_from_group_proofs(packed, w, (uint32_t)lv, idx, (uint32_t)n, split, roots)); return mk_undefined(env);
}

// ---- STARK step helpers and stage-2 hints (device pointers; js/stark_gen_helpers.js and js/polutils.js stage host buffers) ----
FN(BuildXDev) {        // (nBits, shift, dX)  stark_gen_helpers.js:111-116,139-144
    Args a(env, info); uint32_t nBits = (uint32_t)a.u64(0); uint64_t shift = a.u64(1); uint64_t *x = DP(2); if (!a.ok) return nullptr;
    P2(env, pil2gl_build_x_dev(nBits, shift, x, a.stream(3))); return mk_undefined(env);
}
FN(BuildZhInvDev) {    // (nBits, nBitsExt, dOut)  polutils.js:39-55
    Args a(env, info); uint32_t nb = (uint32_t)a.u64(0), nbe = (uint32_t)a.u64(1); uint64_t *o = DP(2); if (!a.ok) return nullptr;
    P2(env, pil2gl_build_zhinv_dev(nb, nbe, o, a.stream(3))); return mk_undefined(env);
}
FN(BuildOneRowZerofierInvDev) {   // (nBits, nBitsExt, rowIndex, dOut)  polutils.js:57-71
    Args a(env, info); uint32_t nb = (uint32_t)a.u64(0), nbe = (uint32_t)a.u64(1); uint64_t row = a.u64(2); uint64_t *o = DP(3); if (!a.ok) return nullptr;
    P2(env, pil2gl_build_one_row_zerofier_inv_dev(nb, nbe, row, o, a.stream(4))); return mk_undefined(env);
}
FN(BuildFrameZerofierDev) {       // (nBits, nBitsExt, offsetMin, offsetMax, dOut)  polutils.js:74-102
    Args a(env, info); uint32_t nb = (uint32_t)a.u64(0), nbe = (uint32_t)a.u64(1); uint64_t mn = a.u64(2), mx = a.u64(3); uint64_t *o = DP(4); if (!a.ok) return nullptr;
    P2(env, pil2gl_build_frame_zerofier_dev(nb, nbe, mn, mx, o, a.stream(5))); return mk_undefined(env);
}
FN(ComputeQSplitDev) { // (dQq1, nBits, nBitsExt, qDim, qDeg, dQq2)  stark_gen_helpers.js:179-190
    Args a(env, info); uint64_t *q1 = DP(0); uint32_t nb = (uint32_t)a.u64(1), nbe = (uint32_t)a.u64(2), qDim = (uint32_t)a.u64(3), qDeg = (uint32_t)a.u64(4); uint64_t *q2 = DP(5); if (!a.ok) return nullptr;
    P2(env, pil2gl_compute_q_split_dev(q1, nb, nbe, qDim, qDeg, q2, a.stream(6))); return mk_undefined(env);
}
FN(ComputeQSplitBrevDev) { // (dQq1, nBits, nBitsExt, qDim, qDeg, dCoefBrev): the pieces as N coefficient rows, row bitrev(i) = coefficient i
    Args a(env, info); uint64_t *q1 = DP(0); uint32_t nb = (uint32_t)a.u64(1), nbe = (uint32_t)a.u64(2), qDim = (uint32_t)a.u64(3), qDeg = (uint32_t)a.u64(4); uint64_t *c = DP(5); if (!a.ok) return nullptr;
    P2(env, pil2gl_compute_q_split_brev_dev(q1, nb, nbe, qDim, qDeg, c, a.stream(6))); return mk_undefined(env);
}
FN(ExtendCoefsBrevDev) { // (dCoefBrev, nPols, nBits, dDst, nBitsExt): fft(nBitsExt) of the zero-padded coefficients (stark_gen_helpers.js:192)
    Args a(env, info); uint64_t s = a.u64(0), nPols = a.u64(1), nBits = a.u64(2), d = a.u64(3), nBitsExt = a.u64(4); if (!a.ok) return nullptr;
    P2(env, pil2gl_extend_coefs_brev_dev((const uint64_t *)(uintptr_t)s, nPols, (uint32_t)nBits, (uint64_t *)(uintptr_t)d, (uint32_t)nBitsExt, a.stream(5))); return mk_undefined(env);
}
FN(XDivXSubXiDev) {    // (nBitsExt, xi BigUint64Array(3), nOpen, iOpen, dOut)  stark_gen_helpers.js:293-322
    Args a(env, info); uint32_t nbe = (uint32_t)a.u64(0); uint64_t *xi = a.arr(1, 3); uint64_t nOpen = a.u64(2), iOpen = a.u64(3); uint64_t *o = DP(4); if (!a.ok) return nullptr;
    P2(env, pil2gl_x_div_x_sub_xi_dev(nbe, xi, nOpen, iOpen, o, a.stream(5))); return mk_undefined(env);
}
FN(BuildLevDev) {      // (nBits, xi BigUint64Array(3), dLev)  stark_gen_helpers.js:216-231
    Args a(env, info); uint32_t nb = (uint32_t)a.u64(0); uint64_t *xi = a.arr(1, 3); uint64_t *lev = DP(2); if (!a.ok) return nullptr;
    P2(env, pil2gl_build_lev_dev(nb, xi, lev, a.stream(3))); return mk_undefined(env);
}
FN(ComputeEvalsDev) {  // (descs BigUint64Array(5*nEvals) = [dBuf,width,offset,dim,levIndex]*, nEvals, nBits, extendBits, levs BigUint64Array(nLev) device ptrs, out BigUint64Array(3*nEvals))
    Args a(env, info); uint64_t nEv = a.u64(1); uint64_t *d = a.arr(0, 5 * nEv); uint32_t nb = (uint32_t)a.u64(2), eb = (uint32_t)a.u64(3);
    uint64_t nLev = 0; uint64_t *levs = a.arr(4, 1, &nLev); uint64_t *out = a.arr(5, 3 * nEv); if (!a.ok) return nullptr;
    std::vector<pil2gl_eval_desc> descs(nEv);
    for (uint64_t i = 0; i < nEv; i++) { descs[i].buf = (const uint64_t *)(uintptr_t)d[5 * i]; descs[i].width = d[5 * i + 1]; descs[i].offset = d[5 * i + 2]; descs[i].dim = (uint32_t)d[5 * i + 3]; descs[i].levIndex = (uint32_t)d[5 * i + 4]; }
    std::vector<const uint64_t *> lp(nLev);
    for (uint64_t i = 0; i < nLev; i++) lp[i] = (const uint64_t *)(uintptr_t)levs[i];
    P2(env, pil2gl_compute_evals_dev(descs.data(), (uint32_t)nEv, nb, eb, lp.data(), (uint32_t)nLev, out, nullptr)); return mk_undefined(env);
}
// the two stages that are matrix-vector products (csrc/dot.hip): FRI polynomial as row sums, evaluations as column sums
FN(RowsDotExtDev) {    // (dBuf, width, nRows, coef BigUint64Array(nOut*width*3), nOut, dAcc, accumulate)
    Args a(env, info); uint64_t *buf = DP(0); uint64_t width = a.u64(1), nRows = a.u64(2); uint32_t nOut = (uint32_t)a.u64(4);
    uint64_t *coef = a.arr(3, (uint64_t)nOut * width * 3); uint64_t *acc = DP(5); int accumulate = (int)a.u64(6); if (!a.ok) return nullptr;
    P2(env, pil2gl_rows_dot_ext_dev(buf, width, nRows, coef, nOut, acc, accumulate, nullptr)); return mk_undefined(env);
}
FN(RowsDotExtMultiDev) {   // (dBufs BigUint64Array(n) device ptrs, widths BigUint64Array(n), nRows, coefs Array(n) of BigUint64Array(nOut*width*3), nOut, dAcc, accumulate)
    Args a(env, info); uint64_t n = 0; uint64_t *ptrs = a.arr(0, 1, &n); uint64_t *widths = a.arr(1, n); uint64_t nRows = a.u64(2);
    uint32_t nOut = (uint32_t)a.u64(4); uint64_t *acc = DP(5); int accumulate = (int)a.u64(6); if (!a.ok || n == 0 || n > 16) return nullptr;
    std::vector<const uint64_t *> bp(n), cp(n);
    for (uint64_t k = 0; k < n; k++) {
        bp[k] = (const uint64_t *)(uintptr_t)ptrs[k];
        napi_value el; if (napi_get_element(env, a.argv[3], (uint32_t)k, &el) != napi_ok) { napi_throw_error(env, nullptr, "coefs must be an array of BigUint64Array"); return nullptr; }
        napi_typedarray_type ty; size_t len; void *data; napi_value ab; size_t off;
        if (napi_get_typedarray_info(env, el, &ty, &len, &data, &ab, &off) != napi_ok || ty != napi_biguint64_array || len < (size_t)nOut * widths[k] * 3) {
            napi_throw_error(env, nullptr, "coefs[k] must be a BigUint64Array of nOut*width*3 words"); return nullptr; }
        cp[k] = (const uint64_t *)data;
    }
    P2(env, pil2gl_rows_dot_ext_multi_dev(bp.data(), widths, (uint32_t)n, nRows, cp.data(), nOut, acc, accumulate, nullptr)); return mk_undefined(env);
}
FN(FriCombineDev) {    // (dAcc, K BigUint64Array(nOpen*3), vf1 BigUint64Array(3), dXDivXSubXi, nOpen, nRows, dF[, order BigUint64Array(nOpen)])
    Args a(env, info); uint64_t *acc = DP(0); uint32_t nOpen = (uint32_t)a.u64(4); uint64_t *K = a.arr(1, 3ull * nOpen), *vf1 = a.arr(2, 3);
    uint64_t *x = DP(3); uint64_t nRows = a.u64(5); uint64_t *f = DP(6);
    uint32_t order[4] = { 0, 1, 2, 3 };
    if (!a.is_nullish(7)) { uint64_t *o = a.arr(7, nOpen); if (a.ok && nOpen <= 4) for (uint32_t k = 0; k < nOpen; k++) order[k] = (uint32_t)o[k]; }
    if (!a.ok) return nullptr;
    P2(env, pil2gl_fri_combine_order_dev(acc, K, vf1, x, nOpen, order, nRows, f, nullptr)); return mk_undefined(env);
}
FN(ColsDotExtDev) {    // (dBuf, width, nRows, rowStep, levs BigUint64Array(nLev) device ptrs, out BigUint64Array(nLev*width*3))
    Args a(env, info); uint64_t *buf = DP(0); uint64_t width = a.u64(1), nRows = a.u64(2), rowStep = a.u64(3);
    uint64_t nLev = 0; uint64_t *levs = a.arr(4, 1, &nLev); uint64_t *out = a.arr(5, nLev * width * 3); if (!a.ok) return nullptr;
    std::vector<const uint64_t *> lp(nLev);
    for (uint64_t i = 0; i < nLev; i++) lp[i] = (const uint64_t *)(uintptr_t)levs[i];
    P2(env, pil2gl_cols_dot_ext_dev(buf, width, nRows, rowStep, lp.data(), (uint32_t)nLev, out, nullptr)); return mk_undefined(env);
}
FN(ColsDotExtMultiDev) {   // (dBufs BigUint64Array(n) device ptrs, widths BigUint64Array(n), nRows, rowStep, levs BigUint64Array(nLev) device ptrs, outs Array(n) of BigUint64Array(nLev*width*3))
    Args a(env, info); uint64_t n = 0; uint64_t *ptrs = a.arr(0, 1, &n); uint64_t *widths = a.arr(1, n); uint64_t nRows = a.u64(2), rowStep = a.u64(3);
    uint64_t nLev = 0; uint64_t *levs = a.arr(4, 1, &nLev); if (!a.ok || n == 0 || n > 8) return nullptr;
    std::vector<const uint64_t *> bp(n), lp(nLev); std::vector<uint64_t *> op(n);
    for (uint64_t i = 0; i < nLev; i++) lp[i] = (const uint64_t *)(uintptr_t)levs[i];
    for (uint64_t k = 0; k < n; k++) {
        bp[k] = (const uint64_t *)(uintptr_t)ptrs[k];
        napi_value el; napi_typedarray_type ty; size_t len; void *data; napi_value ab; size_t off;
        if (napi_get_element(env, a.argv[5], (uint32_t)k, &el) != napi_ok || napi_get_typedarray_info(env, el, &ty, &len, &data, &ab, &off) != napi_ok ||
            ty != napi_biguint64_array || len < (size_t)nLev * widths[k] * 3) { napi_throw_error(env, nullptr, "outs[k] must be a BigUint64Array of nLev*width*3 words"); return nullptr; }
        op[k] = (uint64_t *)data;
    }
    P2(env, pil2gl_cols_dot_ext_multi_dev(bp.data(), widths, (uint32_t)n, nRows, rowStep, lp.data(), (uint32_t)nLev, op.data(), nullptr)); return mk_undefined(env);
}
FN(SynthFibonacciDev) { // (nBits, nPairs, init BigUint64Array(2*nPairs), dCm): synthetic witness for benchmarks (pil2gl.h)
    Args a(env, info); uint32_t nb = (uint32_t)a.u64(0), np = (uint32_t)a.u64(1); uint64_t *init = a.arr(2, 2ull * np); uint64_t *cm = DP(3); if (!a.ok) return nullptr;
    P2(env, pil2gl_synth_fibonacci_dev(nb, np, init, cm, nullptr)); return mk_undefined(env);
}
FN(GprodDev) {         // (dNum, dimNum, dDen, dimDen, n, dOut)  polutils.js:128-143
    Args a(env, info); uint64_t *num = DP(0); uint32_t dn = (uint32_t)a.u64(1); uint64_t *den = DP(2); uint32_t dd = (uint32_t)a.u64(3); uint64_t n = a.u64(4); uint64_t *o = DP(5); if (!a.ok) return nullptr;
    P2(env, pil2gl_gprod_dev(num, dn, den, dd, n, o, a.stream(6))); return mk_undefined(env);
}
FN(GsumDev) {          // (dNum (one element), dimNum, dDen, dimDen, n, dOut)  polutils.js:145-164
    Args a(env, info); uint64_t *num = DP(0); uint32_t dn = (uint32_t)a.u64(1); uint64_t *den = DP(2); uint32_t dd = (uint32_t)a.u64(3); uint64_t n = a.u64(4); uint64_t *o = DP(5); if (!a.ok) return nullptr;
    P2(env, pil2gl_gsum_dev(num, dn, den, dd, n, o, a.stream(6))); return mk_undefined(env);
}
FN(GsumColDev) {       // (dNum (n rows), dimNum, dDen, dimDen, n, dOut): gsum with a column numerator
    Args a(env, info); uint64_t *num = DP(0); uint32_t dn = (uint32_t)a.u64(1); uint64_t *den = DP(2); uint32_t dd = (uint32_t)a.u64(3); uint64_t n = a.u64(4); uint64_t *o = DP(5); if (!a.ok) return nullptr;
    P2(env, pil2gl_gsum_col_dev(num, dn, den, dd, n, o, a.stream(6))); return mk_undefined(env);
}
FN(H1H2Dev) {          // (dF, dT, n, dim, dH1, dH2)  polutils.js:105-126
    Args a(env, info); uint64_t *f = DP(0), *t = DP(1); uint64_t n = a.u64(2); uint32_t dim = (uint32_t)a.u64(3); uint64_t *h1 = DP(4), *h2 = DP(5); if (!a.ok) return nullptr;
    P2(env, pil2gl_h1h2_dev(f, t, n, dim, h1, h2, a.stream(6))); return mk_undefined(env);
}

// ---- recursion witness: the additions and the sMap gather of the *_exec step (csrc/wtns_exec.hip; js/witness_exec.js) ----
static napi_value mk_words(napi_env env, size_t nWords, uint64_t **data) {      // a new BigUint64Array
    napi_value ab, ta; void *p = nullptr;
    if (napi_create_arraybuffer(env, nWords * 8, &p, &ab) != napi_ok || napi_create_typedarray(env, napi_biguint64_array, nWords, ab, 0, &ta) != napi_ok) {
        napi_throw_error(env, nullptr, "cannot allocate a BigUint64Array of this length"); return nullptr; }
    *data = (uint64_t *)p;
    return ta;
}
// (addIdx, idxOffset, idxStride, nAdds, nWitness, coef, coefOffset, coefStride, coefWords) -> { nLevels, adds, coefs, levelStart }: the plan's
// 32-bit records and level table packed into BigUint64Arrays (two records' halves / two entries a word), ready for a DevBuffer
FN(WtnsAddsPlan) {
    Args a(env, info); uint64_t idxLen = 0, coefLen = 0;
    uint64_t *idx = a.arr(0, 0, &idxLen); uint64_t io = a.u64(1), is = a.u64(2), nAdds = a.u64(3), nWitness = a.u64(4);
    uint64_t *coef = a.arr(5, 0, &coefLen); uint64_t co = a.u64(6), cs = a.u64(7); uint32_t cw = (uint32_t)a.u64(8);
    if (!a.ok) return nullptr;
    if (nAdds && (is < 2 || io + (nAdds - 1) * is + 2 > idxLen || (cw != 1 && cw != 4) || co + (nAdds - 1) * cs + 2 * cw > coefLen)) {
        napi_throw_type_error(env, nullptr, "wtnsAddsPlan: the tables are shorter than nAdds additions"); return nullptr; }
    uint32_t nLevels = 0;
    P2(env, pil2gl_wtns_adds_plan(idx + io, is, nAdds, nWitness, nullptr, 0, cw, nullptr, nullptr, nullptr, 0, &nLevels));
    uint64_t *recs, *coefs, *starts;
    napi_value vr = mk_words(env, 2 * nAdds, &recs), vc = mk_words(env, 2 * cw * nAdds, &coefs), vs = mk_words(env, (nLevels + 2) / 2, &starts);
    if (!vr || !vc || !vs) return nullptr;
    starts[(nLevels + 2) / 2 - 1] = 0;
    P2(env, pil2gl_wtns_adds_plan(idx + io, is, nAdds, nWitness, coef + co, cs, cw, (uint32_t *)recs, coefs, (uint32_t *)starts, nLevels + 1, &nLevels));
    napi_value o, v; napi_create_object(env, &o);
    napi_create_uint32(env, nLevels, &v); napi_set_named_property(env, o, "nLevels", v);
    napi_set_named_property(env, o, "adds", vr); napi_set_named_property(env, o, "coefs", vc); napi_set_named_property(env, o, "levelStart", vs);
    return o;
}
FN(WtnsAddsDev) {          // (dW, nWitness, dAdds, dCoefs, nAdds, levelStart (the plan's packed array), nLevels, bn128[, stream])
    Args a(env, info); uint64_t *w = DP(0); uint64_t nWitness = a.u64(1); uint64_t *adds = DP(2), *coefs = DP(3); uint64_t nAdds = a.u64(4);
    uint64_t nLevels = a.u64(6); uint64_t *ls = a.arr(5, (nLevels + 2) / 2); bool bn = a.u64(7) != 0; if (!a.ok) return nullptr;
    P2(env, (bn ? pil2gl_bn128_wtns_adds_dev : pil2gl_wtns_adds_dev)(w, nWitness, (const uint32_t *)adds, coefs, nAdds, (const uint32_t *)ls, (uint32_t)nLevels, a.stream(8)));
    return mk_undefined(env);
}
FN(WtnsGatherDev) {        // (dW, nW, dSMap32, nRows, nCols, dDst, dstCols, bn128, toMontgomery, check[, stream]) -> first bad cell as BigInt (2^64-1: none), undefined without check
    Args a(env, info); uint64_t *w = DP(0); uint64_t nW = a.u64(1); uint64_t *sm = DP(2); uint64_t nRows = a.u64(3), nCols = a.u64(4); uint64_t *d = DP(5);
    uint64_t dc = a.u64(6); bool bn = a.u64(7) != 0; int mont = a.u64(8) != 0; bool check = a.u64(9) != 0; if (!a.ok) return nullptr;
    uint64_t bad = ~0ull;
    if (bn) P2(env, pil2gl_bn128_wtns_gather_dev(w, nW, (const uint32_t *)sm, nRows, nCols, d, dc, mont, check ? &bad : nullptr, a.stream(10)));
    else P2(env, pil2gl_wtns_gather_dev(w, nW, (const uint32_t *)sm, nRows, nCols, d, dc, check ? &bad : nullptr, a.stream(10)));
    return check ? mk_bigint(env, bad) : mk_undefined(env);
}
FN(WtnsExec) {             // (w, nWitness, addsBuff (a, b, ca, cb), nAdds, sMap, nRows, nCols, dst)   compressor_exec.js:17-29
    Args a(env, info); uint64_t nWitness = a.u64(1), nAdds = a.u64(3), nRows = a.u64(5), nCols = a.u64(6);
    uint64_t *w = a.arr(0, nWitness), *adds = a.arr(2, 4 * nAdds), *sm = a.arr(4, nRows * nCols), *d = a.arr(7, nRows * nCols); if (!a.ok) return nullptr;
    P2(env, pil2gl_wtns_exec(w, nWitness, adds, adds + 2, nAdds, sm, nRows, nCols, d)); return mk_undefined(env);
}
FN(Bn128WtnsExec) {        // (w, nWitness, addsIdx, addsCoef, nAdds, sMap, nRows, nCols, dst, toMontgomery)   main_final_exec.js:55-67
    Args a(env, info); uint64_t nWitness = a.u64(1), nAdds = a.u64(4), nRows = a.u64(6), nCols = a.u64(7);
    uint64_t *w = a.arr(0, 4 * nWitness), *idx = a.arr(2, 2 * nAdds), *coef = a.arr(3, 8 * nAdds), *sm = a.arr(5, nRows * nCols), *d = a.arr(8, 4 * nRows * nCols);
    int mont = a.u64(9) != 0; if (!a.ok) return nullptr;
    P2(env, pil2gl_bn128_wtns_exec(w, nWitness, idx, coef, nAdds, sm, nRows, nCols, d, mont)); return mk_undefined(env);
}

// ---- connection polynomials: the S columns of a recursion circuit from its sMap (csrc/conn_pols.hip; js/witness_exec.js) ----
FN(ConnPlan) {             // (nRows, nCols, nW, N, elemWords) -> { passes, threads, tile, sortBlocks, scanChunks, loBits, hiBits, launches, scratchBytes }
    Args a(env, info); uint64_t nRows = a.u64(0), nCols = a.u64(1), nW = a.u64(2), N = a.u64(3); uint32_t ew = (uint32_t)a.u64(4); if (!a.ok) return nullptr;
    uint32_t out[8]; uint64_t bytes = 0;
    P2(env, pil2gl_conn_plan(nRows, nCols, nW, N, ew, out, &bytes));
    static const char *names[8] = { "passes", "threads", "tile", "sortBlocks", "scanChunks", "loBits", "hiBits", "launches" };
    napi_value o, v; napi_create_object(env, &o);
    for (int i = 0; i < 8; i++) { napi_create_uint32(env, out[i], &v); napi_set_named_property(env, o, names[i], v); }
    napi_create_double(env, (double)bytes, &v); napi_set_named_property(env, o, "scratchBytes", v);
    return o;
}
// (dSMap32, nRows, nCols, nW, N, consts = w then ks1 (1 + nCols elements), dDst, dstStride, dstOffset, dScratch, scratchBytes, check)
//   -> first bad cell as BigInt (2^64-1: none), undefined without check
static napi_value conn_pols_dev(napi_env env, napi_callback_info info, uint32_t ew) {
    Args a(env, info); uint64_t *sm = DP(0); uint64_t nRows = a.u64(1), nCols = a.u64(2), nW = a.u64(3), N = a.u64(4);
    uint64_t *c = a.arr(5, ew * (1 + nCols)); uint64_t *d = DP(6); uint64_t stride = a.u64(7), off = a.u64(8); uint64_t *scr = DP(9);
    uint64_t bytes = a.u64(10); bool check = a.u64(11) != 0; if (!a.ok) return nullptr;
    uint64_t bad = ~0ull;
    P2(env, (ew == 4 ? pil2gl_bn128_conn_pols_dev : pil2gl_conn_pols_dev)((const uint32_t *)sm, nRows, nCols, nW, N, c, c + ew, d, stride, off, scr, bytes,
                                                                          check ? &bad : nullptr, nullptr));
    return check ? mk_bigint(env, bad) : mk_undefined(env);
}
FN(ConnPolsDev) { return conn_pols_dev(env, info, 1); }
FN(Bn128ConnPolsDev) { return conn_pols_dev(env, info, 4); }
// (sMap words, layout (0: nRows x nCols u64; 1: nCols arrays of N u32, packed two a word), nRows, nCols, nW, N, consts, dst (N nCols elements))
static napi_value conn_pols_host(napi_env env, napi_callback_info info, uint32_t ew) {
    Args a(env, info); int layout = (int)a.u64(1); uint64_t nRows = a.u64(2), nCols = a.u64(3), nW = a.u64(4), N = a.u64(5);
    uint64_t *sm = a.arr(0, layout == PIL2GL_CONN_SMAP_COLS_U32 ? (N * nCols + 1) / 2 : nRows * nCols);
    uint64_t *c = a.arr(6, ew * (1 + nCols)), *d = a.arr(7, ew * N * nCols); if (!a.ok) return nullptr;
    P2(env, (ew == 4 ? pil2gl_bn128_conn_pols : pil2gl_conn_pols)(sm, layout, nRows, nCols, nW, N, c, c + ew, d)); return mk_undefined(env);
}
FN(ConnPols) { return conn_pols_host(env, info, 1); }
FN(Bn128ConnPols) { return conn_pols_host(env, info, 4); }

// ---- connection check: does a trace meet {a} connect {S} (csrc/conn_check.hip; js/witness_exec.js) ----
FN(ConnCheckPlan) {        // (N, nCols, elemWords) -> { capBits, threads, loBits, hiBits, buildBlocks, checkBlocks, lanesPerCell, launches, scratchBytes }
    Args a(env, info); uint64_t N = a.u64(0), nCols = a.u64(1); uint32_t ew = (uint32_t)a.u64(2); if (!a.ok) return nullptr;
    uint32_t out[8]; uint64_t bytes = 0;
    P2(env, pil2gl_conn_check_plan(N, nCols, ew, out, &bytes));
    static const char *names[8] = { "capBits", "threads", "loBits", "hiBits", "buildBlocks", "checkBlocks", "lanesPerCell", "launches" };
    napi_value o, v; napi_create_object(env, &o);
    for (int i = 0; i < 8; i++) { napi_create_uint32(env, out[i], &v); napi_set_named_property(env, o, names[i], v); }
    napi_create_double(env, (double)bytes, &v); napi_set_named_property(env, o, "scratchBytes", v);
    return o;
}
// (dA, aStride, aOffset, dS, sStride, sOffset, N, nCols, consts = w then ks1 (1 + nCols elements), dScratch, scratchBytes, report BigUint64Array(3))
static napi_value conn_check_dev(napi_env env, napi_callback_info info, uint32_t ew) {
    Args a(env, info); uint64_t *da = DP(0); uint64_t as = a.u64(1), ao = a.u64(2); uint64_t *ds = DP(3); uint64_t ss = a.u64(4), so = a.u64(5);
    uint64_t N = a.u64(6), nCols = a.u64(7); uint64_t *c = a.arr(8, ew * (1 + nCols)); uint64_t *scr = DP(9); uint64_t bytes = a.u64(10);
    uint64_t *rep = a.arr(11, 3); if (!a.ok) return nullptr;
    P2(env, (ew == 4 ? pil2gl_bn128_conn_check_dev : pil2gl_conn_check_dev)(da, as, ao, ds, ss, so, N, nCols, c, c + ew, scr, bytes, rep, nullptr));
    return mk_undefined(env);
}
FN(ConnCheckDev) { return conn_check_dev(env, info, 1); }
FN(Bn128ConnCheckDev) { return conn_check_dev(env, info, 4); }
// (a, S (N nCols elements each, row-major), N, nCols, consts, report BigUint64Array(3))
static napi_value conn_check_host(napi_env env, napi_callback_info info, uint32_t ew) {
    Args a(env, info); uint64_t N = a.u64(2), nCols = a.u64(3);
    uint64_t *ha = a.arr(0, ew * N * nCols), *hs = a.arr(1, ew * N * nCols), *c = a.arr(4, ew * (1 + nCols)), *rep = a.arr(5, 3); if (!a.ok) return nullptr;
    P2(env, (ew == 4 ? pil2gl_bn128_conn_check : pil2gl_conn_check)(ha, hs, N, nCols, c, c + ew, rep)); return mk_undefined(env);
}
FN(ConnCheck) { return conn_check_host(env, info, 1); }
FN(Bn128ConnCheck) { return conn_check_host(env, info, 4); }

// ---- lookup and permutation checks: selF {f..} in / is selT {t..} as statements about the trace (csrc/tuple_check.hip; js/pil_checks.js) ----
// a plan entry's result: the six words under their names, and the byte count under its own
static napi_value plan_object(napi_env env, const char *const (&names)[6], const uint32_t (&out)[6], const char *bytesName, uint64_t bytes) {
    napi_value o, v; napi_create_object(env, &o);
    for (int i = 0; i < 6; i++) { napi_create_uint32(env, out[i], &v); napi_set_named_property(env, o, names[i], v); }
    napi_create_double(env, (double)bytes, &v); napi_set_named_property(env, o, bytesName, v);
    return o;
}
static const char *const TABLE_PLAN[6] = { "capBits", "threads", "blocks", "launches", "headerBytes", "slotBytes" };
FN(TupleCheckPlan) {       // (n, k, elemWords, mode) -> { capBits, threads, blocks, launches, headerBytes, slotBytes, scratchBytes }
    Args a(env, info); uint64_t n = a.u64(0), k = a.u64(1); uint32_t ew = (uint32_t)a.u64(2), mode = (uint32_t)a.u64(3); if (!a.ok) return nullptr;
    uint32_t out[6]; uint64_t bytes = 0;
    P2(env, pil2gl_tuple_check_plan(n, k, ew, mode, out, &bytes));
    return plan_object(env, TABLE_PLAN, out, "scratchBytes", bytes);
}
// A call's description, one BigUint64Array: [0] f, [1] fStride, [2] t, [3] tStride, [4] selF (0: none), [5] selFStride, [6] selFCol, [7] selT,
// [8] selTStride, [9] selTCol, [10] n, [11] k, [12] mode, then k columns of f and k columns of t.  The pointer words are device addresses
// for tupleCheckDev and are not read by tupleCheck, which takes the host matrices as arguments of their own.
enum { TD_F, TD_F_STRIDE, TD_T, TD_T_STRIDE, TD_SELF, TD_SELF_STRIDE, TD_SELF_COL, TD_SELT, TD_SELT_STRIDE, TD_SELT_COL, TD_N, TD_K, TD_MODE, TD_COLS };
static uint64_t *tuple_desc(Args &a, size_t i) {
    uint64_t len = 0; uint64_t *d = a.arr(i, TD_COLS, &len);
    if (a.ok && (d[TD_K] > 16 || len < TD_COLS + 2 * d[TD_K])) a.fail("the description holds 13 words and 2 k columns, k <= 16");
    return d;
}
// the words a host matrix must hold for the library to read it: 0 where the library refuses the shape before it reads anything
static uint64_t tuple_span(uint64_t n, uint64_t stride, const uint64_t *cols, uint64_t k, uint32_t ew) {
    uint64_t top = 0;
    for (uint64_t j = 0; j < k; j++) { if (cols[j] >= stride) return 0; top = cols[j] > top ? cols[j] : top; }
    return n && n <= (1ull << 28) && !(stride >> 32) && n * stride <= (1ull << 58) ? ((n - 1) * stride + top + 1) * ew : 0;
}
FN(TupleCheckDev) {        // (description, dScratch, scratchBytes, report BigUint64Array(5), elemWords)
    Args a(env, info); uint64_t *d = tuple_desc(a, 0); uint64_t *scr = DP(1); uint64_t bytes = a.u64(2); uint64_t *rep = a.arr(3, 5);
    uint32_t ew = (uint32_t)a.u64(4); if (!a.ok) return nullptr;
    const uint64_t k = d[TD_K];
    P2(env, (ew == 4 ? pil2gl_bn128_tuple_check_dev : pil2gl_tuple_check_dev)(
        (const uint64_t *)(uintptr_t)d[TD_F], d[TD_F_STRIDE], d + TD_COLS, (const uint64_t *)(uintptr_t)d[TD_T], d[TD_T_STRIDE], d + TD_COLS + k,
        (const uint64_t *)(uintptr_t)d[TD_SELF], d[TD_SELF_STRIDE], d[TD_SELF_COL], (const uint64_t *)(uintptr_t)d[TD_SELT], d[TD_SELT_STRIDE], d[TD_SELT_COL],
        d[TD_N], k, (uint32_t)d[TD_MODE], scr, bytes, rep, nullptr));
    return mk_undefined(env);
}
FN(TupleCheck) {           // (description, f, t, selF | null, selT | null, report BigUint64Array(5), elemWords): host matrices as BigUint64Array
    Args a(env, info); uint64_t *d = tuple_desc(a, 0); uint32_t ew = (uint32_t)a.u64(6); if (!a.ok) return nullptr;
    if (ew != 1 && ew != 4) { a.fail("elemWords is 1 or 4"); return nullptr; }
    const uint64_t k = d[TD_K], n = d[TD_N];
    uint64_t *f = a.arr(1, tuple_span(n, d[TD_F_STRIDE], d + TD_COLS, k, ew)), *t = a.arr(2, tuple_span(n, d[TD_T_STRIDE], d + TD_COLS + k, k, ew));
    uint64_t *sf = a.is_nullish(3) ? nullptr : a.arr(3, tuple_span(n, d[TD_SELF_STRIDE], d + TD_SELF_COL, 1, ew));
    uint64_t *st = a.is_nullish(4) ? nullptr : a.arr(4, tuple_span(n, d[TD_SELT_STRIDE], d + TD_SELT_COL, 1, ew));
    uint64_t *rep = a.arr(5, 5); if (!a.ok) return nullptr;
    P2(env, (ew == 4 ? pil2gl_bn128_tuple_check : pil2gl_tuple_check)(f, d[TD_F_STRIDE], d + TD_COLS, t, d[TD_T_STRIDE], d + TD_COLS + k, sf, d[TD_SELF_STRIDE],
                                                                      d[TD_SELF_COL], st, d[TD_SELT_STRIDE], d[TD_SELT_COL], n, k, (uint32_t)d[TD_MODE], rep));
    return mk_undefined(env);
}
FN(TupleHome) {            // (canonical words BigUint64Array(k elemWords), k, elemWords, capacity) -> the home slot as BigInt (2^64-1: refused)
    Args a(env, info); uint64_t k = a.u64(1); uint32_t ew = (uint32_t)a.u64(2); uint64_t cap = a.u64(3);
    uint64_t *w = a.arr(0, k <= 16 && ew <= 4 ? k * ew : 0); if (!a.ok) return nullptr;
    return mk_bigint(env, pil2gl_debug_tuple_home(w, k, ew, cap));
}
FN(TupleCheckProbe) { return mk_bigint(env, pil2gl_debug_tuple_check_probe()); }

// ---- lookup multiplicities: the logUp column m of `selF_s {f_s} in selT {t}` (csrc/lookup_mult.hip; js/pil_checks.js) ----
FN(LookupMultPlan) {       // (n, k, nF, elemWords) -> { capBits, threads, blocks, launches, headerBytes, slotBytes, scratchBytes }
    Args a(env, info); uint64_t n = a.u64(0), k = a.u64(1), nF = a.u64(2); uint32_t ew = (uint32_t)a.u64(3); if (!a.ok) return nullptr;
    uint32_t out[6]; uint64_t bytes = 0;
    P2(env, pil2gl_lookup_mult_plan(n, k, nF, ew, out, &bytes));
    return plan_object(env, TABLE_PLAN, out, "scratchBytes", bytes);
}
// A call's description, one BigUint64Array: [0] n, [1] k, [2] nF, [3] m, [4] mStride, [5] mCol, then 1 + nF sides of six words in
// pil2gl_tuple_side's order -- t first, then f_0 .. f_{nF-1}: base, stride, (unused: the columns' place), sel (0: none), selStride, selCol --
// then the sides' k columns each, in the same order.  The pointer words are device addresses for lookupMultDev and are not read by
// lookupMult, which takes the host matrices as an array of its own.
enum { MD_N, MD_K, MD_NF, MD_M, MD_M_STRIDE, MD_M_COL, MD_SIDES, MD_SIDE_WORDS = 6 };
struct MultDesc { uint64_t *d; uint64_t n, k, nF; pil2gl_tuple_side side[9]; };             // side[0]: t
static bool mult_desc(Args &a, size_t i, MultDesc &m) {
    uint64_t len = 0; m.d = a.arr(i, MD_SIDES, &len);
    if (!a.ok) return false;
    m.n = m.d[MD_N]; m.k = m.d[MD_K]; m.nF = m.d[MD_NF];
    if (m.k > 16 || m.nF > 8 || len < MD_SIDES + (1 + m.nF) * (MD_SIDE_WORDS + m.k)) return a.fail("the description holds 6 words, then 1 + nF sides of 6 words and k columns, k <= 16, nF <= 8");
    uint64_t *cols = m.d + MD_SIDES + (1 + m.nF) * MD_SIDE_WORDS;
    for (uint64_t s = 0; s <= m.nF; s++) {
        const uint64_t *w = m.d + MD_SIDES + s * MD_SIDE_WORDS;
        m.side[s] = pil2gl_tuple_side{ (const uint64_t *)(uintptr_t)w[0], w[1], cols + s * m.k, (const uint64_t *)(uintptr_t)w[3], w[4], w[5] };
    }
    return true;
}
FN(LookupMultDev) {        // (description, dScratch, scratchBytes, report BigUint64Array(4), elemWords)
    Args a(env, info); MultDesc m; if (!mult_desc(a, 0, m)) return nullptr;
    uint64_t *scr = DP(1); uint64_t bytes = a.u64(2); uint64_t *rep = a.arr(3, 4); uint32_t ew = (uint32_t)a.u64(4); if (!a.ok) return nullptr;
    P2(env, (ew == 4 ? pil2gl_bn128_lookup_mult_dev : pil2gl_lookup_mult_dev)(m.side + 1, m.nF, m.side, (uint64_t *)(uintptr_t)m.d[MD_M], m.d[MD_M_STRIDE], m.d[MD_M_COL],
                                                                              m.n, m.k, scr, bytes, rep, nullptr));
    return mk_undefined(env);
}
// element i of the Array `arr` as a BigUint64Array of at least minWords; optional: null / undefined give nullptr
static uint64_t *array_words(Args &a, napi_value arr, uint32_t i, uint64_t minWords, bool optional) {
    napi_env env = a.env;
    napi_value v; napi_valuetype t; napi_get_element(env, arr, i, &v); napi_typeof(env, v, &t);
    if (optional && (t == napi_undefined || t == napi_null)) return nullptr;
    bool is = false; napi_is_typedarray(env, v, &is);
    napi_typedarray_type ty = napi_int8_array; size_t n = 0; void *data = nullptr; napi_value ab; size_t off;
    if (is) napi_get_typedarray_info(env, v, &ty, &n, &data, &ab, &off);
    if (!is || (ty != napi_biguint64_array && ty != napi_bigint64_array)) { a.fail("expected a BigUint64Array"); return nullptr; }
    if (n < minWords) { a.fail("buffer too small"); return nullptr; }
    return (uint64_t *)data;
}
// The host matrices of a call, argument 1: an Array of BigUint64Array, [2 s] the matrix of side s of ks[s] columns, [2 s + 1] its selector's or
// null, [2 count] the matrix that is written in place, its highest column outTop.  Fills base and sel of every side -> the written matrix;
// nullptr after a.fail().  expected: what the entry says when the array's length is another
static uint64_t *host_matrices(Args &a, pil2gl_tuple_side *const *sides, const uint64_t *ks, uint64_t count, uint64_t n, uint64_t outStride, uint64_t outTop,
                               uint32_t ew, const char *expected) {
    bool isArray = false; uint32_t len = 0;
    if (a.argc < 2 || napi_is_array(a.env, a.argv[1], &isArray) != napi_ok || !isArray) { a.fail("expected an Array of matrices"); return nullptr; }
    napi_get_array_length(a.env, a.argv[1], &len);
    if (len != 2 * count + 1) { a.fail(expected); return nullptr; }
    for (uint64_t s = 0; s < count && a.ok; s++) {
        pil2gl_tuple_side &x = *sides[s];
        x.base = array_words(a, a.argv[1], (uint32_t)(2 * s), tuple_span(n, x.stride, x.hostCols, ks[s], ew), false);
        x.sel = a.ok ? array_words(a, a.argv[1], (uint32_t)(2 * s + 1), tuple_span(n, x.selStride, &x.selCol, 1, ew), true) : nullptr;
    }
    return a.ok ? array_words(a, a.argv[1], (uint32_t)(2 * count), tuple_span(n, outStride, &outTop, 1, ew), false) : nullptr;
}
// (description, matrices, report BigUint64Array(4), elemWords): matrices = an Array of BigUint64Array, [2 s] the matrix of side s (t first),
// [2 s + 1] its selector's or null, [2 (1 + nF)] m's matrix, which is written in place
FN(LookupMult) {
    Args a(env, info); MultDesc m; if (!mult_desc(a, 0, m)) return nullptr;
    uint64_t *rep = a.arr(2, 4); uint32_t ew = (uint32_t)a.u64(3); if (!a.ok) return nullptr;
    if (ew != 1 && ew != 4) { a.fail("elemWords is 1 or 4"); return nullptr; }
    pil2gl_tuple_side *sides[9]; uint64_t ks[9];
    for (uint64_t s = 0; s <= m.nF; s++) { sides[s] = &m.side[s]; ks[s] = m.k; }
    uint64_t *hm = host_matrices(a, sides, ks, 1 + m.nF, m.n, m.d[MD_M_STRIDE], m.d[MD_M_COL], ew, "expected a matrix and a selector or null for t and every f, then m's matrix");
    if (!a.ok) return nullptr;
    P2(env, (ew == 4 ? pil2gl_bn128_lookup_mult : pil2gl_lookup_mult)(m.side + 1, m.nF, m.side, hm, m.d[MD_M_STRIDE], m.d[MD_M_COL], m.n, m.k, rep));
    return mk_undefined(env);
}
FN(LookupMultProbe) { return mk_bigint(env, pil2gl_debug_lookup_mult_probe()); }

// ---- range-check multiplicities: the column m of `selF_s f_s in [lo, lo + size)` (csrc/range_mult.hip; js/pil_checks.js) ----
FN(RangeMultPlan) {        // (n, size, nF, elemWords, path | undefined) -> { path, threads, blocks, launches, headerBytes, ldsCounters, scratchBytes }
    Args a(env, info); uint64_t n = a.u64(0), size = a.u64(1), nF = a.u64(2); uint32_t ew = (uint32_t)a.u64(3);
    const uint32_t path = a.argc > 4 && !a.is_nullish(4) ? (uint32_t)a.u64(4) : 2; if (!a.ok) return nullptr;
    uint32_t out[6]; uint64_t bytes = 0;
    P2(env, pil2gl_debug_range_mult_plan(n, size, nF, ew, path, out, &bytes));
    static const char *const names[6] = { "path", "threads", "blocks", "launches", "headerBytes", "ldsCounters" };
    return plan_object(env, names, out, "scratchBytes", bytes);
}
// A call's description, one BigUint64Array: [0] n, [1] nF, [2] lo as a two's-complement word, [3] size, [4] row0, [5] m, [6] mStride,
// [7] mCol, then nF sides of six words in pil2gl_tuple_side's order, the column itself in the columns' place: base, stride, col, sel
// (0: none), selStride, selCol.  The pointer words are device addresses for rangeMultDev and are not read by rangeMult, which takes the
// host matrices as an array of its own.
enum { RD_N, RD_NF, RD_LO, RD_SIZE, RD_ROW0, RD_M, RD_M_STRIDE, RD_M_COL, RD_SIDES, RD_SIDE_WORDS = 6 };
struct RangeDesc { uint64_t *d; uint64_t n, nF; pil2gl_tuple_side side[8]; };
static bool range_desc(Args &a, size_t i, RangeDesc &r) {
    uint64_t len = 0; r.d = a.arr(i, RD_SIDES, &len);
    if (!a.ok) return false;
    r.n = r.d[RD_N]; r.nF = r.d[RD_NF];
    if (r.nF > 8 || len < RD_SIDES + r.nF * RD_SIDE_WORDS) return a.fail("the description holds 8 words, then nF sides of 6 words, nF <= 8");
    for (uint64_t s = 0; s < r.nF; s++) {
        const uint64_t *w = r.d + RD_SIDES + s * RD_SIDE_WORDS;
        r.side[s] = pil2gl_tuple_side{ (const uint64_t *)(uintptr_t)w[0], w[1], w + 2, (const uint64_t *)(uintptr_t)w[3], w[4], w[5] };
    }
    return true;
}
FN(RangeMultDev) {         // (description, dScratch, scratchBytes, report BigUint64Array(4), elemWords)
    Args a(env, info); RangeDesc r; if (!range_desc(a, 0, r)) return nullptr;
    uint64_t *scr = DP(1); uint64_t bytes = a.u64(2); uint64_t *rep = a.arr(3, 4); uint32_t ew = (uint32_t)a.u64(4); if (!a.ok) return nullptr;
    P2(env, (ew == 4 ? pil2gl_bn128_range_mult_dev : pil2gl_range_mult_dev)(r.side, r.nF, (int64_t)r.d[RD_LO], r.d[RD_SIZE], r.d[RD_ROW0], (uint64_t *)(uintptr_t)r.d[RD_M],
                                                                            r.d[RD_M_STRIDE], r.d[RD_M_COL], r.n, scr, bytes, rep, nullptr));
    return mk_undefined(env);
}
// (description, matrices, report BigUint64Array(4), elemWords): matrices = an Array of BigUint64Array, [2 s] the matrix of side s,
// [2 s + 1] its selector's or null, [2 nF] m's matrix, which is written in place
FN(RangeMult) {
    Args a(env, info); RangeDesc r; if (!range_desc(a, 0, r)) return nullptr;
    uint64_t *rep = a.arr(2, 4); uint32_t ew = (uint32_t)a.u64(3); if (!a.ok) return nullptr;
    if (ew != 1 && ew != 4) { a.fail("elemWords is 1 or 4"); return nullptr; }
    pil2gl_tuple_side *sides[8]; uint64_t ks[8];
    for (uint64_t s = 0; s < r.nF; s++) { sides[s] = &r.side[s]; ks[s] = 1; }
    uint64_t *hm = host_matrices(a, sides, ks, r.nF, r.n, r.d[RD_M_STRIDE], r.d[RD_M_COL], ew, "expected a matrix and a selector or null for every f, then m's matrix");
    if (!a.ok) return nullptr;
    P2(env, (ew == 4 ? pil2gl_bn128_range_mult : pil2gl_range_mult)(r.side, r.nF, (int64_t)r.d[RD_LO], r.d[RD_SIZE], r.d[RD_ROW0], hm, r.d[RD_M_STRIDE], r.d[RD_M_COL], r.n, rep));
    return mk_undefined(env);
}

// ---- multiplicity sessions: open, add, write (csrc/mult_session.hip; js/pil_checks.js LookupSession, RangeSession) ----
// The descriptions are the two above with the sides' row counts behind them: lookupMult's, then nF words hostRows (t first among the sides,
// as there; an open or a write gives nF = 0); rangeMult's with [0] = nM, then nF words hostRows.
static const char *const LOOKUP_SESSION_PLAN[6] = { "capBits", "threads", "blocks", "launches", "headerBytes", "slotBytes" };
static const char *const RANGE_SESSION_PLAN[6] = { "path", "threads", "blocks", "launches", "headerBytes", "counterBytes" };
FN(LookupSessionPlan) {    // (nT, k, elemWords) -> { capBits, threads, blocks, launches: open | add << 8 | write << 16, headerBytes, slotBytes, scratchBytes }
    Args a(env, info); uint64_t n = a.u64(0), k = a.u64(1); uint32_t ew = (uint32_t)a.u64(2); if (!a.ok) return nullptr;
    uint32_t out[6]; uint64_t bytes = 0;
    P2(env, pil2gl_lookup_session_plan(n, k, ew, out, &bytes));
    return plan_object(env, LOOKUP_SESSION_PLAN, out, "scratchBytes", bytes);
}
FN(RangeSessionPlan) {     // (size, elemWords) -> { path, threads, blocks, launches, headerBytes, counterBytes, scratchBytes }
    Args a(env, info); uint64_t size = a.u64(0); uint32_t ew = (uint32_t)a.u64(1); if (!a.ok) return nullptr;
    uint32_t out[6]; uint64_t bytes = 0;
    P2(env, pil2gl_range_session_plan(size, ew, out, &bytes));
    return plan_object(env, RANGE_SESSION_PLAN, out, "scratchBytes", bytes);
}
// the row counts behind a description of `used` words
static const uint64_t *session_rows(Args &a, size_t i, uint64_t used, uint64_t nF) {
    uint64_t len = 0; const uint64_t *d = a.arr(i, 1, &len);
    if (a.ok && len < used + nF) a.fail("the description ends before the sides' row counts");
    return a.ok ? d + used : nullptr;
}
FN(LookupSessionOpenDev) { // (description, dScratch, scratchBytes, elemWords)
    Args a(env, info); MultDesc m; if (!mult_desc(a, 0, m)) return nullptr;
    uint64_t *scr = DP(1); uint64_t bytes = a.u64(2); uint32_t ew = (uint32_t)a.u64(3); if (!a.ok) return nullptr;
    P2(env, (ew == 4 ? pil2gl_bn128_lookup_session_open_dev : pil2gl_lookup_session_open_dev)(m.side, m.n, m.k, scr, bytes, nullptr));
    return mk_undefined(env);
}
FN(LookupSessionAddDev) {  // (description, dScratch, scratchBytes, report BigUint64Array(4), elemWords)
    Args a(env, info); MultDesc m; if (!mult_desc(a, 0, m)) return nullptr;
    const uint64_t *rows = session_rows(a, 0, MD_SIDES + (1 + m.nF) * (MD_SIDE_WORDS + m.k), m.nF);
    uint64_t *scr = DP(1); uint64_t bytes = a.u64(2); uint64_t *rep = a.arr(3, 4); uint32_t ew = (uint32_t)a.u64(4); if (!a.ok) return nullptr;
    P2(env, (ew == 4 ? pil2gl_bn128_lookup_session_add_dev : pil2gl_lookup_session_add_dev)(m.side, m.n, m.k, m.side + 1, rows, m.nF, scr, bytes, rep, nullptr));
    return mk_undefined(env);
}
FN(LookupSessionWriteDev) {        // (description, dScratch, scratchBytes, elemWords) -> the session's matched rows
    Args a(env, info); MultDesc m; if (!mult_desc(a, 0, m)) return nullptr;
    uint64_t *scr = DP(1); uint64_t bytes = a.u64(2); uint32_t ew = (uint32_t)a.u64(3); if (!a.ok) return nullptr;
    uint64_t total = 0;
    P2(env, (ew == 4 ? pil2gl_bn128_lookup_session_write_dev : pil2gl_lookup_session_write_dev)(m.side, m.n, m.k, (uint64_t *)(uintptr_t)m.d[MD_M], m.d[MD_M_STRIDE],
                                                                                                m.d[MD_M_COL], scr, bytes, &total, nullptr));
    return mk_bigint(env, total);
}
FN(RangeSessionOpenDev) {  // (size, dScratch, scratchBytes)
    Args a(env, info); uint64_t size = a.u64(0); uint64_t *scr = DP(1); uint64_t bytes = a.u64(2); if (!a.ok) return nullptr;
    P2(env, pil2gl_range_session_open_dev(size, scr, bytes, nullptr));
    return mk_undefined(env);
}
FN(RangeSessionAddDev) {   // (description, dScratch, scratchBytes, report BigUint64Array(4), elemWords)
    Args a(env, info); RangeDesc r; if (!range_desc(a, 0, r)) return nullptr;
    const uint64_t *rows = session_rows(a, 0, RD_SIDES + r.nF * RD_SIDE_WORDS, r.nF);
    uint64_t *scr = DP(1); uint64_t bytes = a.u64(2); uint64_t *rep = a.arr(3, 4); uint32_t ew = (uint32_t)a.u64(4); if (!a.ok) return nullptr;
    P2(env, (ew == 4 ? pil2gl_bn128_range_session_add_dev : pil2gl_range_session_add_dev)((int64_t)r.d[RD_LO], r.d[RD_SIZE], r.side, rows, r.nF, scr, bytes, rep, nullptr));
    return mk_undefined(env);
}
FN(RangeSessionWriteDev) { // (description, dScratch, scratchBytes, elemWords) -> the session's matched rows
    Args a(env, info); RangeDesc r; if (!range_desc(a, 0, r)) return nullptr;
    uint64_t *scr = DP(1); uint64_t bytes = a.u64(2); uint32_t ew = (uint32_t)a.u64(3); if (!a.ok) return nullptr;
    uint64_t total = 0;
    P2(env, (ew == 4 ? pil2gl_bn128_range_session_write_dev : pil2gl_range_session_write_dev)(r.d[RD_SIZE], r.d[RD_ROW0], (uint64_t *)(uintptr_t)r.d[RD_M], r.d[RD_M_STRIDE],
                                                                                              r.d[RD_M_COL], r.n, scr, bytes, &total, nullptr));
    return mk_bigint(env, total);
}

// ---- lookup grand sum: the logUp column s from f, t and m (csrc/logup_sum_plan.h; js/pil_checks.js) ----
FN(LogupSumPlan) {         // (n, nTerms, elemWords) -> { threads, items, blocks, launches, depth, outWidth, workBytes }
    Args a(env, info); uint64_t n = a.u64(0), nT = a.u64(1); uint32_t ew = (uint32_t)a.u64(2); if (!a.ok) return nullptr;
    uint32_t out[6]; uint64_t bytes = 0;
    P2(env, pil2gl_logup_sum_plan(n, nT, ew, out, &bytes));
    static const char *const names[6] = { "threads", "items", "blocks", "launches", "depth", "outWidth" };
    return plan_object(env, names, out, "workBytes", bytes);
}
FN(LogupTermLayout) {      // -> { size, side, k, coef, busId }: sizeof and offsetof of pil2gl_logup_term as this addon was compiled
    static const char *names[5] = { "size", "side", "k", "coef", "busId" };
    const size_t at[5] = { sizeof(pil2gl_logup_term), offsetof(pil2gl_logup_term, side), offsetof(pil2gl_logup_term, k), offsetof(pil2gl_logup_term, coef),
                           offsetof(pil2gl_logup_term, busId) };
    napi_value o, v; napi_create_object(env, &o);
    for (int i = 0; i < 5; i++) { napi_create_uint32(env, (uint32_t)at[i], &v); napi_set_named_property(env, o, names[i], v); }
    return o;
}
// A call's description, one BigUint64Array: [0] n, [1] nTerms, [2] out, [3] outStride, [4] outCol, [5..8] alpha, [9..12] beta (three words
// used over Goldilocks), then nTerms terms of 14 words -- base, stride, k, sel (0: none), selStride, selCol, coef[4], busId[4] -- then 16
// column slots a term, the first k used.  The pointer words are device addresses for logupSumDev and are not read by logupSum, which
// takes the host matrices as an array of its own.
enum { LD_N, LD_NTERMS, LD_OUT, LD_OUT_STRIDE, LD_OUT_COL, LD_ALPHA, LD_BETA = LD_ALPHA + 4, LD_TERMS = LD_BETA + 4, LD_TERM_WORDS = 14, LD_COL_SLOTS = 16 };
struct LogupDesc { uint64_t *d; uint64_t n, nTerms; pil2gl_logup_term term[9]; };
static bool logup_desc(Args &a, size_t i, LogupDesc &L) {
    uint64_t len = 0; L.d = a.arr(i, LD_TERMS, &len);
    if (!a.ok) return false;
    L.n = L.d[LD_N]; L.nTerms = L.d[LD_NTERMS];
    if (L.nTerms < 1 || L.nTerms > 9 || len < LD_TERMS + L.nTerms * (LD_TERM_WORDS + LD_COL_SLOTS)) return a.fail("the description holds 13 words, then 1 .. 9 terms of 14 words and 16 column slots each");
    uint64_t *cols = L.d + LD_TERMS + L.nTerms * LD_TERM_WORDS;
    for (uint64_t u = 0; u < L.nTerms; u++) {
        const uint64_t *w = L.d + LD_TERMS + u * LD_TERM_WORDS;
        pil2gl_logup_term &t = L.term[u];
        t.side = pil2gl_tuple_side{ (const uint64_t *)(uintptr_t)w[0], w[1], cols + u * LD_COL_SLOTS, (const uint64_t *)(uintptr_t)w[3], w[4], w[5] };
        t.k = w[2];
        for (int c = 0; c < 4; c++) { t.coef[c] = w[6 + c]; t.busId[c] = w[10 + c]; }
    }
    return true;
}
FN(LogupSumDev) {          // (description, elemWords[, stream]): only enqueues
    Args a(env, info); LogupDesc L; if (!logup_desc(a, 0, L)) return nullptr;
    uint32_t ew = (uint32_t)a.u64(1); if (!a.ok) return nullptr;
    P2(env, (ew == 4 ? pil2gl_bn128_logup_sum_dev : pil2gl_logup_sum_dev)(L.term, L.nTerms, L.d + LD_ALPHA, L.d + LD_BETA, (uint64_t *)(uintptr_t)L.d[LD_OUT], L.d[LD_OUT_STRIDE],
                                                                          L.d[LD_OUT_COL], L.n, a.stream(2)));
    return mk_undefined(env);
}
// (description, matrices, elemWords): matrices = an Array of BigUint64Array, [2 u] the matrix of term u, [2 u + 1] its numerator's or null,
// [2 nTerms] out's matrix, which is written in place
FN(LogupSum) {
    Args a(env, info); LogupDesc L; if (!logup_desc(a, 0, L)) return nullptr;
    uint32_t ew = (uint32_t)a.u64(2); if (!a.ok) return nullptr;
    if (ew != 1 && ew != 4) { a.fail("elemWords is 1 or 4"); return nullptr; }
    pil2gl_tuple_side *sides[9]; uint64_t ks[9];
    for (uint64_t u = 0; u < L.nTerms; u++) {
        sides[u] = &L.term[u].side; ks[u] = L.term[u].k;
        if (ks[u] < 1 || ks[u] > 16) { a.fail("k must be 1 .. 16 columns"); return nullptr; }
    }
    uint64_t *ho = host_matrices(a, sides, ks, L.nTerms, L.n, L.d[LD_OUT_STRIDE], L.d[LD_OUT_COL] + (ew == 1 ? 2 : 0), ew,
                                 "expected a matrix and a numerator's matrix or null for every term, then out's matrix");
    if (!a.ok) return nullptr;
    P2(env, (ew == 4 ? pil2gl_bn128_logup_sum : pil2gl_logup_sum)(L.term, L.nTerms, L.d + LD_ALPHA, L.d + LD_BETA, ho, L.d[LD_OUT_STRIDE], L.d[LD_OUT_COL], L.n));
    return mk_undefined(env);
}

// ---- range-check grand sum: the logUp column s from f, m and the ranges as numbers (csrc/range_sum_plan.h; js/pil_checks.js) ----
FN(RangeSumPlan) {         // (n, nF, nR, elemWords) -> { threads, items, blocks, launches, depth, outWidth, workBytes }
    Args a(env, info); uint64_t n = a.u64(0), nF = a.u64(1), nR = a.u64(2); uint32_t ew = (uint32_t)a.u64(3); if (!a.ok) return nullptr;
    uint32_t out[6]; uint64_t bytes = 0;
    P2(env, pil2gl_range_sum_plan(n, nF, nR, ew, out, &bytes));
    static const char *const names[6] = { "threads", "items", "blocks", "launches", "depth", "outWidth" };
    return plan_object(env, names, out, "workBytes", bytes);
}
FN(RangeTermLayout) {      // -> sizeof and offsetof of pil2gl_range_term as this addon was compiled
    static const char *names[9] = { "size", "m", "mStride", "mCol", "lo", "rangeSize", "row0", "coef", "busId" };
    const size_t at[9] = { sizeof(pil2gl_range_term), offsetof(pil2gl_range_term, m), offsetof(pil2gl_range_term, mStride), offsetof(pil2gl_range_term, mCol),
                           offsetof(pil2gl_range_term, lo), offsetof(pil2gl_range_term, size), offsetof(pil2gl_range_term, row0), offsetof(pil2gl_range_term, coef),
                           offsetof(pil2gl_range_term, busId) };
    napi_value o, v; napi_create_object(env, &o);
    for (int i = 0; i < 9; i++) { napi_create_uint32(env, (uint32_t)at[i], &v); napi_set_named_property(env, o, names[i], v); }
    return o;
}
// A call's description, one BigUint64Array: [0] n, [1] nF, [2] nR, [3] out, [4] outStride, [5] outCol, [6..9] alpha, [10..13] beta (three
// words used over Goldilocks), then nF terms of logupSum's 14 words, then nR ranges of 14 words -- m, mStride, mCol, lo as a
// two's-complement word, size, row0, coef[4], busId[4] -- then 16 column slots an f term, the first k used.  The pointer words are device
// addresses for rangeSumDev and are not read by rangeSum, which takes the host matrices as an array of its own.
enum { SD_N, SD_NF, SD_NR, SD_OUT, SD_OUT_STRIDE, SD_OUT_COL, SD_ALPHA, SD_BETA = SD_ALPHA + 4, SD_TERMS = SD_BETA + 4, SD_TERM_WORDS = 14, SD_COL_SLOTS = 16 };
// the 14 words of an f term (its columns in slots of their own) and of a range
static void term_of_words(const uint64_t *w, const uint64_t *cols, pil2gl_logup_term &t) {
    t.side = pil2gl_tuple_side{ (const uint64_t *)(uintptr_t)w[0], w[1], cols, (const uint64_t *)(uintptr_t)w[3], w[4], w[5] };
    t.k = w[2];
    for (int c = 0; c < 4; c++) { t.coef[c] = w[6 + c]; t.busId[c] = w[10 + c]; }
}
static void range_of_words(const uint64_t *w, pil2gl_range_term &t) {
    t.m = (const uint64_t *)(uintptr_t)w[0]; t.mStride = w[1]; t.mCol = w[2]; t.lo = (int64_t)w[3]; t.size = w[4]; t.row0 = w[5];
    for (int c = 0; c < 4; c++) { t.coef[c] = w[6 + c]; t.busId[c] = w[10 + c]; }
}
struct RangeSumDesc { uint64_t *d; uint64_t n, nF, nR; pil2gl_logup_term term[8]; pil2gl_range_term range[8]; };
static bool range_sum_desc(Args &a, size_t i, RangeSumDesc &L) {
    uint64_t len = 0; L.d = a.arr(i, SD_TERMS, &len);
    if (!a.ok) return false;
    L.n = L.d[SD_N]; L.nF = L.d[SD_NF]; L.nR = L.d[SD_NR];
    if (L.nF > 8 || L.nR < 1 || L.nR > 8 || len < SD_TERMS + (L.nF + L.nR) * SD_TERM_WORDS + L.nF * SD_COL_SLOTS)
        return a.fail("the description holds 14 words, then 0 .. 8 terms and 1 .. 8 ranges of 14 words, then 16 column slots a term");
    uint64_t *cols = L.d + SD_TERMS + (L.nF + L.nR) * SD_TERM_WORDS;
    for (uint64_t u = 0; u < L.nF; u++) term_of_words(L.d + SD_TERMS + u * SD_TERM_WORDS, cols + u * SD_COL_SLOTS, L.term[u]);
    for (uint64_t r = 0; r < L.nR; r++) range_of_words(L.d + SD_TERMS + (L.nF + r) * SD_TERM_WORDS, L.range[r]);
    return true;
}
FN(RangeSumDev) {          // (description, elemWords[, stream]): only enqueues
    Args a(env, info); RangeSumDesc L; if (!range_sum_desc(a, 0, L)) return nullptr;
    uint32_t ew = (uint32_t)a.u64(1); if (!a.ok) return nullptr;
    P2(env, (ew == 4 ? pil2gl_bn128_range_sum_dev : pil2gl_range_sum_dev)(L.term, L.nF, L.range, L.nR, L.d + SD_ALPHA, L.d + SD_BETA, (uint64_t *)(uintptr_t)L.d[SD_OUT],
                                                                          L.d[SD_OUT_STRIDE], L.d[SD_OUT_COL], L.n, a.stream(2)));
    return mk_undefined(env);
}
// (description, matrices, elemWords): matrices = an Array of BigUint64Array, [2 u] the matrix of term u, [2 u + 1] its numerator's or null,
// [2 (nF + r)] the m matrix of range r, [2 (nF + r) + 1] null, [2 (nF + nR)] out's matrix, which is written in place
FN(RangeSum) {
    Args a(env, info); RangeSumDesc L; if (!range_sum_desc(a, 0, L)) return nullptr;
    uint32_t ew = (uint32_t)a.u64(2); if (!a.ok) return nullptr;
    if (ew != 1 && ew != 4) { a.fail("elemWords is 1 or 4"); return nullptr; }
    pil2gl_tuple_side mSide[8] = {};
    pil2gl_tuple_side *sides[16]; uint64_t ks[16];
    for (uint64_t u = 0; u < L.nF; u++) {
        sides[u] = &L.term[u].side; ks[u] = L.term[u].k;
        if (ks[u] < 1 || ks[u] > 16) { a.fail("k must be 1 .. 16 columns"); return nullptr; }
    }
    for (uint64_t r = 0; r < L.nR; r++) {            // an m column as a side of one column without a selector
        mSide[r].stride = L.range[r].mStride; mSide[r].hostCols = &L.range[r].mCol;
        sides[L.nF + r] = &mSide[r]; ks[L.nF + r] = 1;
    }
    uint64_t *ho = host_matrices(a, sides, ks, L.nF + L.nR, L.n, L.d[SD_OUT_STRIDE], L.d[SD_OUT_COL] + (ew == 1 ? 2 : 0), ew,
                                 "expected a matrix and a numerator's matrix or null for every term, m's matrix and null for every range, then out's matrix");
    if (!a.ok) return nullptr;
    for (uint64_t r = 0; r < L.nR; r++) L.range[r].m = mSide[r].base;
    P2(env, (ew == 4 ? pil2gl_bn128_range_sum : pil2gl_range_sum)(L.term, L.nF, L.range, L.nR, L.d + SD_ALPHA, L.d + SD_BETA, ho, L.d[SD_OUT_STRIDE], L.d[SD_OUT_COL], L.n));
    return mk_undefined(env);
}

// ---- clustered logUp sum: the im columns and s in one call (csrc/logup_cluster_plan.h; js/pil_checks.js) ----
FN(LogupClusterPlan) {     // (n, nF, nR, nIm, elemWords) -> { threads, items, blocks, launches, depth, outWidth, workBytes }
    Args a(env, info); uint64_t n = a.u64(0), nF = a.u64(1), nR = a.u64(2), nIm = a.u64(3); uint32_t ew = (uint32_t)a.u64(4); if (!a.ok) return nullptr;
    uint32_t out[6]; uint64_t bytes = 0;
    P2(env, pil2gl_logup_cluster_plan(n, nF, nR, nIm, ew, out, &bytes));
    static const char *const names[6] = { "threads", "items", "blocks", "launches", "depth", "outWidth" };
    return plan_object(env, names, out, "workBytes", bytes);
}
FN(LogupImColLayout) {     // -> sizeof and offsetof of pil2gl_logup_im_col as this addon was compiled
    static const char *names[4] = { "size", "base", "stride", "col" };
    const size_t at[4] = { sizeof(pil2gl_logup_im_col), offsetof(pil2gl_logup_im_col, base), offsetof(pil2gl_logup_im_col, stride), offsetof(pil2gl_logup_im_col, col) };
    napi_value o, v; napi_create_object(env, &o);
    for (int i = 0; i < 4; i++) { napi_create_uint32(env, (uint32_t)at[i], &v); napi_set_named_property(env, o, names[i], v); }
    return o;
}
// A call's description, one BigUint64Array: [0] n, [1] nF, [2] nR, [3] nIm, [4] out, [5] outStride, [6] outCol, [7..10] alpha, [11..14] beta
// (three words used over Goldilocks), then nF terms and nR ranges of rangeSum's 14 words, then nF + nR cluster words (all ones: DIRECT),
// then nIm im columns of three words -- base, stride, col -- then 16 column slots an f term.  The pointer words are device addresses for
// logupClusterDev and are not read by logupCluster, which takes the host matrices as an array of its own.
enum { CD_N, CD_NF, CD_NR, CD_NIM, CD_OUT, CD_OUT_STRIDE, CD_OUT_COL, CD_ALPHA, CD_BETA = CD_ALPHA + 4, CD_TERMS = CD_BETA + 4 };
struct ClusterDesc { uint64_t *d; uint64_t n, nF, nR, nIm; pil2gl_logup_term term[8]; pil2gl_range_term range[8]; const uint64_t *cluster; pil2gl_logup_im_col im[9]; };
static bool cluster_desc(Args &a, size_t i, ClusterDesc &L) {
    uint64_t len = 0; L.d = a.arr(i, CD_TERMS, &len);
    if (!a.ok) return false;
    L.n = L.d[CD_N]; L.nF = L.d[CD_NF]; L.nR = L.d[CD_NR]; L.nIm = L.d[CD_NIM];
    if (L.nF > 8 || L.nR > 8 || L.nIm > 9 || len < CD_TERMS + (L.nF + L.nR) * (SD_TERM_WORDS + 1) + 3 * L.nIm + L.nF * SD_COL_SLOTS)
        return a.fail("the description holds 15 words, then 0 .. 8 terms and 0 .. 8 ranges of 14 words, a cluster word each, 0 .. 9 im columns of 3 words, then 16 column slots a term");
    uint64_t *cl = L.d + CD_TERMS + (L.nF + L.nR) * SD_TERM_WORDS, *im = cl + L.nF + L.nR, *cols = im + 3 * L.nIm;
    for (uint64_t u = 0; u < L.nF; u++) term_of_words(L.d + CD_TERMS + u * SD_TERM_WORDS, cols + u * SD_COL_SLOTS, L.term[u]);
    for (uint64_t r = 0; r < L.nR; r++) range_of_words(L.d + CD_TERMS + (L.nF + r) * SD_TERM_WORDS, L.range[r]);
    L.cluster = cl;
    for (uint64_t c = 0; c < L.nIm; c++) L.im[c] = pil2gl_logup_im_col{ (uint64_t *)(uintptr_t)im[3 * c], im[3 * c + 1], im[3 * c + 2] };
    return true;
}
FN(LogupClusterDev) {      // (description, elemWords[, stream]): only enqueues
    Args a(env, info); ClusterDesc L; if (!cluster_desc(a, 0, L)) return nullptr;
    uint32_t ew = (uint32_t)a.u64(1); if (!a.ok) return nullptr;
    P2(env, (ew == 4 ? pil2gl_bn128_logup_cluster_dev : pil2gl_logup_cluster_dev)(L.term, L.nF, L.range, L.nR, L.cluster, L.im, L.nIm, L.d + CD_ALPHA, L.d + CD_BETA,
                                                                                  (uint64_t *)(uintptr_t)L.d[CD_OUT], L.d[CD_OUT_STRIDE], L.d[CD_OUT_COL], L.n, a.stream(2)));
    return mk_undefined(env);
}
// (description, matrices, elemWords): matrices = an Array of BigUint64Array, [2 u] the matrix of term u, [2 u + 1] its numerator's or null,
// [2 (nF + r)] the m matrix of range r and null, [2 (nF + nR + c)] the matrix of im column c and null, then out's matrix; the output
// matrices are written in place, and outputs of ONE matrix must be given as one array
FN(LogupCluster) {
    Args a(env, info); ClusterDesc L; if (!cluster_desc(a, 0, L)) return nullptr;
    uint32_t ew = (uint32_t)a.u64(2); if (!a.ok) return nullptr;
    if (ew != 1 && ew != 4) { a.fail("elemWords is 1 or 4"); return nullptr; }
    const uint64_t wide = ew == 1 ? 2 : 0;
    pil2gl_tuple_side one[17] = {};                  // an m column, an im element's highest word column: sides of one column without a selector
    uint64_t top[9];
    pil2gl_tuple_side *sides[25]; uint64_t ks[25];
    for (uint64_t u = 0; u < L.nF; u++) {
        sides[u] = &L.term[u].side; ks[u] = L.term[u].k;
        if (ks[u] < 1 || ks[u] > 16) { a.fail("k must be 1 .. 16 columns"); return nullptr; }
    }
    for (uint64_t r = 0; r < L.nR; r++) {
        one[r].stride = L.range[r].mStride; one[r].hostCols = &L.range[r].mCol;
        sides[L.nF + r] = &one[r]; ks[L.nF + r] = 1;
    }
    for (uint64_t c = 0; c < L.nIm; c++) {
        top[c] = L.im[c].col + wide;
        one[8 + c].stride = L.im[c].stride; one[8 + c].hostCols = &top[c];
        sides[L.nF + L.nR + c] = &one[8 + c]; ks[L.nF + L.nR + c] = 1;
    }
    uint64_t *ho = host_matrices(a, sides, ks, L.nF + L.nR + L.nIm, L.n, L.d[CD_OUT_STRIDE], L.d[CD_OUT_COL] + wide, ew,
                                 "expected a matrix and a numerator's matrix or null for every term, a matrix and null for every range and every im column, then out's matrix");
    if (!a.ok) return nullptr;
    for (uint64_t r = 0; r < L.nR; r++) L.range[r].m = one[r].base;
    for (uint64_t c = 0; c < L.nIm; c++) L.im[c].base = (uint64_t *)one[8 + c].base;
    P2(env, (ew == 4 ? pil2gl_bn128_logup_cluster : pil2gl_logup_cluster)(L.term, L.nF, L.range, L.nR, L.cluster, L.im, L.nIm, L.d + CD_ALPHA, L.d + CD_BETA, ho,
                                                                          L.d[CD_OUT_STRIDE], L.d[CD_OUT_COL], L.n));
    return mk_undefined(env);
}

// ---- grand product: the column z of a permutation or a connection (csrc/grand_prod_plan.h; js/pil_checks.js) ----
FN(GrandProdPlan) {        // (n, nTerms, sumK, elemWords) -> { threads, items, blocks, launches, depth, outWidth, workBytes }
    Args a(env, info); uint64_t n = a.u64(0), nT = a.u64(1), sumK = a.u64(2); uint32_t ew = (uint32_t)a.u64(3); if (!a.ok) return nullptr;
    uint32_t out[6]; uint64_t bytes = 0;
    P2(env, pil2gl_grand_prod_plan(n, nT, sumK, ew, out, &bytes));
    static const char *const names[6] = { "threads", "items", "blocks", "launches", "depth", "outWidth" };
    return plan_object(env, names, out, "workBytes", bytes);
}
FN(GrandProdTermLayout) {  // -> sizeof and offsetof of pil2gl_grand_prod_term as this addon was compiled
    static const char *names[8] = { "size", "side", "k", "den", "id", "idStride", "idCol", "idCoef" };
    typedef pil2gl_grand_prod_term T;
    const size_t at[8] = { sizeof(T), offsetof(T, side), offsetof(T, k), offsetof(T, den), offsetof(T, id), offsetof(T, idStride), offsetof(T, idCol), offsetof(T, idCoef) };
    napi_value o, v; napi_create_object(env, &o);
    for (int i = 0; i < 8; i++) { napi_create_uint32(env, (uint32_t)at[i], &v); napi_set_named_property(env, o, names[i], v); }
    return o;
}
// A call's description, one BigUint64Array: [0] n, [1] nTerms, [2] out, [3] outStride, [4] outCol, [5..8] alpha, [9..12] beta, [13..16] gamma
// (three words used over Goldilocks), then nTerms terms of 14 words -- base, stride, k, sel (0: none), selStride, selCol, den, id (0: none),
// idStride, idCol, idCoef[4] -- then 16 column slots a term, the first k used.  The pointer words are device addresses for grandProdDev
// and are not read by grandProd, which takes the host matrices as an array of its own.
enum { GD_N, GD_NTERMS, GD_OUT, GD_OUT_STRIDE, GD_OUT_COL, GD_ALPHA, GD_BETA = GD_ALPHA + 4, GD_GAMMA = GD_BETA + 4, GD_TERMS = GD_GAMMA + 4, GD_TERM_WORDS = 14,
       GD_COL_SLOTS = 16, GD_MAX_TERMS = 40 };
struct GrandProdDesc { uint64_t *d; uint64_t n, nTerms; pil2gl_grand_prod_term term[GD_MAX_TERMS]; };
static bool grand_prod_desc(Args &a, size_t i, GrandProdDesc &G) {
    uint64_t len = 0; G.d = a.arr(i, GD_TERMS, &len);
    if (!a.ok) return false;
    G.n = G.d[GD_N]; G.nTerms = G.d[GD_NTERMS];
    if (G.nTerms < 1 || G.nTerms > GD_MAX_TERMS || len < GD_TERMS + G.nTerms * (GD_TERM_WORDS + GD_COL_SLOTS))
        return a.fail("the description holds 17 words, then 1 .. 40 terms of 14 words and 16 column slots each");
    uint64_t *cols = G.d + GD_TERMS + G.nTerms * GD_TERM_WORDS;
    for (uint64_t u = 0; u < G.nTerms; u++) {
        const uint64_t *w = G.d + GD_TERMS + u * GD_TERM_WORDS;
        pil2gl_grand_prod_term &t = G.term[u];
        t.side = pil2gl_tuple_side{ (const uint64_t *)(uintptr_t)w[0], w[1], cols + u * GD_COL_SLOTS, (const uint64_t *)(uintptr_t)w[3], w[4], w[5] };
        t.k = w[2]; t.den = w[6]; t.id = (const uint64_t *)(uintptr_t)w[7]; t.idStride = w[8]; t.idCol = w[9];
        for (int c = 0; c < 4; c++) t.idCoef[c] = w[10 + c];
    }
    return true;
}
FN(GrandProdDev) {         // (description, elemWords[, stream]): only enqueues
    Args a(env, info); GrandProdDesc G; if (!grand_prod_desc(a, 0, G)) return nullptr;
    uint32_t ew = (uint32_t)a.u64(1); if (!a.ok) return nullptr;
    P2(env, (ew == 4 ? pil2gl_bn128_grand_prod_dev : pil2gl_grand_prod_dev)(G.term, G.nTerms, G.d + GD_ALPHA, G.d + GD_BETA, G.d + GD_GAMMA, (uint64_t *)(uintptr_t)G.d[GD_OUT],
                                                                            G.d[GD_OUT_STRIDE], G.d[GD_OUT_COL], G.n, a.stream(2)));
    return mk_undefined(env);
}
// (description, matrices, elemWords): matrices = an Array of BigUint64Array, four a term -- [4 u] the term's matrix, [4 u + 1] its selector's
// or null, [4 u + 2] the term's matrix again, [4 u + 3] its id column's or null -- then out's matrix, which is written in place: the id
// column travels through host_matrices as the selector of a second side over the same matrix
FN(GrandProd) {
    Args a(env, info); GrandProdDesc G; if (!grand_prod_desc(a, 0, G)) return nullptr;
    uint32_t ew = (uint32_t)a.u64(2); if (!a.ok) return nullptr;
    if (ew != 1 && ew != 4) { a.fail("elemWords is 1 or 4"); return nullptr; }
    pil2gl_tuple_side ids[GD_MAX_TERMS], *sides[2 * GD_MAX_TERMS]; uint64_t ks[2 * GD_MAX_TERMS];
    for (uint64_t u = 0; u < G.nTerms; u++) {
        pil2gl_grand_prod_term &t = G.term[u];
        if (t.k < 1 || t.k > 16) { a.fail("k must be 1 .. 16 columns"); return nullptr; }
        ids[u] = t.side; ids[u].selStride = t.idStride; ids[u].selCol = t.idCol;
        sides[2 * u] = &t.side; sides[2 * u + 1] = &ids[u]; ks[2 * u] = ks[2 * u + 1] = t.k;
    }
    uint64_t *ho = host_matrices(a, sides, ks, 2 * G.nTerms, G.n, G.d[GD_OUT_STRIDE], G.d[GD_OUT_COL] + (ew == 1 ? 2 : 0), ew,
                                 "expected a matrix, a selector's or null, the matrix again and an id column's or null for every term, then out's matrix");
    if (!a.ok) return nullptr;
    for (uint64_t u = 0; u < G.nTerms; u++) G.term[u].id = ids[u].sel;
    P2(env, (ew == 4 ? pil2gl_bn128_grand_prod : pil2gl_grand_prod)(G.term, G.nTerms, G.d + GD_ALPHA, G.d + GD_BETA, G.d + GD_GAMMA, ho, G.d[GD_OUT_STRIDE], G.d[GD_OUT_COL], G.n));
    return mk_undefined(env);
}

// ---- plookup: the fold of F and T and the column z from f, t, h1 and h2 (csrc/plookup_plan.h; js/pil_checks.js) ----
FN(PlookupPlan) {          // (n, kF, kT, elemWords) -> { threads, items, blocks, launches, depth, outWidth, workBytes }
    Args a(env, info); uint64_t n = a.u64(0), kF = a.u64(1), kT = a.u64(2); uint32_t ew = (uint32_t)a.u64(3); if (!a.ok) return nullptr;
    uint32_t out[6]; uint64_t bytes = 0;
    P2(env, pil2gl_plookup_plan(n, kF, kT, ew, out, &bytes));
    static const char *const names[6] = { "threads", "items", "blocks", "launches", "depth", "outWidth" };
    return plan_object(env, names, out, "workBytes", bytes);
}
// A call's description, one BigUint64Array: [0] n, [1] kF, [2] kT, [3] hDim, [4..7] alpha, [8..11] beta, [12..15] gamma, [16..19] delta (three
// words used over Goldilocks; the fold reads no gamma and delta), then f and t as five words each -- base, stride, sel (0: none), selStride,
// selCol -- then three columns of three words each -- base, stride, col: the product's h1, h2 and out, the fold's outF and outT (the third
// unused) -- then 16 column slots for f and 16 for t, the first k used.  The pointer words are device addresses for the Dev entries and are
// not read by the others, which take the host matrices as an array of their own.
enum { PD_N, PD_KF, PD_KT, PD_HDIM, PD_ALPHA, PD_BETA = PD_ALPHA + 4, PD_GAMMA = PD_BETA + 4, PD_DELTA = PD_GAMMA + 4, PD_F = PD_DELTA + 4, PD_T = PD_F + 5,
       PD_COLS = PD_T + 5, PD_F_SLOTS = PD_COLS + 9, PD_T_SLOTS = PD_F_SLOTS + 16, PD_WORDS = PD_T_SLOTS + 16 };
struct PlookupDesc { uint64_t *d; uint64_t n, kF, kT; uint32_t hDim; pil2gl_tuple_side f, t; };
static bool plookup_desc(Args &a, size_t i, PlookupDesc &L) {
    L.d = a.arr(i, PD_WORDS);
    if (!a.ok) return false;
    L.n = L.d[PD_N]; L.kF = L.d[PD_KF]; L.kT = L.d[PD_KT]; L.hDim = (uint32_t)L.d[PD_HDIM];
    const uint64_t *f = L.d + PD_F, *t = L.d + PD_T;
    L.f = pil2gl_tuple_side{ (const uint64_t *)(uintptr_t)f[0], f[1], L.d + PD_F_SLOTS, (const uint64_t *)(uintptr_t)f[2], f[3], f[4] };
    L.t = pil2gl_tuple_side{ (const uint64_t *)(uintptr_t)t[0], t[1], L.d + PD_T_SLOTS, (const uint64_t *)(uintptr_t)t[2], t[3], t[4] };
    return true;
}
#define PD_PTR(L, c) ((uint64_t *)(uintptr_t)(L).d[PD_COLS + 3 * (c)])
#define PD_STRIDE(L, c) ((L).d[PD_COLS + 3 * (c) + 1])
#define PD_COL(L, c) ((L).d[PD_COLS + 3 * (c) + 2])
FN(PlookupFoldDev) {       // (description, elemWords[, stream]): only enqueues
    Args a(env, info); PlookupDesc L; if (!plookup_desc(a, 0, L)) return nullptr;
    uint32_t ew = (uint32_t)a.u64(1); if (!a.ok) return nullptr;
    P2(env, (ew == 4 ? pil2gl_bn128_plookup_fold_dev : pil2gl_plookup_fold_dev)(&L.f, L.kF, &L.t, L.kT, L.d + PD_ALPHA, L.d + PD_BETA, L.hDim, PD_PTR(L, 0), PD_STRIDE(L, 0),
                                                                                PD_COL(L, 0), PD_PTR(L, 1), PD_STRIDE(L, 1), PD_COL(L, 1), L.n, a.stream(2)));
    return mk_undefined(env);
}
FN(PlookupProdDev) {       // (description, elemWords[, stream]): only enqueues
    Args a(env, info); PlookupDesc L; if (!plookup_desc(a, 0, L)) return nullptr;
    uint32_t ew = (uint32_t)a.u64(1); if (!a.ok) return nullptr;
    P2(env, (ew == 4 ? pil2gl_bn128_plookup_prod_dev : pil2gl_plookup_prod_dev)(&L.f, L.kF, &L.t, L.kT, PD_PTR(L, 0), PD_STRIDE(L, 0), PD_COL(L, 0), PD_PTR(L, 1),
                                                                                PD_STRIDE(L, 1), PD_COL(L, 1), L.hDim, L.d + PD_ALPHA, L.d + PD_BETA, L.d + PD_GAMMA,
                                                                                L.d + PD_DELTA, PD_PTR(L, 2), PD_STRIDE(L, 2), PD_COL(L, 2), L.n, a.stream(2)));
    return mk_undefined(env);
}
// the host forms: a column travels through host_matrices as a side of one column (its highest word) over its matrix
static bool plookup_host(Args &a, PlookupDesc &L, uint32_t &ew) {
    if (!plookup_desc(a, 0, L)) return false;
    ew = (uint32_t)a.u64(2); if (!a.ok) return false;
    if (ew != 1 && ew != 4) return a.fail("elemWords is 1 or 4");
    if (L.kF < 1 || L.kF > 16 || L.kT < 1 || L.kT > 16) return a.fail("kF and kT must be 1 .. 16 columns");
    if (L.hDim != 1 && L.hDim != 3) return a.fail("hDim is 1 or 3");
    return true;
}
// (description, matrices, elemWords): matrices = [f's matrix, selF's or null, t's matrix, selT's or null, outF's matrix, null, outT's matrix];
// both outputs are written in place (one matrix given twice is one matrix)
FN(PlookupFold) {
    Args a(env, info); PlookupDesc L; uint32_t ew; if (!plookup_host(a, L, ew)) return nullptr;
    const uint64_t hw = ew == 1 ? L.hDim : 1;
    uint64_t topF = PD_COL(L, 0) + hw - 1;
    pil2gl_tuple_side oF{ nullptr, PD_STRIDE(L, 0), &topF, nullptr, 0, 0 }, *sides[3] = { &L.f, &L.t, &oF };
    const uint64_t ks[3] = { L.kF, L.kT, 1 };
    uint64_t *oT = host_matrices(a, sides, ks, 3, L.n, PD_STRIDE(L, 1), PD_COL(L, 1) + hw - 1, ew,
                                 "expected f's matrix, selF's or null, t's matrix, selT's or null, outF's matrix, null, then outT's matrix");
    if (!a.ok) return nullptr;
    P2(env, (ew == 4 ? pil2gl_bn128_plookup_fold : pil2gl_plookup_fold)(&L.f, L.kF, &L.t, L.kT, L.d + PD_ALPHA, L.d + PD_BETA, L.hDim, (uint64_t *)oF.base, PD_STRIDE(L, 0),
                                                                        PD_COL(L, 0), oT, PD_STRIDE(L, 1), PD_COL(L, 1), L.n));
    return mk_undefined(env);
}
// (description, matrices, elemWords): matrices = [f's matrix, selF's or null, t's matrix, selT's or null, h1's matrix, null, h2's matrix, null,
// out's matrix], the last written in place
FN(PlookupProd) {
    Args a(env, info); PlookupDesc L; uint32_t ew; if (!plookup_host(a, L, ew)) return nullptr;
    const uint64_t hw = ew == 1 ? L.hDim : 1;
    uint64_t top1 = PD_COL(L, 0) + hw - 1, top2 = PD_COL(L, 1) + hw - 1;
    pil2gl_tuple_side h1{ nullptr, PD_STRIDE(L, 0), &top1, nullptr, 0, 0 }, h2{ nullptr, PD_STRIDE(L, 1), &top2, nullptr, 0, 0 }, *sides[4] = { &L.f, &L.t, &h1, &h2 };
    const uint64_t ks[4] = { L.kF, L.kT, 1, 1 };
    uint64_t *ho = host_matrices(a, sides, ks, 4, L.n, PD_STRIDE(L, 2), PD_COL(L, 2) + (ew == 1 ? 2 : 0), ew,
                                 "expected f's matrix, selF's or null, t's matrix, selT's or null, h1's matrix, null, h2's matrix, null, then out's matrix");
    if (!a.ok) return nullptr;
    P2(env, (ew == 4 ? pil2gl_bn128_plookup_prod : pil2gl_plookup_prod)(&L.f, L.kF, &L.t, L.kT, h1.base, PD_STRIDE(L, 0), PD_COL(L, 0), h2.base, PD_STRIDE(L, 1), PD_COL(L, 1),
                                                                        L.hDim, L.d + PD_ALPHA, L.d + PD_BETA, L.d + PD_GAMMA, L.d + PD_DELTA, ho, PD_STRIDE(L, 2),
                                                                        PD_COL(L, 2), L.n));
    return mk_undefined(env);
}

// ---- BN128 Merkle commitment (merklehash_bn128_p.js / merklehash_bn128_worker.js) ----
FN(Bn128Poseidon) {  // (in BigUint64Array(4*nIn*count) normal form, init BigUint64Array(4*count)|null, count, nIn, nOut, out(4*nOut*count))
    Args a(env, info); uint64_t count = a.u64(2), nIn = a.u64(3), nOut = a.u64(4);
    uint64_t *in = a.arr(0, 4 * nIn * count), *init = a.is_nullish(1) ? nullptr : a.arr(1, 4 * count), *out = a.arr(5, 4 * nOut * count); if (!a.ok) return nullptr;
    P2(env, pil2gl_bn128_poseidon(in, init, count, (uint32_t)nIn, (uint32_t)nOut, out)); return mk_undefined(env);
}
FN(Bn128SpongeAbsorb) {  // (blocks BigUint64Array(4*nIn*n) normal form, n, nIn, init BigUint64Array(4), out BigUint64Array(4*(nIn+1)))  transcript.bn128.js:56-83 for a list
    Args a(env, info); uint64_t n = a.u64(1), nIn = a.u64(2);
    uint64_t *blocks = a.arr(0, 4 * nIn * n), *init = a.arr(3, 4), *out = a.arr(4, 4 * (nIn + 1)); if (!a.ok) return nullptr;
    P2(env, pil2gl_bn128_sponge_absorb(blocks, n, (uint32_t)nIn, init, out)); return mk_undefined(env);
}
FN(Bn128LinearHashRows) { // (in, width, height, arity, custom, out(4*height) Montgomery)  merklehash_bn128_worker.js:13
    Args a(env, info); uint64_t w = a.u64(1), h = a.u64(2), arity = a.u64(3); int custom = (int)a.u64(4);
    uint64_t *in = a.arr(0, w * h), *out = a.arr(5, 4 * h); if (!a.ok) return nullptr;
    P2(env, pil2gl_bn128_linear_hash_rows(in, w, h, (uint32_t)arity, custom, out)); return mk_undefined(env);
}
FN(Bn128MerkleNumNodes) { Args a(env, info); uint64_t h = a.u64(0), arity = a.u64(1); if (!a.ok) return nullptr; napi_value v; napi_create_double(env, (double)pil2gl_bn128_merkle_num_nodes(h, (uint32_t)arity), &v); return v; }
FN(Bn128Merkelize) { // (elems, width, height, arity, custom, nodes(4*nNodes))  merklehash_bn128_p.js:47
    Args a(env, info); uint64_t w = a.u64(1), h = a.u64(2), arity = a.u64(3); int custom = (int)a.u64(4);
    uint64_t *el = a.arr(0, w * h), *nodes = a.arr(5, 4 * pil2gl_bn128_merkle_num_nodes(h, (uint32_t)arity)); if (!a.ok) return nullptr;
    P2(env, pil2gl_bn128_merkelize(el, w, h, (uint32_t)arity, custom, nodes)); return mk_undefined(env);
}
FN(Bn128MerkelizeDev) { // (devElems, width, height, arity, custom, devNodes)
    Args a(env, info); uint64_t el = a.u64(0), w = a.u64(1), h = a.u64(2), arity = a.u64(3); int custom = (int)a.u64(4); uint64_t nodes = a.u64(5); if (!a.ok) return nullptr;
    P2(env, pil2gl_bn128_merkelize_dev((const uint64_t *)(uintptr_t)el, w, h, (uint32_t)arity, custom, (uint64_t *)(uintptr_t)nodes, a.stream(6))); return mk_undefined(env);
}
static uint32_t bn128_levels(uint64_t h, uint64_t arity) { uint32_t nl = 0; if (arity >= 2) for (uint64_t n = h; n > 1; n = (n - 1) / arity + 1) nl++; return nl; }
FN(Bn128GroupProofDev) {  // (devElems, devNodes, width, height, arity, idx, vals BigUint64Array(width), siblings BigUint64Array(levels*arity*4) normal form) -> nLevels
    Args a(env, info); uint64_t el = a.u64(0), nodes = a.u64(1), w = a.u64(2), h = a.u64(3), arity = a.u64(4), idx = a.u64(5);
    uint64_t *vals = a.arr(6, w), *sib = a.arr(7, 4ull * arity * bn128_levels(h, arity)); if (!a.ok) return nullptr;
    uint32_t nl = 0;
    P2(env, pil2gl_bn128_group_proof_dev((const uint64_t *)(uintptr_t)el, (const uint64_t *)(uintptr_t)nodes, w, h, (uint32_t)arity, idx, vals, sib, &nl));
    napi_value v; napi_create_uint32(env, nl, &v); return v;
}
FN(Bn128GroupProofsDev) { // (devElems, devNodes, width, height, arity, idxs BigUint64Array(n), vals BigUint64Array(n*width), siblings BigUint64Array(n*levels*arity*4)) -> nLevels: one gather
    Args a(env, info); uint64_t el = a.u64(0), nodes = a.u64(1), w = a.u64(2), h = a.u64(3), arity = a.u64(4);
    uint64_t n = 0; uint64_t *idxs = a.arr(5, 1, &n); if (!a.ok) return nullptr;
    uint64_t *vals = a.arr(6, n * w), *sib = a.arr(7, n * 4ull * arity * bn128_levels(h, arity)); if (!a.ok) return nullptr;
    uint32_t nl = 0;
    P2(env, pil2gl_bn128_group_proofs_dev((const uint64_t *)(uintptr_t)el, (const uint64_t *)(uintptr_t)nodes, w, h, (uint32_t)arity, idxs, (uint32_t)n, vals, sib, &nl));
    napi_value v; napi_create_uint32(env, nl, &v); return v;
}
FN(Bn128RootsFromGroupProofs) {  // (vals BigUint64Array(n*width), siblings BigUint64Array(n*levels*arity*4), width, levels, arity, custom, siblingsMontgomery, idxs BigUint64Array(n), n, roots BigUint64Array(4n))
    Args a(env, info); uint64_t w = a.u64(2), lv = a.u64(3), arity = a.u64(4), n = a.u64(8); int custom = (int)a.u64(5), mont = (int)a.u64(6);
    uint64_t *vals = a.arr(0, n * w), *sib = a.arr(1, n * lv * arity * 4), *idx = a.arr(7, n), *roots = a.arr(9, 4 * n); if (!a.ok) return nullptr;
    P2(env, pil2gl_bn128_roots_from_group_proofs(vals, sib, w, (uint32_t)lv, (uint32_t)arity, custom, mont, idx, (uint32_t)n, roots)); return mk_undefined(env);
}
FN(Bn128Convert) {   // (in BigUint64Array(4n), n, toMontgomery, out)
    Args a(env, info); uint64_t n = a.u64(1); int toM = (int)a.u64(2);
    uint64_t *in = a.arr(0, 4 * n), *out = a.arr(3, 4 * n); if (!a.ok) return nullptr;
    P2(env, pil2gl_bn128_convert(in, n, toM, out)); return mk_undefined(env);
}

// ---- FRI ----
FN(FriFold) {        // (pol, polBits, outBits, shiftInv, challenge[3], out)  fri.js:22
    Args a(env, info); uint32_t pb = (uint32_t)a.u64(1), ob = (uint32_t)a.u64(2); uint64_t sinv = a.u64(3);
    if (pb > 40 || ob > pb) a.fail("Invalid polynomial size");
    uint64_t *pol = a.arr(0, a.ok ? 3ull << pb : 0), *ch = a.arr(4, 3), *out = a.arr(5, a.ok ? 3ull << ob : 0); if (!a.ok) return nullptr;
    P2(env, pil2gl_fri_fold(pol, pb, ob, sinv, ch, out)); return mk_undefined(env);
}
FN(FriVerifyFold) {  // (groups BigUint64Array(3*2^foldBits*nQ), foldBits, nQ, sinv BigUint64Array(nQ), challenge[3], out BigUint64Array(3*nQ))  fri.js:121-127
    Args a(env, info); uint32_t fb = (uint32_t)a.u64(1), nq = (uint32_t)a.u64(2);
    if (fb > 20 || nq == 0) a.fail("Invalid group size or query count");
    uint64_t *g = a.arr(0, a.ok ? (3ull << fb) * nq : 0), *sinv = a.arr(3, nq), *ch = a.arr(4, 3), *out = a.arr(5, 3ull * nq); if (!a.ok) return nullptr;
    P2(env, pil2gl_fri_verify_fold(g, fb, nq, sinv, ch, out)); return mk_undefined(env);
}
FN(FriTranspose) {   // (pol, polBits, transposeBits, out)  fri.js:187
    Args a(env, info); uint32_t pb = (uint32_t)a.u64(1), tb = (uint32_t)a.u64(2);
    if (pb > 40) a.fail("Invalid polynomial size");
    uint64_t *pol = a.arr(0, a.ok ? 3ull << pb : 0), *out = a.arr(3, a.ok ? 3ull << pb : 0); if (!a.ok) return nullptr;
    P2(env, pil2gl_fri_transpose(pol, pb, tb, out)); return mk_undefined(env);
}

FN(FriFoldDev) {     // (dPol, polBits, outBits, shiftInv, challenge BigUint64Array(3), dOut)
    Args a(env, info); uint64_t pol = a.u64(0); uint32_t pb = (uint32_t)a.u64(1), ob = (uint32_t)a.u64(2); uint64_t sinv = a.u64(3);
    uint64_t *ch = a.arr(4, 3); uint64_t out = a.u64(5); if (!a.ok) return nullptr;
    P2(env, pil2gl_fri_fold_dev((const uint64_t *)(uintptr_t)pol, pb, ob, sinv, ch, (uint64_t *)(uintptr_t)out, a.stream(6))); return mk_undefined(env);
}
FN(FriTransposeDev) { // (dPol, polBits, transposeBits, dOut)
    Args a(env, info); uint64_t pol = a.u64(0); uint32_t pb = (uint32_t)a.u64(1), tb = (uint32_t)a.u64(2); uint64_t out = a.u64(3); if (!a.ok) return nullptr;
    P2(env, pil2gl_fri_transpose_dev((const uint64_t *)(uintptr_t)pol, pb, tb, (uint64_t *)(uintptr_t)out, a.stream(4))); return mk_undefined(env);
}

// ---- expression evaluator ----
// (opsBuf BigUint64Array = packed glx_op[], nOps, nTmp, nBits, primeShift, sectionPtrs BigUint64Array, sectionWidths BigUint64Array, scalars BigUint64Array)
FN(EvalProgramDev) {
    Args a(env, info); uint64_t nOps = a.u64(1), nTmp = a.u64(2), nBits = a.u64(3), ps = a.u64(4);
    uint64_t nSec = 0, nSec2 = 0, nSc = 0;
    uint64_t *ops = a.arr(0, nOps * (sizeof(glx_op) / 8)), *ptrs = a.arr(5, 0, &nSec), *widths = a.arr(6, 0, &nSec2), *scal = a.arr(7, 0, &nSc);
    if (a.ok && nSec != nSec2) a.fail("section arrays differ in length");
    if (!a.ok) return nullptr;
    std::vector<glx_section> secs(nSec);
    for (uint64_t i = 0; i < nSec; i++) { secs[i].ptr = (uint64_t *)(uintptr_t)ptrs[i]; secs[i].width = widths[i]; }
    glx_program prog = { (uint32_t)nOps, (uint32_t)nTmp, (const glx_op *)ops };
    glx_ctx ctx = { (uint32_t)nBits, (uint32_t)ps, (uint32_t)nSec, (uint32_t)nSc, secs.data(), scal };
    P2(env, pil2gl_eval_program_dev(&prog, &ctx, nullptr)); return mk_undefined(env);
}

// ---- compile at setup, prove many times (host only: none of the three touches a device) ----
FN(JitCacheSetDir) { // (dir | null | undefined)
    Args a(env, info);
    if (a.is_nullish(0)) { P2(env, pil2gl_jit_cache_set_dir(nullptr)); return mk_undefined(env); }
    size_t n = 0;
    if (napi_get_value_string_utf8(env, a.argv[0], nullptr, 0, &n) != napi_ok) { a.fail("expected a directory name"); return nullptr; }
    std::string dir(n + 1, 0);
    napi_get_value_string_utf8(env, a.argv[0], &dir[0], n + 1, &n);
    P2(env, pil2gl_jit_cache_set_dir(dir.c_str())); return mk_undefined(env);
}
FN(JitCacheStats) {  // -> { memoryHits, diskHits, compiles, diskWrites, rejected, failedWrites, compileMs, diskLoadMs }
    static const char *names[8] = { "memoryHits", "diskHits", "compiles", "diskWrites", "rejected", "failedWrites", "compileMs", "diskLoadMs" };
    uint64_t st[8];
    P2(env, pil2gl_jit_cache_stats(st));
    napi_value o, v; NAPI_CALL(env, napi_create_object(env, &o));
    for (int k = 0; k < 8; k++) { NAPI_CALL(env, napi_create_double(env, (double)st[k], &v)); NAPI_CALL(env, napi_set_named_property(env, o, names[k], v)); }
    return o;
}
// (opsBuf, nOps, nTmp, nBits, primeShift, sectionWidths BigUint64Array, scalars BigUint64Array) -> { routed, origin, codeBytes, slots }
FN(PrecompileProgram) {
    Args a(env, info); uint64_t nOps = a.u64(1), nTmp = a.u64(2), nBits = a.u64(3), ps = a.u64(4);
    uint64_t nSec = 0, nSc = 0;
    uint64_t *ops = a.arr(0, nOps * (sizeof(glx_op) / 8)), *widths = a.arr(5, 0, &nSec), *scal = a.arr(6, 0, &nSc);
    if (!a.ok) return nullptr;
    std::vector<glx_section> secs(nSec);
    for (uint64_t i = 0; i < nSec; i++) { secs[i].ptr = nullptr; secs[i].width = widths[i]; }
    glx_program prog = { (uint32_t)nOps, (uint32_t)nTmp, (const glx_op *)ops };
    glx_ctx ctx = { (uint32_t)nBits, (uint32_t)ps, (uint32_t)nSec, (uint32_t)nSc, secs.data(), scal };
    uint32_t out[4];
    P2(env, pil2gl_precompile_program(&prog, &ctx, out));
    static const char *origin[3] = { "none", "compiled", "disk" };
    napi_value o, v; NAPI_CALL(env, napi_create_object(env, &o));
    NAPI_CALL(env, napi_create_string_utf8(env, out[0] ? "jit" : "interp", NAPI_AUTO_LENGTH, &v)); NAPI_CALL(env, napi_set_named_property(env, o, "routed", v));
    NAPI_CALL(env, napi_create_string_utf8(env, origin[out[1] < 3 ? out[1] : 0], NAPI_AUTO_LENGTH, &v)); NAPI_CALL(env, napi_set_named_property(env, o, "origin", v));
    NAPI_CALL(env, napi_create_uint32(env, out[2], &v)); NAPI_CALL(env, napi_set_named_property(env, o, "codeBytes", v));
    NAPI_CALL(env, napi_create_uint32(env, out[3], &v)); NAPI_CALL(env, napi_set_named_property(env, o, "slots", v));
    return o;
}

// (devCol, dim, first, last) -> [row, v0, v1, v2] as BigInt, row = 2^64-1 when the column is zero on [first, last)
FN(FirstNonzeroRowDev) {
    Args a(env, info); uint64_t col = a.u64(0), dim = a.u64(1), first = a.u64(2), last = a.u64(3);
    if (!a.ok) return nullptr;
    uint64_t out[4] = { 0, 0, 0, 0 };
    P2(env, pil2gl_first_nonzero_row_dev((const uint64_t *)(uintptr_t)col, (uint32_t)dim, first, last, &out[0], &out[1], nullptr));
    napi_value arr; NAPI_CALL(env, napi_create_array_with_length(env, 4, &arr));
    for (uint32_t i = 0; i < 4; i++) { napi_value v; NAPI_CALL(env, napi_create_bigint_uint64(env, out[i], &v)); NAPI_CALL(env, napi_set_element(env, arr, i, v)); }
    return arr;
}

// worker-level operators (fft_worker.js:6-67) on a device block, in place
FN(FftBlockDev) {
    Args a(env, info); uint64_t buf = a.u64(0), startPos = a.u64(1), nPols = a.u64(2), nBits = a.u64(3), s = a.u64(4), blockBits = a.u64(5), layers = a.u64(6);
    if (!a.ok) return nullptr;
    P2(env, pil2gl_fft_block_dev((uint64_t *)(uintptr_t)buf, startPos, nPols, (uint32_t)nBits, (uint32_t)s, (uint32_t)blockBits, (uint32_t)layers, a.stream(7)));
    return mk_undefined(env);
}
FN(InterpolatePrepareBlockDev) {
    Args a(env, info); uint64_t buf = a.u64(0), width = a.u64(1), height = a.u64(2), start = a.u64(3), inc = a.u64(4);
    if (!a.ok) return nullptr;
    P2(env, pil2gl_interpolate_prepare_block_dev((uint64_t *)(uintptr_t)buf, width, height, start, inc, a.stream(5)));
    return mk_undefined(env);
}

static napi_value ModuleInit(napi_env env, napi_value exports) {
    struct { const char *name; napi_callback fn; } fns[] = {
        { "init", Init }, { "shutdown", Shutdown }, { "deviceInfo", DeviceInfo },
        { "devAlloc", DevAlloc }, { "devFree", DevFree }, { "devZero", DevZero }, { "devUpload", DevUpload }, { "devDownload", DevDownload }, { "sync", Sync },
        { "hostAlloc", HostAlloc }, { "hostFree", HostFree }, { "hostRegister", HostRegister }, { "hostUnregister", HostUnregister },
        { "devUploadAsync", DevUploadAsync }, { "devDownloadAsync", DevDownloadAsync }, { "copyAfter", CopyAfter }, { "copyFence", CopyFence }, { "copySync", CopySync },
        { "landRowsDev", LandRowsDev }, { "devLoadFile", DevLoadFile }, { "devSaveFile", DevSaveFile },
        { "interpolate", Interpolate }, { "fft", Fft }, { "ifft", Ifft },
        { "interpolateDev", InterpolateDev }, { "fftDev", FftDev }, { "ifftDev", IfftDev },
        { "poseidon", Poseidon }, { "linearHashRows", LinearHashRows }, { "merkelizeLevel", MerkelizeLevel },
        { "merkleNumNodes", MerkleNumNodes }, { "merkelize", Merkelize }, { "merkelizeDev", MerkelizeDev }, { "groupProofDev", GroupProofDev }, { "groupProofsDev", GroupProofsDev },
        { "rootsFromGroupProofs", RootsFromGroupProofs }, { "spongeAbsorb", SpongeAbsorb },
        { "bn128Poseidon", Bn128Poseidon }, { "bn128SpongeAbsorb", Bn128SpongeAbsorb }, { "bn128LinearHashRows", Bn128LinearHashRows }, { "bn128MerkleNumNodes", Bn128MerkleNumNodes },
        { "bn128Merkelize", Bn128Merkelize }, { "bn128MerkelizeDev", Bn128MerkelizeDev }, { "bn128GroupProofDev", Bn128GroupProofDev }, { "bn128GroupProofsDev", Bn128GroupProofsDev },
        { "bn128RootsFromGroupProofs", Bn128RootsFromGroupProofs }, { "bn128Convert", Bn128Convert },
        { "bn128Fft", Bn128Fft }, { "bn128Ifft", Bn128Ifft }, { "bn128Interpolate", Bn128Interpolate },
        { "bn128FftDev", Bn128FftDev }, { "bn128IfftDev", Bn128IfftDev }, { "bn128InterpolateDev", Bn128InterpolateDev },
        { "bn128G1MsmDev", Bn128G1MsmDev }, { "bn128G1CommitDev", Bn128G1CommitDev }, { "bn128EvalProgramDev", Bn128EvalProgramDev }, { "bn128FirstNonzeroRowDev", Bn128FirstNonzeroRowDev },
        { "bn128PolyDivDev", Bn128PolyDivDev }, { "bn128PolyEvalDev", Bn128PolyEvalDev },
        { "bn128PolyFmaDev", Bn128PolyFmaDev }, { "bn128PolyDegreeDev", Bn128PolyDegreeDev },
        { "bn128BatchInverseDev", Bn128BatchInverseDev }, { "bn128GprodDev", Bn128GprodDev }, { "bn128GsumDev", Bn128GsumDev }, { "bn128GsumColDev", Bn128GsumColDev },
        { "bn128H1h2Dev", Bn128H1h2Dev },
        { "wtnsAddsPlan", WtnsAddsPlan }, { "wtnsAddsDev", WtnsAddsDev }, { "wtnsGatherDev", WtnsGatherDev }, { "wtnsExec", WtnsExec }, { "bn128WtnsExec", Bn128WtnsExec },
        { "connPlan", ConnPlan }, { "connPolsDev", ConnPolsDev }, { "bn128ConnPolsDev", Bn128ConnPolsDev }, { "connPols", ConnPols }, { "bn128ConnPols", Bn128ConnPols },
        { "connCheckPlan", ConnCheckPlan }, { "connCheckDev", ConnCheckDev }, { "bn128ConnCheckDev", Bn128ConnCheckDev }, { "connCheck", ConnCheck }, { "bn128ConnCheck", Bn128ConnCheck },
        { "tupleCheckPlan", TupleCheckPlan }, { "tupleCheckDev", TupleCheckDev }, { "tupleCheck", TupleCheck }, { "tupleHome", TupleHome }, { "tupleCheckProbe", TupleCheckProbe },
        { "lookupMultPlan", LookupMultPlan }, { "lookupMultDev", LookupMultDev }, { "lookupMult", LookupMult }, { "lookupMultProbe", LookupMultProbe },
        { "rangeMultPlan", RangeMultPlan }, { "rangeMultDev", RangeMultDev }, { "rangeMult", RangeMult },
        { "lookupSessionPlan", LookupSessionPlan }, { "lookupSessionOpenDev", LookupSessionOpenDev }, { "lookupSessionAddDev", LookupSessionAddDev },
        { "lookupSessionWriteDev", LookupSessionWriteDev }, { "rangeSessionPlan", RangeSessionPlan }, { "rangeSessionOpenDev", RangeSessionOpenDev },
        { "rangeSessionAddDev", RangeSessionAddDev }, { "rangeSessionWriteDev", RangeSessionWriteDev },
        { "logupSumPlan", LogupSumPlan }, { "logupTermLayout", LogupTermLayout }, { "logupSumDev", LogupSumDev }, { "logupSum", LogupSum },
        { "rangeSumPlan", RangeSumPlan }, { "rangeTermLayout", RangeTermLayout }, { "rangeSumDev", RangeSumDev }, { "rangeSum", RangeSum },
        { "logupClusterPlan", LogupClusterPlan }, { "logupImColLayout", LogupImColLayout }, { "logupClusterDev", LogupClusterDev }, { "logupCluster", LogupCluster },
        { "grandProdPlan", GrandProdPlan }, { "grandProdTermLayout", GrandProdTermLayout }, { "grandProdDev", GrandProdDev }, { "grandProd", GrandProd },
        { "plookupPlan", PlookupPlan }, { "plookupFoldDev", PlookupFoldDev }, { "plookupFold", PlookupFold }, { "plookupProdDev", PlookupProdDev }, { "plookupProd", PlookupProd },
        { "buildXDev", BuildXDev }, { "buildZhInvDev", BuildZhInvDev }, { "buildOneRowZerofierInvDev", BuildOneRowZerofierInvDev },
        { "buildFrameZerofierDev", BuildFrameZerofierDev }, { "computeQSplitDev", ComputeQSplitDev }, { "computeQSplitBrevDev", ComputeQSplitBrevDev }, { "extendCoefsBrevDev", ExtendCoefsBrevDev }, { "xDivXSubXiDev", XDivXSubXiDev },
        { "buildLevDev", BuildLevDev }, { "computeEvalsDev", ComputeEvalsDev }, { "gprodDev", GprodDev }, { "gsumDev", GsumDev }, { "gsumColDev", GsumColDev }, { "h1h2Dev", H1H2Dev },
        { "rowsDotExtDev", RowsDotExtDev }, { "rowsDotExtMultiDev", RowsDotExtMultiDev }, { "friCombineDev", FriCombineDev }, { "colsDotExtDev", ColsDotExtDev }, { "colsDotExtMultiDev", ColsDotExtMultiDev }, { "synthFibonacciDev", SynthFibonacciDev },
        { "friFoldDev", FriFoldDev }, { "friTransposeDev", FriTransposeDev },
        { "friFold", FriFold }, { "friVerifyFold", FriVerifyFold }, { "friTranspose", FriTranspose }, { "evalProgramDev", EvalProgramDev }, { "jitCacheSetDir", JitCacheSetDir }, { "jitCacheStats", JitCacheStats }, { "precompileProgram", PrecompileProgram }, { "firstNonzeroRowDev", FirstNonzeroRowDev },
        { "fftBlockDev", FftBlockDev }, { "interpolatePrepareBlockDev", InterpolatePrepareBlockDev },
    };
    for (auto &f : fns) {
        napi_value v;
        NAPI_CALL(env, napi_create_function(env, f.name, NAPI_AUTO_LENGTH, f.fn, nullptr, &v));
        NAPI_CALL(env, napi_set_named_property(env, exports, f.name, v));
    }
    return exports;
}
NAPI_MODULE(NODE_GYP_MODULE_NAME, ModuleInit)
