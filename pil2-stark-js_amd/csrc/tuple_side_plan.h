// Host half of one side of a lookup or a permutation, `sel {c0..ck-1}` as include/pil2gl.h's pil2gl_tuple_side: what tuple_check.hip and
// lookup_mult.hip refuse about a side, the bytes of it that a call touches, and its staging for the host-pointer entries.  No HIP header:
// it builds with the plain C++ compiler (tests/*_plan_dump.cpp run it under the sanitizers).  The device half is tuple_side.cuh.  A file
// pair of its own rather than sections of the index table's: conn_check.hip builds on the table and knows no tuples.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <ctype.h>
#include "../../include/pil2gl.h"
#include "smap_plan.h"

namespace tupleside {

constexpr uint64_t MAX_N = 1ull << 28;
constexpr uint32_t MAX_K = 16;

// the k columns of a tuple inside n <= MAX_N rows of `stride` elements; cols may be in any order and may repeat.  n stride <= 2^58 elements
// keeps span_bytes below 2^63 over either field
inline const char *check_columns(uint64_t n, uint64_t stride, const uint64_t *cols, uint64_t k) {
    if (stride >> 32) return "stride >= 2^32";
    if (n * stride > 1ull << 58) return "n stride above 2^58 elements";
    if (!cols) return "null cols";
    for (uint64_t j = 0; j < k; j++) if (cols[j] >= stride) return "a column >= stride";
    return nullptr;
}
// bytes from the matrix's first element to the end of the last one touched: n rows, highest column `top`
inline uint64_t span_bytes(uint64_t n, uint64_t stride, uint64_t top, uint32_t elemWords) {
    return n ? ((n - 1) * stride + top + 1) * 8 * elemWords : 0;
}
inline uint64_t top_column(const uint64_t *cols, uint64_t k) {
    uint64_t top = 0;
    for (uint64_t j = 0; j < k; j++) top = cols[j] > top ? cols[j] : top;
    return top;
}

// 0, or the message for PIL2GL_EINVAL, made in `why`: "<name>: .." about the columns, then "sel<Name>: .." about the selector's (the
// name's first letter in upper case: "f 3" gives "selF 3")
inline const char *check_side(const char *name, const pil2gl_tuple_side &s, uint64_t n, uint64_t k, char (&why)[80]) {
    if (const char *m = check_columns(n, s.stride, s.hostCols, k)) { snprintf(why, sizeof why, "%s: %s", name, m); return why; }
    const char *m = s.sel ? check_columns(n, s.selStride, &s.selCol, 1) : nullptr;
    if (m) snprintf(why, sizeof why, "sel%c%s: %s", toupper((unsigned char)name[0]), name + 1, m);
    return m ? why : nullptr;
}

// the bytes a call touches of a side's matrix and of its selector's (0: no selector); the side has passed check_side()
inline uint64_t matrix_bytes(const pil2gl_tuple_side &s, uint64_t n, uint64_t k, uint32_t words) { return span_bytes(n, s.stride, top_column(s.hostCols, k), words); }
inline uint64_t sel_bytes(const pil2gl_tuple_side &s, uint64_t n, uint32_t words) { return s.sel ? span_bytes(n, s.selStride, s.selCol, words) : 0; }

// a host side staged up to the last element touched, matrix then selector, each part on 16 bytes: the 64-bit words it takes, and the
// staging itself, after which base and sel are the device's (sel stays null).  Stage: common.h's, a template parameter to keep HIP out
inline uint64_t staged_words(const pil2gl_tuple_side &s, uint64_t n, uint64_t k, uint32_t words) {
    return smapplan::pad16(matrix_bytes(s, n, k, words) / 8) + smapplan::pad16(sel_bytes(s, n, words) / 8);
}
template <class Stage> inline void stage_side(Stage &st, pil2gl_tuple_side &s, uint64_t n, uint64_t k, uint32_t words) {
    const uint64_t nBase = matrix_bytes(s, n, k, words) / 8, nSel = sel_bytes(s, n, words) / 8;
    s.base = st.put(s.base, nBase); st.take(smapplan::pad16(nBase) - nBase);
    s.sel = st.put(s.sel, nSel); st.take(smapplan::pad16(nSel) - nSel);
}

}  // namespace tupleside
