#include "bn_column_stage.h"                         // no kernel here: the host side of the Fr blocks' entries

namespace pil2gl {

ColumnStage::ColumnStage(const bncol::Col *cols, u32 nCols, u64 extraWords) : p_(bncol::stage_plan(cols, nCols)), s_(p_.words + extraWords) {
    for (u32 r = 0; r < p_.nRanges; r++) {
        const bncol::Range &g = p_.range[r];
        base_[r] = g.upload ? const_cast<u64 *>(s_.put((const u64 *)g.lo, g.words)) : s_.take(g.words);
    }
}
u64 *ColumnStage::dev(u32 i) const {
    const u32 r = p_.of[i];
    return r == bncol::NO_RANGE || !base_[r] ? nullptr : base_[r] + p_.off[i];
}
int ColumnStage::copy_back() {
    for (u32 r = 0; r < p_.nRanges; r++)
        if (p_.range[r].download) P2_TRY(s_.get((u64 *)p_.range[r].lo, base_[r], p_.range[r].words));
    return s_.rc();
}

int check_column(const void *p, u64 n, u64 stride, const char *what) {
    if (const char *m = bncol::check_size(n)) return fail(PIL2GL_EINVAL, "%s: n = %llu: %s", what, (unsigned long long)n, m);
    if (const char *m = bncol::check_stride(stride)) return fail(PIL2GL_EINVAL, "%s: stride = %llu: %s", what, (unsigned long long)stride, m);
    if (n && !p) return fail(PIL2GL_EINVAL, "%s: null buffer", what);
    return PIL2GL_OK;
}
int check_aligned16(std::initializer_list<const void *> cols) {
    for (const void *p : cols)
        if ((uintptr_t)p & 15) return fail(PIL2GL_EINVAL, "device columns must be 16-byte aligned");
    return PIL2GL_OK;
}

}  // namespace pil2gl
