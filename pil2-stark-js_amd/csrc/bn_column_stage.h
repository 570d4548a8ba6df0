// The .hip side of the BN254 Fr blocks' column contract (bn_column.h): the refusals as error codes, the staging decision carried out on a Stage.
#pragma once
#include <initializer_list>
#include "common.h"
#include "bn_column.h"

namespace pil2gl {

// a host-pointer call's columns on the device, staged as bncol::stage_plan decides; `extraWords` more for what is no column (poly_eval's results)
class ColumnStage {
public:
    ColumnStage(const bncol::Col *cols, u32 nCols, u64 extraWords = 0);
    int rc() const { return s_.rc(); }
    u64 *dev(u32 i) const;                            // column i on the device; null for an empty column
    Stage &stage() { return s_; }
    int copy_back();                                  // every range that holds a written column, whole
private:
    bncol::StagePlan p_;
    Stage s_;
    u64 *base_[bncol::MAX_COLS];
};

// what every such entry refuses about a column (n, stride, a null pointer with n > 0), and the device forms about its pointers: 0 or PIL2GL_EINVAL
int check_column(const void *p, u64 n, u64 stride, const char *what);
int check_aligned16(std::initializer_list<const void *> cols);

}  // namespace pil2gl
