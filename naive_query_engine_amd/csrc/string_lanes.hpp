// string_lanes.hpp — how the kernels that give 2^LG lanes to every string are sized and picked (take_utf8, string_fn.hip, string_args.hip):
// the lanes per string from the mean length, the grid of a kernel that takes 64 >> LG strings per wave and step, and the instance.
#pragma once

#include <cstdint>

#include "nqe_internal.hpp"

namespace nqe {

// lanes per string (log2) from the mean length: a lane moves 8 bytes per step
inline int lanes_log2(int64_t bytes, int64_t rows) {
    const uint64_t mean = uint64_t(bytes) / uint64_t(rows);
    return mean <= 32 ? 2 : mean <= 96 ? 3 : mean <= 256 ? 4 : mean <= 1024 ? 5 : 6;
}
inline int group_grid(nqe_ctx *ctx, int64_t rows, int lg) { return stream_grid(ctx, (rows + (64 >> lg) - 1) / (64 >> lg), 4); }
#define NQE_STR_PICK(kernel, lg) ((lg) == 2 ? kernel<2> : (lg) == 3 ? kernel<3> : (lg) == 4 ? kernel<4> : (lg) == 5 ? kernel<5> : kernel<6>)

} // namespace nqe
