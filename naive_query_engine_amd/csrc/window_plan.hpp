// window_plan.hpp — the constants of the window operator's host analysis (quirk Q23, window.hip): the tile and carry counts of the
// segmented scan, the scan operators a function needs and the position arrays it reads.  The analysis itself — plan_window_ex, and
// plan_window, the first entry's adapter onto it — is window_ex_plan.hpp, which needs these constants and which this header includes at
// its end: whoever includes either header has plan_window and WindowPlan, as before the two analyses became one.
// Plain C++17, no HIP and no nqe_table.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "expr_shapes.hpp" // is_word_type
#include "nqe_error.hpp"

namespace nqe {

// rows per workgroup of the segmented scan and of the position scans: 256 threads x 16 consecutive rows (the tests read this line)
constexpr int64_t WIN_TILE = 4096;
constexpr int WIN_THREADS = 256;
constexpr int WIN_ITEMS = int(WIN_TILE / WIN_THREADS);
static_assert(WIN_ITEMS == 16, "a thread's rows are one 16-bit piece of each bitmap");

// tiles of n rows = carries of one scan (one carry per tile)
inline int64_t win_tiles(int64_t n) { return (n + WIN_TILE - 1) / WIN_TILE; }
// rows of the scan's buffers: whole tiles, so that a tile loads and stores 16 bytes at a time without a guard
inline int64_t win_padded_rows(int64_t n) { return win_tiles(n) * WIN_TILE; }
// the one-workgroup carry scan walks the carries in chunks of WIN_THREADS
inline int64_t win_carry_chunks(int64_t n) { return (win_tiles(n) + WIN_THREADS - 1) / WIN_THREADS; }

// the scan operators of one value column (a bit set: some function of the call needs it)
enum WinOp : int { WIN_OP_SUM = 1, WIN_OP_COUNT = 2, WIN_OP_MIN = 4, WIN_OP_MAX = 8 };
// the position arrays over the sorted order (a bit set: some function of the call reads it)
enum WinPos : int {
    WIN_POS_PART_FIRST = 1, // the first position of the row's partition: ROW_NUMBER, RANK, DENSE_RANK
    WIN_POS_PEER_FIRST = 2, // the first position of the row's peer group: RANK
    WIN_POS_PEER_COUNT = 4, // peer starts up to and including the position: DENSE_RANK
    WIN_POS_PEER_LAST = 8,  // the last position of the row's peer group: the RANGE frame
    WIN_POS_PART_LAST = 16  // the last position of the row's partition: the PARTITION frame
};

inline int win_ops_of(int func) {
    switch (func) {
    case NQE_WIN_COUNT: return WIN_OP_COUNT;
    case NQE_WIN_SUM: return WIN_OP_SUM;
    case NQE_WIN_MIN: return WIN_OP_MIN;
    case NQE_WIN_MAX: return WIN_OP_MAX;
    case NQE_WIN_AVG: return WIN_OP_SUM | WIN_OP_COUNT;
    default: return 0;
    }
}
inline int win_positions_of(int func, int frame) {
    switch (func) {
    case NQE_WIN_ROW_NUMBER: return WIN_POS_PART_FIRST;
    case NQE_WIN_RANK: return WIN_POS_PART_FIRST | WIN_POS_PEER_FIRST;
    case NQE_WIN_DENSE_RANK: return WIN_POS_PART_FIRST | WIN_POS_PEER_COUNT;
    default: return frame == NQE_FRAME_RANGE ? WIN_POS_PEER_LAST : frame == NQE_FRAME_PARTITION ? WIN_POS_PART_LAST : 0;
    }
}

} // namespace nqe

#include "window_ex_plan.hpp" // (behind the constants it reads; it includes this header first when it is the one included)
