// window_plan.hpp — the host analysis of the window operator (quirk Q23, window.hip): the argument checks in the order include/nqe.h
// states them, the distinct value columns of the framed aggregates with the scan operators each needs, which position arrays the
// function list reads, and the tile and carry counts of the segmented scan.
// Plain C++17, no HIP and no nqe_table: the input is seen as its column dtypes and row count, so tests/cpp/test_window_plan.cpp
// compiles this header alone.
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

inline bool win_is_ranking(int func) { return func >= NQE_WIN_ROW_NUMBER && func <= NQE_WIN_DENSE_RANK; }
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

struct WindowPlan {
    std::vector<int32_t> val_cols; // the distinct value columns of the framed aggregates, in order of first appearance
    std::vector<int> val_ops;      // per value column: WinOp bits
    std::vector<int> slot;         // per function: its index in val_cols, -1 for a ranking function
    int positions = 0;             // WinPos bits
    std::vector<nqe_sort_key> sort_keys; // the partition keys with default options, then the order keys: the sorted order
};

// What nqe_window_execute refuses, in the order of include/nqe.h; launches and allocates nothing.  `dtypes`: the input's column dtypes.
inline WindowPlan plan_window(bool ctx_ok, bool in_ok, bool out_ok, const int *dtypes, int32_t num_cols, int64_t rows, const int32_t *partition_cols,
                              int32_t num_partition, const nqe_sort_key *order_keys, int32_t num_order, const nqe_window_spec *funcs, int32_t num_funcs) {
    if (!ctx_ok || !in_ok || !out_ok || (num_partition > 0 && !partition_cols) || (num_order > 0 && !order_keys) || (num_funcs > 0 && !funcs))
        fail(NQE_ERR_INVALID_ARGUMENT, "bad arguments");
    for (int32_t f = 0; f < num_funcs; ++f) {
        if (funcs[f].func < NQE_WIN_ROW_NUMBER || funcs[f].func > NQE_WIN_AVG) fail(NQE_ERR_INVALID_ARGUMENT, "window: unknown window function");
        if (!win_is_ranking(funcs[f].func) && (funcs[f].frame < NQE_FRAME_PARTITION || funcs[f].frame > NQE_FRAME_RANGE))
            fail(NQE_ERR_INVALID_ARGUMENT, "window: unknown frame");
    }
    if (num_funcs <= 0) fail(NQE_ERR_PLAN, "window: the list of window functions is empty");
    if (num_partition > NQE_MAX_WINDOW_KEYS || num_order > NQE_MAX_WINDOW_KEYS)
        fail(NQE_ERR_NOT_SUPPORTED, "window: at most " + std::to_string(NQE_MAX_WINDOW_KEYS) + " partition keys and as many order keys per call");
    if (num_funcs > NQE_MAX_WINDOW_FUNCS) fail(NQE_ERR_NOT_SUPPORTED, "window: at most " + std::to_string(NQE_MAX_WINDOW_FUNCS) + " window functions per call");
    WindowPlan p;
    for (int32_t k = 0; k < num_partition; ++k) p.sort_keys.push_back(nqe_sort_key{partition_cols[k], 0, 1});
    for (int32_t k = 0; k < num_order; ++k) p.sort_keys.push_back(order_keys[k]);
    for (const nqe_sort_key &k : p.sort_keys)
        if (k.column < 0 || k.column >= num_cols) fail(NQE_ERR_NOT_SUPPORTED, "window: key column index out of range");
    for (int32_t f = 0; f < num_funcs; ++f)
        if (!win_is_ranking(funcs[f].func) && (funcs[f].column < 0 || funcs[f].column >= num_cols)) fail(NQE_ERR_NOT_SUPPORTED, "aggregate column index out of range");
    for (const nqe_sort_key &k : p.sort_keys) {
        const int dt = dtypes[k.column];
        if (!(is_word_type(dt) || dt == NQE_BOOLEAN || dt == NQE_UTF8)) fail(NQE_ERR_NOT_SUPPORTED, "order by: keys of this type are not implemented");
    }
    for (int32_t f = 0; f < num_funcs; ++f)
        if (!win_is_ranking(funcs[f].func) && !is_word_type(dtypes[funcs[f].column])) fail(NQE_ERR_NOT_SUPPORTED, "aggregate func for this column type is not supported");
    // the permutation is u32: refused before anything is allocated
    if (rows >= (int64_t(1) << 32)) fail(NQE_ERR_NOT_SUPPORTED, "window: " + std::to_string(rows) + " rows, the sort handles fewer than 2^32");
    for (int32_t f = 0; f < num_funcs; ++f) {
        const nqe_window_spec &w = funcs[f];
        p.positions |= win_positions_of(w.func, w.frame);
        if (win_is_ranking(w.func)) {
            p.slot.push_back(-1);
            continue;
        }
        size_t j = 0;
        while (j < p.val_cols.size() && p.val_cols[j] != w.column) ++j;
        if (j == p.val_cols.size()) {
            p.val_cols.push_back(w.column);
            p.val_ops.push_back(0);
        }
        p.val_ops[j] |= win_ops_of(w.func);
        p.slot.push_back(int(j));
    }
    return p;
}

} // namespace nqe
