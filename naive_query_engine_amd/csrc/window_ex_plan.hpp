// window_ex_plan.hpp — the one host analysis of the window operator, for both entries (quirk Q23, window.hip): the argument checks in the
// order include/nqe.h states them, the distinct value columns with their scan operators, the position arrays the function list reads,
// the clamping and classification of ROWS BETWEEN frames, the grouping of bounded frames by (value column, width), plan_window — the
// adapter that takes nqe_window_execute's narrower specs through the same analysis — and
// win_frame_pieces / win_ntile_bucket — the position arithmetic the emit kernels call, written once for host and device so that
// tests/cpp/test_window_ex_plan.cpp checks on the CPU exactly what the device computes.
// Plain C++17, no HIP (the two shared functions carry their qualifiers through NQE_WIN_HD).
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "window_plan.hpp"

#if defined(__HIPCC__)
#define NQE_WIN_HD __host__ __device__ __forceinline__
#else
#define NQE_WIN_HD inline
#endif

namespace nqe {

inline bool winx_is_ranking(int func) { return func >= NQE_WINX_ROW_NUMBER && func <= NQE_WINX_DENSE_RANK; }
inline bool winx_is_aggregate(int func) { return func >= NQE_WINX_COUNT && func <= NQE_WINX_AVG; }
inline bool winx_is_shift(int func) { return func == NQE_WINX_LAG || func == NQE_WINX_LEAD; }
inline bool winx_is_pick(int func) { return func == NQE_WINX_FIRST_VALUE || func == NQE_WINX_LAST_VALUE; }
inline bool winx_is_value(int func) { return winx_is_shift(func) || winx_is_pick(func); } // a column of the argument's dtype, with validity
inline bool winx_is_framed(int func) { return winx_is_aggregate(func) || winx_is_pick(func); }
inline bool winx_reads_column(int func) { return winx_is_aggregate(func) || winx_is_value(func); }

// what a frame is after clamping
enum WinFrameClass : int {
    WIN_FC_OLD = 0,      // PARTITION, ROWS or RANGE (ROWS BETWEEN with both ends unbounded is PARTITION)
    WIN_FC_UP_END = 1,   // UNBOUNDED PRECEDING .. i + end: the partition's forward scan read at min(i + end, pl)
    WIN_FC_START_UF = 2, // i + start .. UNBOUNDED FOLLOWING: the same scan from the other end read at max(i + start, pf)
    WIN_FC_BOUNDED = 3   // i + start .. i + end, both within +-rows: width w = end - start + 1 <= 2 rows + 1
};
struct WinFrameEx {
    int cls = WIN_FC_OLD;
    int frame = NQE_FRAMEX_PARTITION; // WIN_FC_OLD: which one
    int64_t start = 0, end = 0;       // the clamped offsets (only the side that is bounded is read)
    int64_t w = 0;                    // WIN_FC_BOUNDED: the width
};

// An offset below -rows is UNBOUNDED PRECEDING, one above +rows UNBOUNDED FOLLOWING: it reaches past every partition from every
// position.  A start above +rows (an end below -rows) makes every frame empty, and so does +rows (-rows) itself.  Nothing here negates
// INT64_MIN or adds to INT64_MAX: -rows is the only negation and rows >= 0.  The caller has checked start <= end and the sentinels' sides.
inline WinFrameEx win_clamp_frame(int64_t start, int64_t end, int64_t rows) {
    const int64_t lo = -rows;
    const bool up = start < lo, uf = end > rows;
    if (!up && start > rows) start = rows; // (then end > rows too: unbounded following, and i + rows lies behind every partition)
    if (!uf && end < lo) end = lo;         // (then start < -rows too)
    WinFrameEx f;
    if (up && uf) return f; // PARTITION
    f.frame = NQE_FRAMEX_ROWS_BETWEEN;
    f.start = up ? INT64_MIN : start;
    f.end = uf ? INT64_MAX : end;
    f.cls = up ? WIN_FC_UP_END : uf ? WIN_FC_START_UF : WIN_FC_BOUNDED;
    if (f.cls == WIN_FC_BOUNDED) f.w = end - start + 1;
    return f;
}
// the width as the kernels divide by it: positions are below 2^32 - 1, so every width of 2^32 - 1 or more is one single block
inline uint32_t win_block_width(int64_t w) { return w >= int64_t(0xffffffffll) ? 0xffffffffu : uint32_t(w); }

// ---- the decomposition of one row's frame (van Herk / Gil-Werman, segment-aware).  The sorted positions are cut into aligned blocks of w;
// pre[p] is the forward scan restarting where p % w == 0 or p starts a partition, suf[p] the backward scan restarting where
// p % w == w - 1 or p ends a partition.  For the clipped frame [a, b] every piece lies INSIDE the frame:
//   a > b                         empty
//   a / w != b / w                suf[a] and pre[b]   (w >= b - a + 1: the two blocks are neighbours)
//   a % w == 0 or a == pf         pre[b]
//   else                          suf[a]              (then b is a block end or pl)
// The half-unbounded classes have no blocks: pre (the partition's forward scan) at b, or suf at a.
enum WinPiece : int { WIN_PIECE_EMPTY = 0, WIN_PIECE_BOTH = 1, WIN_PIECE_PRE = 2, WIN_PIECE_SUF = 3 };
struct WinPieces {
    int kind;
    uint32_t a, b; // the clipped frame (kind != WIN_PIECE_EMPTY)
};
NQE_WIN_HD WinPieces win_frame_pieces(int cls, int64_t start, int64_t end, uint32_t w, uint32_t i, uint32_t pf, uint32_t pl) {
    int64_t a = int64_t(pf), b = int64_t(pl);
    if (cls != WIN_FC_UP_END) {
        const int64_t s = int64_t(i) + start; // |start| <= rows < 2^32
        if (s > a) a = s;
    }
    if (cls != WIN_FC_START_UF) {
        const int64_t e = int64_t(i) + end;
        if (e < b) b = e;
    }
    WinPieces p{WIN_PIECE_EMPTY, 0u, 0u};
    if (a > b) return p;
    p.a = uint32_t(a), p.b = uint32_t(b);
    if (cls == WIN_FC_UP_END) p.kind = WIN_PIECE_PRE;
    else if (cls == WIN_FC_START_UF) p.kind = WIN_PIECE_SUF;
    else if (p.a / w != p.b / w) p.kind = WIN_PIECE_BOTH;
    else p.kind = (p.a % w == 0 || p.a == pf) ? WIN_PIECE_PRE : WIN_PIECE_SUF;
    return p;
}

// NTILE: the 1-based bucket of the row at offset k = i - pf of a partition of m rows cut into b buckets (b >= 1; 2^32 - 1 stands for
// every larger b: m is smaller).  q = m / b, r = m % b: the first r buckets hold q + 1 rows, the others q.
NQE_WIN_HD uint64_t win_ntile_bucket(uint32_t k, uint32_t m, uint32_t b) {
    const uint32_t q = m / b, r = m % b;
    const uint64_t head = uint64_t(r) * (uint64_t(q) + 1); // rows in the longer buckets (<= m)
    if (uint64_t(k) < head) return uint64_t(k / (q + 1)) + 1;
    return uint64_t(r) + uint64_t((k - uint32_t(head)) / q) + 1; // (q == 0 means head == m > k: not reached)
}

// one (value column, width) pair of bounded frames — or, with w == 0, a value column's scan from the other end (WIN_FC_START_UF):
// two scans (one with w == 0) for the union of the operators of its functions, whatever their `start`
struct WinExGroup {
    int32_t column;
    int64_t w;
    int ops; // WinOp bits
};

struct WindowExPlan {
    std::vector<nqe_sort_key> sort_keys;
    int positions = 0;               // WinPos bits
    std::vector<int32_t> val_cols;   // the value columns scanned forward by partition (old frames and WIN_FC_UP_END), in order of first appearance
    std::vector<int> val_ops;
    std::vector<WinExGroup> groups;  // in order of first appearance
    std::vector<int32_t> rev_cols;   // the distinct columns of `groups`: each needs its gathered values in reverse
    // per function
    std::vector<WinFrameEx> frame;
    std::vector<int> slot;           // index in val_cols, or -1
    std::vector<int> group;          // index in groups, or -1
    std::vector<int64_t> param;      // LAG / LEAD: k clamped to rows; NTILE: b clamped to 2^32 - 1
    std::vector<int> out_dtype;
    bool any_old = false;            // some function 0..7 over an old frame: nqe_window_execute's emit runs
    bool any_frame = false;          // some aggregate over a half-unbounded or bounded frame: the frame emit runs
    bool any_value = false;          // some value function or NTILE: the value emit runs
};

inline bool winx_is_old(int func, const WinFrameEx &f) { return winx_is_ranking(func) || (winx_is_aggregate(func) && f.cls == WIN_FC_OLD); }

// The one analysis of a window call: what nqe_window_execute_ex refuses, in the order of include/nqe.h, and the plan of what it does not;
// launches and allocates nothing.  `dtypes`: the input's column dtypes.  `max_func`, `max_frame`: the last function and frame the entry
// knows (narrower for nqe_window_execute, see plan_window).
inline WindowExPlan plan_window_ex(bool ctx_ok, bool in_ok, bool out_ok, const int *dtypes, int32_t num_cols, int64_t rows, const int32_t *partition_cols,
                                   int32_t num_partition, const nqe_sort_key *order_keys, int32_t num_order, const nqe_window_spec_ex *funcs, int32_t num_funcs,
                                   int max_func = NQE_WINX_NTILE, int max_frame = NQE_FRAMEX_ROWS_BETWEEN) {
    if (!ctx_ok || !in_ok || !out_ok || (num_partition > 0 && !partition_cols) || (num_order > 0 && !order_keys) || (num_funcs > 0 && !funcs))
        fail(NQE_ERR_INVALID_ARGUMENT, "bad arguments");
    for (int32_t f = 0; f < num_funcs; ++f) {
        const nqe_window_spec_ex &s = funcs[f];
        if (s.func < NQE_WINX_ROW_NUMBER || s.func > max_func) fail(NQE_ERR_INVALID_ARGUMENT, "window: unknown window function");
        if (winx_is_framed(s.func)) {
            if (s.frame < NQE_FRAMEX_PARTITION || s.frame > max_frame) fail(NQE_ERR_INVALID_ARGUMENT, "window: unknown frame");
            if (s.frame == NQE_FRAMEX_ROWS_BETWEEN) {
                if (s.start == NQE_FRAME_UNBOUNDED_FOLLOWING) fail(NQE_ERR_INVALID_ARGUMENT, "window: a frame cannot start at UNBOUNDED FOLLOWING");
                if (s.end == NQE_FRAME_UNBOUNDED_PRECEDING) fail(NQE_ERR_INVALID_ARGUMENT, "window: a frame cannot end at UNBOUNDED PRECEDING");
                if (s.start > s.end) fail(NQE_ERR_INVALID_ARGUMENT, "window: the frame's start lies behind its end");
            }
        }
        if (winx_is_shift(s.func) && s.param < 0) fail(NQE_ERR_INVALID_ARGUMENT, "window: the offset of lag / lead is negative");
        if (s.func == NQE_WINX_NTILE && s.param < 1) fail(NQE_ERR_INVALID_ARGUMENT, "window: ntile needs at least one bucket");
    }
    if (num_funcs <= 0) fail(NQE_ERR_PLAN, "window: the list of window functions is empty");
    if (num_partition > NQE_MAX_WINDOW_KEYS || num_order > NQE_MAX_WINDOW_KEYS)
        fail(NQE_ERR_NOT_SUPPORTED, "window: at most " + std::to_string(NQE_MAX_WINDOW_KEYS) + " partition keys and as many order keys per call");
    if (num_funcs > NQE_MAX_WINDOW_FUNCS) fail(NQE_ERR_NOT_SUPPORTED, "window: at most " + std::to_string(NQE_MAX_WINDOW_FUNCS) + " window functions per call");
    WindowExPlan p;
    for (int32_t k = 0; k < num_partition; ++k) p.sort_keys.push_back(nqe_sort_key{partition_cols[k], 0, 1});
    for (int32_t k = 0; k < num_order; ++k) p.sort_keys.push_back(order_keys[k]);
    for (const nqe_sort_key &k : p.sort_keys)
        if (k.column < 0 || k.column >= num_cols) fail(NQE_ERR_NOT_SUPPORTED, "window: key column index out of range");
    for (int32_t f = 0; f < num_funcs; ++f)
        if (winx_reads_column(funcs[f].func) && (funcs[f].column < 0 || funcs[f].column >= num_cols))
            fail(NQE_ERR_NOT_SUPPORTED, winx_is_aggregate(funcs[f].func) ? "aggregate column index out of range" : "window: value column index out of range");
    for (const nqe_sort_key &k : p.sort_keys) {
        const int dt = dtypes[k.column];
        if (!(is_word_type(dt) || dt == NQE_BOOLEAN || dt == NQE_UTF8)) fail(NQE_ERR_NOT_SUPPORTED, "order by: keys of this type are not implemented");
    }
    for (int32_t f = 0; f < num_funcs; ++f)
        if (winx_reads_column(funcs[f].func) && !is_word_type(dtypes[funcs[f].column]))
            fail(NQE_ERR_NOT_SUPPORTED, winx_is_aggregate(funcs[f].func) ? "aggregate func for this column type is not supported"
                                                                         : "window: value functions take Int64, UInt64 and Float64 columns only");
    if (rows >= (int64_t(1) << 32)) fail(NQE_ERR_NOT_SUPPORTED, "window: " + std::to_string(rows) + " rows, the sort handles fewer than 2^32");

    for (int32_t f = 0; f < num_funcs; ++f) {
        const nqe_window_spec_ex &s = funcs[f];
        WinFrameEx fr;
        if (winx_is_framed(s.func)) {
            if (s.frame == NQE_FRAMEX_ROWS_BETWEEN) fr = win_clamp_frame(s.start, s.end, rows);
            else fr.frame = s.frame;
        }
        int slot = -1, group = -1;
        int64_t param = 0;
        int out_dtype = NQE_UINT64;
        if (winx_is_ranking(s.func)) {
            p.positions |= win_positions_of(s.func, 0);
            p.any_old = true;
        } else if (winx_is_aggregate(s.func)) {
            out_dtype = s.func == NQE_WINX_COUNT ? NQE_UINT64 : NQE_FLOAT64;
            const int ops = win_ops_of(s.func);
            if (fr.cls == WIN_FC_OLD || fr.cls == WIN_FC_UP_END) { // the partition's forward scan
                size_t j = 0;
                while (j < p.val_cols.size() && p.val_cols[j] != s.column) ++j;
                if (j == p.val_cols.size()) {
                    p.val_cols.push_back(s.column);
                    p.val_ops.push_back(0);
                }
                p.val_ops[j] |= ops;
                slot = int(j);
            }
            if (fr.cls == WIN_FC_OLD) {
                p.positions |= win_positions_of(s.func, fr.frame);
                p.any_old = true;
            } else {
                p.positions |= WIN_POS_PART_FIRST | WIN_POS_PART_LAST;
                p.any_frame = true;
            }
            if (fr.cls == WIN_FC_START_UF || fr.cls == WIN_FC_BOUNDED) {
                const int64_t w = fr.cls == WIN_FC_BOUNDED ? fr.w : 0;
                size_t g = 0;
                while (g < p.groups.size() && !(p.groups[g].column == s.column && p.groups[g].w == w)) ++g;
                if (g == p.groups.size()) p.groups.push_back(WinExGroup{s.column, w, 0});
                p.groups[g].ops |= ops;
                group = int(g);
                size_t r = 0;
                while (r < p.rev_cols.size() && p.rev_cols[r] != s.column) ++r;
                if (r == p.rev_cols.size()) p.rev_cols.push_back(s.column);
            }
        } else {
            p.any_value = true;
            p.positions |= WIN_POS_PART_FIRST | WIN_POS_PART_LAST;
            if (winx_is_value(s.func)) out_dtype = dtypes[s.column];
            if (winx_is_pick(s.func) && fr.cls == WIN_FC_OLD && fr.frame == NQE_FRAMEX_RANGE) p.positions |= WIN_POS_PEER_LAST;
            if (winx_is_shift(s.func)) param = s.param > rows ? rows : s.param; // i -+ rows lies outside every partition
            if (s.func == NQE_WINX_NTILE) param = s.param > int64_t(0xffffffffll) ? int64_t(0xffffffffll) : s.param;
        }
        p.frame.push_back(fr);
        p.slot.push_back(slot);
        p.group.push_back(group);
        p.param.push_back(param);
        p.out_dtype.push_back(out_dtype);
    }
    return p;
}

// ---- nqe_window_execute is nqe_window_execute_ex over functions 0..7 and frames 0..2 (the enum values are equal): its specs widened,
// every other field zero (a null list stays null) ...
inline std::vector<nqe_window_spec_ex> win_widen(const nqe_window_spec *funcs, int32_t num_funcs) {
    std::vector<nqe_window_spec_ex> wide;
    for (int32_t f = 0; funcs && f < num_funcs; ++f) {
        nqe_window_spec_ex s{};
        s.func = funcs[f].func, s.column = funcs[f].column, s.frame = funcs[f].frame;
        wide.push_back(s);
    }
    return wide;
}
// ... and the same analysis with the two limits that are narrower for it: the same refusals in the same order, the same plan
using WindowPlan = WindowExPlan;
inline WindowPlan plan_window(bool ctx_ok, bool in_ok, bool out_ok, const int *dtypes, int32_t num_cols, int64_t rows, const int32_t *partition_cols, int32_t num_partition,
                              const nqe_sort_key *order_keys, int32_t num_order, const nqe_window_spec *funcs, int32_t num_funcs) {
    const std::vector<nqe_window_spec_ex> wide = win_widen(funcs, num_funcs);
    return plan_window_ex(ctx_ok, in_ok, out_ok, dtypes, num_cols, rows, partition_cols, num_partition, order_keys, num_order, funcs ? wide.data() : nullptr, num_funcs,
                          NQE_WIN_AVG, NQE_FRAME_RANGE);
}

} // namespace nqe
