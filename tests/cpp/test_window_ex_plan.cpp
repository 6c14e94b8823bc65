// The host analysis of nqe_window_execute_ex (naive_query_engine_amd/csrc/window_ex_plan.hpp) on the CPU: every refusal in the order
// include/nqe.h states, with its message; the clamping of frame offsets at the edges of int64 and of the row count; the classification of
// frames; the grouping of bounded frames by (value column, width) with the union of their operators; and win_frame_pieces — the function
// the emit kernel calls — by brute force against the frame's own index list, with win_ntile_bucket against SQL's rule written out.
//   g++ -std=c++17 -I naive_query_engine_amd/csrc tests/cpp/test_window_ex_plan.cpp && ./a.out
//   (with -fsanitize=address,undefined too: the clamping is where a signed overflow would hide)
#include <algorithm>
#include <cstdio>
#include <string>

#include "window_ex_plan.hpp"

using namespace nqe;

static int failures = 0;
#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) {                                                           \
            if (++failures <= 40) std::printf("%s:%d: CHECK(%s)\n", __FILE__, __LINE__, #cond); \
        }                                                                        \
    } while (0)

enum { I, U, F, B, S, NONE, NCOLS };
static const int kDtypes[NCOLS] = {NQE_INT64, NQE_UINT64, NQE_FLOAT64, NQE_BOOLEAN, NQE_UTF8, NQE_NULLTYPE};
using Keys = std::vector<nqe_sort_key>;
using Funcs = std::vector<nqe_window_spec_ex>;
static const int64_t UP = NQE_FRAME_UNBOUNDED_PRECEDING, UF = NQE_FRAME_UNBOUNDED_FOLLOWING;

static nqe_window_spec_ex spec(int func, int column = 0, int frame = 0, int64_t start = 0, int64_t end = 0, int64_t param = 0) {
    nqe_window_spec_ex s{};
    s.func = func, s.column = column, s.frame = frame, s.start = start, s.end = end, s.param = param;
    return s;
}
static nqe_window_spec_ex between(int func, int column, int64_t start, int64_t end) { return spec(func, column, NQE_FRAMEX_ROWS_BETWEEN, start, end); }

struct Call {
    bool ctx = true, in = true, out = true;
    std::vector<int32_t> parts;
    Keys order;
    Funcs funcs{spec(NQE_WINX_RANK)};
    int64_t rows = 100;
    bool null_parts = false, null_order = false, null_funcs = false;
    int32_t num_parts = -1, num_order = -1, num_funcs = -1; // -1: the vector's size
};

static int status(const Call &c, std::string *msg = nullptr, WindowExPlan *plan = nullptr) {
    try {
        WindowExPlan p = plan_window_ex(c.ctx, c.in, c.out, kDtypes, NCOLS, c.rows, c.null_parts ? nullptr : c.parts.data(), c.num_parts < 0 ? int32_t(c.parts.size()) : c.num_parts,
                                        c.null_order ? nullptr : c.order.data(), c.num_order < 0 ? int32_t(c.order.size()) : c.num_order, c.null_funcs ? nullptr : c.funcs.data(),
                                        c.num_funcs < 0 ? int32_t(c.funcs.size()) : c.num_funcs);
        if (plan) *plan = p;
        return NQE_OK;
    } catch (const Error &e) {
        if (msg) *msg = e.msg;
        return e.code;
    }
}

static void test_layout() {
    static_assert(sizeof(nqe_window_spec_ex) == 48, "nqe_window_spec_ex is 48 bytes");
    static_assert(offsetof(nqe_window_spec_ex, func) == 0 && offsetof(nqe_window_spec_ex, column) == 4 && offsetof(nqe_window_spec_ex, frame) == 8 &&
                      offsetof(nqe_window_spec_ex, has_default) == 12 && offsetof(nqe_window_spec_ex, start) == 16 && offsetof(nqe_window_spec_ex, end) == 24 &&
                      offsetof(nqe_window_spec_ex, param) == 32 && offsetof(nqe_window_spec_ex, default_value) == 40,
                  "the offsets include/nqe.h states");
    static_assert(int(NQE_WINX_ROW_NUMBER) == int(NQE_WIN_ROW_NUMBER) && int(NQE_WINX_RANK) == int(NQE_WIN_RANK) && int(NQE_WINX_DENSE_RANK) == int(NQE_WIN_DENSE_RANK) &&
                      int(NQE_WINX_COUNT) == int(NQE_WIN_COUNT) && int(NQE_WINX_SUM) == int(NQE_WIN_SUM) && int(NQE_WINX_MIN) == int(NQE_WIN_MIN) &&
                      int(NQE_WINX_MAX) == int(NQE_WIN_MAX) && int(NQE_WINX_AVG) == int(NQE_WIN_AVG) && NQE_WINX_NTILE == 12,
                  "0..7 are nqe_window_func's values");
    static_assert(int(NQE_FRAMEX_PARTITION) == int(NQE_FRAME_PARTITION) && int(NQE_FRAMEX_ROWS) == int(NQE_FRAME_ROWS) && int(NQE_FRAMEX_RANGE) == int(NQE_FRAME_RANGE) &&
                      NQE_FRAMEX_ROWS_BETWEEN == 3,
                  "0..2 are nqe_window_frame's values");
}

static void test_errors_in_order() {
    Call ok;
    CHECK(status(ok) == NQE_OK);
    std::string msg;
    // 1. NULL ctx / in / out, a NULL array with a positive count — before anything else
    for (int k = 0; k < 3; ++k) {
        Call c;
        (k == 0 ? c.ctx : k == 1 ? c.in : c.out) = false;
        c.funcs = {spec(99)};
        CHECK(status(c) == NQE_ERR_INVALID_ARGUMENT);
    }
    {
        Call c; c.null_parts = true; c.num_parts = 1; CHECK(status(c) == NQE_ERR_INVALID_ARGUMENT);
        Call d; d.null_order = true; d.num_order = 2; CHECK(status(d) == NQE_ERR_INVALID_ARGUMENT);
        Call e; e.null_funcs = true; e.num_funcs = 1; CHECK(status(e) == NQE_ERR_INVALID_ARGUMENT);
        Call f; f.null_parts = f.null_order = true; f.num_parts = f.num_order = 0; CHECK(status(f) == NQE_OK);
    }
    // 2. per function in list order — before the empty list, the limits, the indices
    for (int bad : {-1, 13, 1000}) {
        Call c; c.funcs = Funcs(20, spec(NQE_WINX_RANK)); c.funcs[19].func = bad; c.parts = {99};
        CHECK(status(c, &msg) == NQE_ERR_INVALID_ARGUMENT && msg == "window: unknown window function");
    }
    for (int fn : {int(NQE_WINX_SUM), int(NQE_WINX_FIRST_VALUE), int(NQE_WINX_LAST_VALUE)})
        for (int bad : {-1, 4}) {
            Call c; c.funcs = {spec(fn, 99, bad)};
            CHECK(status(c, &msg) == NQE_ERR_INVALID_ARGUMENT && msg == "window: unknown frame");
        }
    for (int fn : {int(NQE_WINX_DENSE_RANK), int(NQE_WINX_LAG), int(NQE_WINX_LEAD), int(NQE_WINX_NTILE)}) { // no frame: it is not read
        Call c; c.funcs = {spec(fn, I, 77, UF, UP, 1)};
        CHECK(status(c) == NQE_OK);
    }
    {
        Call a; a.funcs = {between(NQE_WINX_SUM, 99, UF, UF)};
        CHECK(status(a, &msg) == NQE_ERR_INVALID_ARGUMENT && msg == "window: a frame cannot start at UNBOUNDED FOLLOWING");
        Call b; b.funcs = {between(NQE_WINX_LAST_VALUE, 99, UP, UP)};
        CHECK(status(b, &msg) == NQE_ERR_INVALID_ARGUMENT && msg == "window: a frame cannot end at UNBOUNDED PRECEDING");
        Call c; c.funcs = {between(NQE_WINX_MIN, 99, 1, 0)};
        CHECK(status(c, &msg) == NQE_ERR_INVALID_ARGUMENT && msg == "window: the frame's start lies behind its end");
        Call d; d.funcs = {spec(NQE_WINX_SUM, F, NQE_FRAMEX_ROWS, UF, UP)}; // start and end are read with ROWS_BETWEEN only
        CHECK(status(d) == NQE_OK);
        Call e; e.funcs = {spec(NQE_WINX_LAG, 99, 0, 0, 0, -1)};
        CHECK(status(e, &msg) == NQE_ERR_INVALID_ARGUMENT && msg == "window: the offset of lag / lead is negative");
        Call f; f.funcs = {spec(NQE_WINX_LEAD, 99, 0, 0, 0, INT64_MIN)};
        CHECK(status(f, &msg) == NQE_ERR_INVALID_ARGUMENT && msg == "window: the offset of lag / lead is negative");
        Call g; g.funcs = {spec(NQE_WINX_NTILE, 99, 0, 0, 0, 0)};
        CHECK(status(g, &msg) == NQE_ERR_INVALID_ARGUMENT && msg == "window: ntile needs at least one bucket");
        // list order: the first function's complaint wins
        Call h; h.funcs = {spec(NQE_WINX_NTILE, 0, 0, 0, 0, 0), spec(44)};
        CHECK(status(h, &msg) == NQE_ERR_INVALID_ARGUMENT && msg == "window: ntile needs at least one bucket");
        Call i; i.funcs = {spec(NQE_WINX_RANK), spec(44), spec(NQE_WINX_NTILE, 0, 0, 0, 0, 0)};
        CHECK(status(i, &msg) == NQE_ERR_INVALID_ARGUMENT && msg == "window: unknown window function");
    }
    // 3. no functions
    {
        Call c; c.funcs.clear(); c.parts = std::vector<int32_t>(9, 99);
        CHECK(status(c, &msg) == NQE_ERR_PLAN && msg == "window: the list of window functions is empty");
    }
    // 4. the limits — before the indices
    {
        Call c; c.parts = std::vector<int32_t>(NQE_MAX_WINDOW_KEYS + 1, 99);
        CHECK(status(c, &msg) == NQE_ERR_NOT_SUPPORTED && msg.find("at most 8 partition keys") != std::string::npos);
        Call d; d.order = Keys(NQE_MAX_WINDOW_KEYS + 1, nqe_sort_key{99, 0, 1});
        CHECK(status(d, &msg) == NQE_ERR_NOT_SUPPORTED && msg.find("at most 8 partition keys") != std::string::npos);
        Call e; e.funcs = Funcs(NQE_MAX_WINDOW_FUNCS + 1, spec(NQE_WINX_LAG, 99));
        CHECK(status(e, &msg) == NQE_ERR_NOT_SUPPORTED && msg.find("at most 16 window functions") != std::string::npos);
        Call f; f.parts = std::vector<int32_t>(NQE_MAX_WINDOW_KEYS, I); f.order = Keys(NQE_MAX_WINDOW_KEYS, nqe_sort_key{S, 1, 0}); f.funcs = Funcs(NQE_MAX_WINDOW_FUNCS, between(NQE_WINX_SUM, F, -1, 1));
        CHECK(status(f) == NQE_OK);
    }
    // 5. a key or value column index out of range — before the dtypes
    for (int32_t bad : {-1, int32_t(NCOLS)}) {
        Call c; c.parts = {I, bad}; c.funcs = {spec(NQE_WINX_LAG, S)};
        CHECK(status(c, &msg) == NQE_ERR_NOT_SUPPORTED && msg == "window: key column index out of range");
        Call e; e.funcs = {spec(NQE_WINX_RANK), between(NQE_WINX_MAX, bad, -1, 0)}; e.parts = {NONE};
        CHECK(status(e, &msg) == NQE_ERR_NOT_SUPPORTED && msg == "aggregate column index out of range");
        for (int fn = NQE_WINX_LAG; fn <= NQE_WINX_LAST_VALUE; ++fn) {
            Call v; v.funcs = {spec(NQE_WINX_NTILE, bad, 0, 0, 0, 2), spec(fn, bad)}; v.parts = {NONE}; // NTILE reads no column
            CHECK(status(v, &msg) == NQE_ERR_NOT_SUPPORTED && msg == "window: value column index out of range");
        }
    }
    // 6. a key dtype the sort refuses, then the arguments' dtypes in list order — before the row count
    {
        Call c; c.parts = {NONE}; c.funcs = {spec(NQE_WINX_LAG, S)};
        CHECK(status(c, &msg) == NQE_ERR_NOT_SUPPORTED && msg == "order by: keys of this type are not implemented");
    }
    for (int32_t col : {int32_t(B), int32_t(S), int32_t(NONE)}) {
        for (int fn = NQE_WINX_COUNT; fn <= NQE_WINX_AVG; ++fn) {
            Call c; c.funcs = {between(fn, col, -1, 1)}; c.rows = int64_t(1) << 32;
            CHECK(status(c, &msg) == NQE_ERR_NOT_SUPPORTED && msg == "aggregate func for this column type is not supported");
        }
        for (int fn = NQE_WINX_LAG; fn <= NQE_WINX_LAST_VALUE; ++fn) {
            Call c; c.funcs = {spec(NQE_WINX_LAG, I), spec(fn, col)}; c.rows = int64_t(1) << 32;
            CHECK(status(c, &msg) == NQE_ERR_NOT_SUPPORTED && msg == "window: value functions take Int64, UInt64 and Float64 columns only");
        }
    }
    // 7. 2^32 rows or more
    {
        Call c; c.rows = int64_t(1) << 32; c.funcs = {spec(NQE_WINX_NTILE, 0, 0, 0, 0, 3)};
        CHECK(status(c, &msg) == NQE_ERR_NOT_SUPPORTED && msg.find("4294967296 rows, the sort handles fewer than 2^32") != std::string::npos);
        c.rows = (int64_t(1) << 32) - 1;
        CHECK(status(c) == NQE_OK);
        c.rows = 0;
        CHECK(status(c) == NQE_OK);
    }
}

static void test_clamping() {
    const int64_t rows = 1000;
    struct { int64_t start, end; int cls; int64_t cs, ce, w; } want[] = {
        {-2, 0, WIN_FC_BOUNDED, -2, 0, 3},
        {-rows, rows, WIN_FC_BOUNDED, -rows, rows, 2 * rows + 1},           // +-rows stay offsets: the widest bounded frame
        {-(rows + 1), rows, WIN_FC_UP_END, INT64_MIN, rows, 0},             // one more is unbounded
        {-rows, rows + 1, WIN_FC_START_UF, -rows, INT64_MAX, 0},
        {-(rows + 1), rows + 1, WIN_FC_OLD, 0, 0, 0},                       // both: PARTITION
        {UP, UF, WIN_FC_OLD, 0, 0, 0},
        {INT64_MIN + 1, INT64_MAX - 1, WIN_FC_OLD, 0, 0, 0},
        {INT64_MIN + 1, 5, WIN_FC_UP_END, INT64_MIN, 5, 0},
        {-5, INT64_MAX - 1, WIN_FC_START_UF, -5, INT64_MAX, 0},
        {UP, -3, WIN_FC_UP_END, INT64_MIN, -3, 0},
        {3, UF, WIN_FC_START_UF, 3, INT64_MAX, 0},
        {INT64_MAX - 1, INT64_MAX - 1, WIN_FC_START_UF, rows, INT64_MAX, 0}, // every frame empty: i + rows lies behind every partition
        {INT64_MAX - 1, UF, WIN_FC_START_UF, rows, INT64_MAX, 0},
        {INT64_MIN + 1, INT64_MIN + 1, WIN_FC_UP_END, INT64_MIN, -rows, 0}, // every frame empty: i - rows lies in front of every partition
        {UP, INT64_MIN + 1, WIN_FC_UP_END, INT64_MIN, -rows, 0},
        {rows, rows, WIN_FC_BOUNDED, rows, rows, 1},
        {rows + 1, rows + 1, WIN_FC_START_UF, rows, INT64_MAX, 0},
        {-rows, -rows, WIN_FC_BOUNDED, -rows, -rows, 1},
        {-(rows + 1), -(rows + 1), WIN_FC_UP_END, INT64_MIN, -rows, 0},
    };
    for (auto &w : want) {
        const WinFrameEx f = win_clamp_frame(w.start, w.end, rows);
        CHECK(f.cls == w.cls);
        if (w.cls == WIN_FC_OLD) {
            CHECK(f.frame == NQE_FRAMEX_PARTITION);
            continue;
        }
        CHECK(f.frame == NQE_FRAMEX_ROWS_BETWEEN && f.start == w.cs && f.end == w.ce && f.w == w.w);
    }
    // zero rows and the largest table: nothing overflows
    CHECK(win_clamp_frame(-1, 1, 0).cls == WIN_FC_OLD && win_clamp_frame(0, 0, 0).cls == WIN_FC_BOUNDED && win_clamp_frame(0, 0, 0).w == 1);
    const int64_t big = (int64_t(1) << 32) - 1;
    CHECK(win_clamp_frame(-big, big, big).w == 2 * big + 1 && win_block_width(2 * big + 1) == 0xffffffffu && win_block_width(big) == 0xffffffffu && win_block_width(big - 1) == 0xfffffffeu);
    CHECK(win_block_width(1) == 1u && win_block_width(4097) == 4097u);
    // LAG / LEAD offsets and NTILE's buckets are clamped too
    Call c;
    c.funcs = {spec(NQE_WINX_LAG, I, 0, 0, 0, INT64_MAX), spec(NQE_WINX_LEAD, I, 0, 0, 0, 99), spec(NQE_WINX_LEAD, I, 0, 0, 0, 101), spec(NQE_WINX_NTILE, 0, 0, 0, 0, INT64_MAX), spec(NQE_WINX_NTILE, 0, 0, 0, 0, 7)};
    WindowExPlan p;
    CHECK(status(c, nullptr, &p) == NQE_OK && (p.param == std::vector<int64_t>{100, 99, 100, int64_t(0xffffffffll), 7}));
}

static void test_plan() {
    Call c;
    c.parts = {S, I};
    c.order = {{F, 1, 0}};
    c.funcs = {
        between(NQE_WINX_SUM, F, -2, 0),                     // 0: (F, 3)
        between(NQE_WINX_MIN, F, 0, 2),                      // 1: (F, 3) again — another start, the same scans
        between(NQE_WINX_AVG, F, -3, 3),                     // 2: (F, 7)
        between(NQE_WINX_MAX, U, -1, 1),                     // 3: (U, 3)
        between(NQE_WINX_COUNT, F, UP, 5),                   // 4: the partition's forward scan at i + 5
        between(NQE_WINX_SUM, F, -5, UF),                    // 5: (F, 0): the scan from the other end
        between(NQE_WINX_MAX, F, UP, UF),                    // 6: PARTITION — the old emit
        spec(NQE_WINX_SUM, I, NQE_FRAMEX_ROWS),              // 7: old
        spec(NQE_WINX_DENSE_RANK, 77, 77),                   // 8: old
        spec(NQE_WINX_LAG, U, 0, 0, 0, 2),                   // 9
        between(NQE_WINX_FIRST_VALUE, I, -1, 1),             // 10: reads positions only: no scan, no group
        spec(NQE_WINX_LAST_VALUE, I, NQE_FRAMEX_RANGE),      // 11
        spec(NQE_WINX_NTILE, 0, 0, 0, 0, 4),                 // 12
        between(NQE_WINX_MIN, F, -200, -100),                // 13: (F, 101); with 100 rows -200 is UNBOUNDED PRECEDING: forward scan
    };
    WindowExPlan p;
    CHECK(status(c, nullptr, &p) == NQE_OK);
    CHECK((p.val_cols == std::vector<int32_t>{F, I}));
    CHECK((p.val_ops == std::vector<int>{WIN_OP_COUNT | WIN_OP_MAX | WIN_OP_MIN, WIN_OP_SUM}));
    CHECK(p.groups.size() == 4);
    const WinExGroup want[4] = {{F, 3, WIN_OP_SUM | WIN_OP_MIN}, {F, 7, WIN_OP_SUM | WIN_OP_COUNT}, {U, 3, WIN_OP_MAX}, {F, 0, WIN_OP_SUM}};
    for (size_t g = 0; g < 4 && g < p.groups.size(); ++g) CHECK(p.groups[g].column == want[g].column && p.groups[g].w == want[g].w && p.groups[g].ops == want[g].ops);
    CHECK((p.rev_cols == std::vector<int32_t>{F, U}));
    CHECK((p.group == std::vector<int>{0, 0, 1, 2, -1, 3, -1, -1, -1, -1, -1, -1, -1, -1}));
    CHECK((p.slot == std::vector<int>{-1, -1, -1, -1, 0, -1, 0, 1, -1, -1, -1, -1, -1, 0}));
    const int cls[14] = {WIN_FC_BOUNDED, WIN_FC_BOUNDED, WIN_FC_BOUNDED, WIN_FC_BOUNDED, WIN_FC_UP_END, WIN_FC_START_UF, WIN_FC_OLD, WIN_FC_OLD, WIN_FC_OLD, WIN_FC_OLD,
                         WIN_FC_BOUNDED, WIN_FC_OLD, WIN_FC_OLD, WIN_FC_UP_END};
    for (size_t f = 0; f < 14 && f < p.frame.size(); ++f) CHECK(p.frame[f].cls == cls[f]);
    CHECK(p.frame[6].frame == NQE_FRAMEX_PARTITION && p.frame[7].frame == NQE_FRAMEX_ROWS && p.frame[11].frame == NQE_FRAMEX_RANGE && p.frame[13].end == -100);
    CHECK(p.positions == (WIN_POS_PART_FIRST | WIN_POS_PEER_COUNT | WIN_POS_PEER_LAST | WIN_POS_PART_LAST));
    CHECK(p.any_old && p.any_frame && p.any_value);
    CHECK((p.out_dtype == std::vector<int>{NQE_FLOAT64, NQE_FLOAT64, NQE_FLOAT64, NQE_FLOAT64, NQE_UINT64, NQE_FLOAT64, NQE_FLOAT64, NQE_FLOAT64, NQE_UINT64, NQE_UINT64, NQE_INT64,
                                           NQE_INT64, NQE_UINT64, NQE_FLOAT64}));
    CHECK(p.sort_keys.size() == 3 && p.sort_keys[0].column == S && p.sort_keys[2].column == F && p.sort_keys[2].descending == 1);

    // the old functions alone: exactly plan_window's plan, and no new launch
    Call o;
    o.funcs = {spec(NQE_WINX_SUM, F, NQE_FRAMEX_ROWS), spec(NQE_WINX_ROW_NUMBER), spec(NQE_WINX_AVG, U, NQE_FRAMEX_RANGE), spec(NQE_WINX_MIN, F, NQE_FRAMEX_PARTITION)};
    const nqe_window_spec same[4] = {{NQE_WIN_SUM, F, NQE_FRAME_ROWS}, {NQE_WIN_ROW_NUMBER, 0, 0}, {NQE_WIN_AVG, U, NQE_FRAME_RANGE}, {NQE_WIN_MIN, F, NQE_FRAME_PARTITION}};
    const WindowPlan q = plan_window(true, true, true, kDtypes, NCOLS, 100, nullptr, 0, nullptr, 0, same, 4);
    CHECK(status(o, nullptr, &p) == NQE_OK && p.val_cols == q.val_cols && p.val_ops == q.val_ops && p.slot == q.slot && p.positions == q.positions);
    CHECK(p.any_old && !p.any_frame && !p.any_value && p.groups.empty() && p.rev_cols.empty());
    Call v; v.funcs = {spec(NQE_WINX_LEAD, F, 0, 0, 0, 1)};
    CHECK(status(v, nullptr, &p) == NQE_OK && !p.any_old && !p.any_frame && p.any_value && p.val_cols.empty() && p.positions == (WIN_POS_PART_FIRST | WIN_POS_PART_LAST));
}

// win_frame_pieces against the frame's own index list: pre[p] = the positions from p's segment start (a block start or a partition
// start) to p, suf[p] = p to its segment end; the pieces must cover exactly [a, b], every position once
static void test_frame_pieces() {
    uint64_t seed = 12345, combos = 0;
    auto next = [&] { seed = seed * 6364136223846793005ull + 1442695040888963407ull; return uint32_t(seed >> 33); };
    for (int n = 1; n <= 25; ++n) {
        for (int layout = 0; layout < 6; ++layout) { // one partition, lengths of 1..4, four draws of random lengths
            std::vector<int> pf(size_t(n), 0), pl(size_t(n), 0);
            for (int p = 0; p < n;) {
                const int len = layout == 0 ? n : 1 + int(next() % uint32_t(layout == 1 ? 4 : n));
                const int e = std::min(n, p + len) - 1;
                for (int k = p; k <= e; ++k) pf[size_t(k)] = p, pl[size_t(k)] = e;
                p = e + 1;
            }
            for (int64_t start = -n - 1; start <= n + 1; ++start)
                for (int64_t end = start; end <= n + 1; ++end) {
                    ++combos;
                    const WinFrameEx fr = win_clamp_frame(start, end, n);
                    const uint32_t w = fr.cls == WIN_FC_BOUNDED ? win_block_width(fr.w) : 0;
                    for (int i = 0; i < n; ++i) {
                        const int a = std::max<int64_t>(i + start, pf[size_t(i)]), b = std::min<int64_t>(i + end, pl[size_t(i)]);
                        std::vector<int> cover(size_t(n), 0);
                        if (fr.cls == WIN_FC_OLD) { // PARTITION: not a case of the function
                            CHECK(a == pf[size_t(i)] && b == pl[size_t(i)]);
                            continue;
                        }
                        const WinPieces p = win_frame_pieces(fr.cls, fr.start, fr.end, w ? w : 1u, uint32_t(i), uint32_t(pf[size_t(i)]), uint32_t(pl[size_t(i)]));
                        if (a > b) {
                            CHECK(p.kind == WIN_PIECE_EMPTY);
                            continue;
                        }
                        CHECK(p.kind != WIN_PIECE_EMPTY && int(p.a) == a && int(p.b) == b);
                        if (p.kind == WIN_PIECE_BOTH || p.kind == WIN_PIECE_PRE) { // pre[b]
                            int s = pf[size_t(b)];
                            if (w) s = std::max(s, int(uint32_t(b) / w * w));
                            for (int k = s; k <= b; ++k) ++cover[size_t(k)];
                        }
                        if (p.kind == WIN_PIECE_BOTH || p.kind == WIN_PIECE_SUF) { // suf[a]
                            int e = pl[size_t(a)];
                            if (w) e = int(std::min<int64_t>(e, int64_t(uint32_t(a) / w) * w + w - 1));
                            for (int k = a; k <= e; ++k) ++cover[size_t(k)];
                        }
                        bool exact = true;
                        for (int k = 0; k < n; ++k) exact = exact && cover[size_t(k)] == (k >= a && k <= b ? 1 : 0);
                        CHECK(exact);
                    }
                }
        }
    }
    CHECK(combos == 80850);
    // positions near 2^32 and the widest block: 32-bit arithmetic holds
    const uint32_t last = 0xfffffffeu;
    WinPieces p = win_frame_pieces(WIN_FC_BOUNDED, -3, 0, 4, last, 10, last);
    CHECK(p.kind == WIN_PIECE_BOTH && p.a == last - 3 && p.b == last); // last - 3 = 4k + 3 ends a block
    p = win_frame_pieces(WIN_FC_BOUNDED, -int64_t(last), int64_t(last), 0xffffffffu, 5, 0, last);
    CHECK(p.kind == WIN_PIECE_PRE && p.a == 0 && p.b == last);
    p = win_frame_pieces(WIN_FC_START_UF, int64_t(last) + 1, INT64_MAX, 1, last, 0, last);
    CHECK(p.kind == WIN_PIECE_EMPTY);
    p = win_frame_pieces(WIN_FC_UP_END, INT64_MIN, -int64_t(last) - 1, 1, last, 0, last);
    CHECK(p.kind == WIN_PIECE_EMPTY);
}

static void test_ntile() {
    for (uint32_t m = 1; m <= 40; ++m)
        for (uint32_t b : {1u, 2u, 3u, 7u, m > 1 ? m - 1 : 1u, m, m + 1, 1000u, 0xffffffffu}) {
            // SQL's rule written out: hand the rows to the buckets in order
            const uint32_t q = m / b, r = m % b;
            uint32_t k = 0;
            for (uint32_t bucket = 1; bucket <= b && k < m; ++bucket)
                for (uint32_t j = 0; j < q + (bucket <= r ? 1u : 0u) && k < m; ++j, ++k) CHECK(win_ntile_bucket(k, m, b) == bucket);
            CHECK(k == m);
        }
    const uint32_t big = 0xffffffffu;
    CHECK(win_ntile_bucket(big - 1, big, big) == big && win_ntile_bucket(0, big, 2) == 1 && win_ntile_bucket(big - 1, big, 2) == 2 && win_ntile_bucket(big / 2, big, 2) == 1 &&
          win_ntile_bucket(big / 2 + 1, big, 2) == 2);
}

int main() {
    test_layout();
    test_errors_in_order();
    test_clamping();
    test_plan();
    test_frame_pieces();
    test_ntile();
    if (failures) {
        std::printf("%d checks failed\n", failures);
        return 1;
    }
    std::printf("window ex plan ok\n");
    return 0;
}
