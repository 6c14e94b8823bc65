// window.hip — window functions as an operator (quirk Q23; the reference has no window expression, logical_plan/expression.rs:22-46):
// f(...) OVER (PARTITION BY ... ORDER BY ...).  All functions of a call share one window.  There is ONE analysis (plan_window_ex,
// window_ex_plan.hpp) and ONE body (win_execute below) behind both entries.  nqe_window_execute_ex is that pair as it stands;
// nqe_window_execute — ROW_NUMBER / RANK / DENSE_RANK and Q10's count / sum / min / max / avg over the frames PARTITION, ROWS ... CURRENT
// ROW and RANGE ... CURRENT ROW, the wider entry's functions 0..7 over its frames 0..2 — is the adapter: plan_window checks its two
// narrower limits through the same analysis, win_widen zero-extends its specs, and the same body runs.  The stages:
//
//   sort         build_sort_permutation (order_by.hip) by (partition keys, order keys): the u32 permutation; no keys, no sort
//   win_bounds   row perm[i] against row perm[i - 1] on every key: the partition-start and peer-start bitmaps
//   win_pos_*    reduce / carry / apply over the bitmaps (integer scans, exact): per position the first position of its partition
//                and of its peer group, the running count of peer starts, and — the same scan from the other end — the last position
//                of its peer group and of its partition; only the arrays the function list reads
//   win_gather   per distinct value column: the column through the permutation as f64, plus its valid bits
//   win_scan_*   reduce / carry / apply: the scan of (sum, count, min, max — those the column's functions need) segmented by the
//                partition-start bitmap; the state at every position
//   win_emit     ONE launch for every output column of the functions 0..7 over the frames 0..2: picks the state at i (ROWS), the peer
//                group's last position (RANGE) or the partition's last position (PARTITION), finishes avg and the ranks, and stores to
//                row perm[i] — the only scatter.  A list of such functions alone (every call of nqe_window_execute) ends here.
// Frames with offsets (n PRECEDING, FOLLOWING) and LAG / LEAD / FIRST_VALUE / LAST_VALUE / NTILE — nqe_window_execute_ex alone — add
// (window_ex_kernels.hpp):
//   win_flags       per distinct width w of a bounded frame: partition starts | block starts, and in reversed positions partition ends |
//                   block ends (w = 0, a frame that runs to UNBOUNDED FOLLOWING: the partition ends alone)
//   win_reverse     per value column of such a frame: the gathered column and its valid bits back to front
//   win_scan_*      per (column, w): the same scan over the column with the first bitmap (pre) and over the reversed column with the
//                   second (suf) — a bounded frame is suf[a] combined with pre[b], both inside the frame, never a prefix difference
//   win_frame_emit  the aggregates over those frames, stored to row perm[i]
//   win_inverse     pos[perm[i]] = i
//   win_value_emit  one thread per INPUT row: LAG / LEAD / FIRST_VALUE / LAST_VALUE with validity words by wave ballot, and NTILE
// Out of scope for both: several different windows in one call (callers call once per window); SQL parsing.
#include <string>

#include "device_utils.hpp"
#include "nqe_internal.hpp"
#include "window_ex_kernels.hpp"
#include "window_ex_plan.hpp"
#include "window_kernels.hpp"
#include "window_plan.hpp"

namespace nqe {

namespace {

template <int OPS> void win_scan_ops(nqe_ctx *ctx, WinScanArgs a) {
    const dim3 tiles(unsigned(a.tiles)), block(WIN_THREADS);
    BufRef carry;
    if (a.tiles > 1) {
        carry = dev_alloc(ctx, size_t(a.tiles) * sizeof(WinVal<OPS>));
        a.carry = carry->ptr;
        launch(ctx, "win_scan_reduce", win_scan_reduce_kernel<OPS>, tiles, block, 0, a);
        launch(ctx, "win_scan_carry", win_scan_carry_kernel<OPS>, dim3(1), block, 0, a);
    }
    launch(ctx, "win_scan_apply", win_scan_apply_kernel<OPS>, tiles, block, 0, a);
}

// the segmented scan of one gathered column for the operators `ops` (WinOp bits, not 0)
void win_scan(nqe_ctx *ctx, int ops, const WinScanArgs &a) {
    switch (ops) {
#define NQE_WIN_CASE(N) case N: win_scan_ops<N>(ctx, a); break;
        NQE_WIN_CASE(1) NQE_WIN_CASE(2) NQE_WIN_CASE(3) NQE_WIN_CASE(4) NQE_WIN_CASE(5) NQE_WIN_CASE(6) NQE_WIN_CASE(7) NQE_WIN_CASE(8)
        NQE_WIN_CASE(9) NQE_WIN_CASE(10) NQE_WIN_CASE(11) NQE_WIN_CASE(12) NQE_WIN_CASE(13) NQE_WIN_CASE(14) NQE_WIN_CASE(15)
#undef NQE_WIN_CASE
    default: fail(NQE_ERR_OTHERS, "window: no scan operator");
    }
}

// ---- the stages of one window call, each called from win_execute alone
// the sorted order, the two bitmaps and the position arrays
struct WinOrder {
    SortPermutation sp;
    BufRef part_start, peer_start, pos[5], pos_carry;
    const uint32_t *part_first = nullptr, *peer_first = nullptr, *peers = nullptr, *peer_last = nullptr, *part_last = nullptr;
    int64_t n = 0, padded = 0, tiles = 0;
    dim3 wave_grid;
};
// one value column through the permutation: its values as f64 and its valid bits (null: no NULLs)
struct WinGathered {
    int32_t column;
    BufRef x, vbits;
};

void win_order(nqe_ctx *ctx, const nqe_table *in, const std::vector<nqe_sort_key> &sort_keys, int32_t num_partition, int positions, WinOrder &o) {
    const int64_t n = in->rows, padded = win_padded_rows(n), tiles = win_tiles(n);
    o.n = n, o.padded = padded, o.tiles = tiles;
    // the sorted order
    SortPermutation &sp = o.sp;
    const int32_t num_keys = int32_t(sort_keys.size());
    if (n > 1 && num_keys > 0) {
        build_sort_permutation(ctx, in, sort_keys.data(), num_keys, &sp);
        sp.keys_in.reset();
        sp.keys_out.reset();
    }
    const dim3 block(WIN_THREADS);
    o.wave_grid = dim3(unsigned(stream_grid(ctx, (n + 63) / 64, WIN_THREADS / 64)));

    // partition starts and peer starts (bitmaps of whole tiles: a tile reads its pieces without a guard)
    o.part_start = dev_alloc(ctx, size_t(padded) / 8), o.peer_start = dev_alloc(ctx, size_t(padded) / 8);
    {
        WinBoundsArgs a;
        std::memset(&a, 0, sizeof(a));
        for (int32_t k = 0; k < num_keys; ++k) {
            const DevColumn &c = in->cols[size_t(sort_keys[size_t(k)].column)];
            WinKeyCol &kc = a.key[k];
            kc.dtype = c.dtype;
            kc.valid = c.null_count == 0 ? nullptr : c.valid();
            if (c.dtype == NQE_UTF8) {
                kc.off = static_cast<const int32_t *>(c.values->ptr);
                kc.data = c.data ? static_cast<const uint8_t *>(c.data->ptr) : nullptr;
            } else if (c.dtype == NQE_BOOLEAN) {
                kc.bits = c.bits();
            } else {
                kc.words = c.words();
            }
        }
        a.num_partition = num_partition;
        a.num_keys = num_keys;
        a.perm = sp.cur;
        a.n = n;
        a.part_start = static_cast<uint64_t *>(o.part_start->ptr);
        a.peer_start = static_cast<uint64_t *>(o.peer_start->ptr);
        launch(ctx, "win_bounds", win_bounds_kernel, o.wave_grid, block, 0, a);
    }

    // positions from the bitmaps
    if (positions) {
        WinPosArgs a;
        std::memset(&a, 0, sizeof(a));
        a.part_start = static_cast<const uint16_t *>(o.part_start->ptr);
        a.peer_start = static_cast<const uint16_t *>(o.peer_start->ptr);
        a.n = n;
        a.tiles = tiles;
        uint32_t **want[5] = {&a.part_first, &a.peer_first, &a.peers, &a.peer_last, &a.part_last};
        for (int b = 0; b < 5; ++b) {
            if (!(positions & (1 << b))) continue;
            o.pos[b] = dev_alloc(ctx, size_t(padded) * 4);
            *want[b] = static_cast<uint32_t *>(o.pos[b]->ptr);
        }
        if (tiles > 1) {
            o.pos_carry = dev_alloc(ctx, size_t(tiles) * sizeof(WinPosCarry));
            a.carry = static_cast<WinPosCarry *>(o.pos_carry->ptr);
            launch(ctx, "win_pos_reduce", win_pos_reduce_kernel, dim3(unsigned(tiles)), block, 0, a);
            launch(ctx, "win_pos_carry", win_pos_carry_kernel, dim3(1), block, 0, a);
        }
        launch(ctx, "win_pos_apply", win_pos_apply_kernel, dim3(unsigned(tiles)), block, 0, a);
        o.part_first = a.part_first, o.peer_first = a.peer_first, o.peers = a.peers, o.peer_last = a.peer_last, o.part_last = a.part_last;
    }
}

// one segmented scan of a gathered column for `ops`, restarting at the bits of `flags`: the state arrays (kept alive by `keep`)
WinEmitVal win_scan_states(nqe_ctx *ctx, const WinOrder &o, const BufRef &x, const BufRef &vbits, const BufRef &flags, int ops, std::vector<BufRef> &keep) {
    WinScanArgs a;
    std::memset(&a, 0, sizeof(a));
    a.x = static_cast<const double *>(x->ptr);
    a.valid = vbits ? static_cast<const uint16_t *>(vbits->ptr) : nullptr;
    a.part_start = static_cast<const uint16_t *>(flags->ptr);
    a.n = o.n;
    a.tiles = o.tiles;
    auto state = [&](int op, size_t width) -> void * {
        if (!(ops & op)) return nullptr;
        keep.push_back(dev_alloc(ctx, size_t(o.padded) * width));
        return keep.back()->ptr;
    };
    a.sum = static_cast<double *>(state(WIN_OP_SUM, 8));
    a.mn = static_cast<double *>(state(WIN_OP_MIN, 8));
    a.mx = static_cast<double *>(state(WIN_OP_MAX, 8));
    a.count = static_cast<uint32_t *>(state(WIN_OP_COUNT, 4));
    win_scan(ctx, ops, a);
    return WinEmitVal{a.sum, a.mn, a.mx, a.count};
}

// column `column` through the permutation as f64, with its valid bits (null: the column has no NULLs)
WinGathered win_gather(nqe_ctx *ctx, const nqe_table *in, const WinOrder &o, int32_t column) {
    const DevColumn &c = in->cols[size_t(column)];
    const uint8_t *valid = c.null_count == 0 ? nullptr : c.valid();
    WinGathered g{column, dev_alloc(ctx, size_t(o.padded) * 8), valid ? dev_alloc(ctx, size_t(o.padded) / 8) : nullptr};
    launch(ctx, "win_gather", win_gather_kernel, o.wave_grid, dim3(WIN_THREADS), 0, c.words(), valid, c.dtype, o.sp.cur, o.n, static_cast<double *>(g.x->ptr),
           g.vbits ? static_cast<uint64_t *>(g.vbits->ptr) : nullptr);
    return g;
}

// every distinct value column: gathered once, scanned once by partition for all the operators its functions need.  `gathered`: where
// the gathered columns are kept for later scans, or null
void win_partition_states(nqe_ctx *ctx, const nqe_table *in, const WinOrder &o, const std::vector<int32_t> &val_cols, const std::vector<int> &val_ops, WinEmitVal *val,
                          std::vector<BufRef> &keep, std::vector<WinGathered> *gathered) {
    for (size_t j = 0; j < val_cols.size(); ++j) {
        const WinGathered g = win_gather(ctx, in, o, val_cols[j]); // (released behind its scan unless the caller keeps it)
        val[j] = win_scan_states(ctx, o, g.x, g.vbits, o.part_start, val_ops[j], keep);
        if (gathered) gathered->push_back(g);
    }
}

// the one emit launch over the functions `e.f`: functions 0..7 over the frames 0..2
void win_emit_old(nqe_ctx *ctx, const WinOrder &o, WinEmitArgs &e) {
    e.part_first = o.part_first, e.peer_first = o.peer_first, e.peers = o.peers, e.peer_last = o.peer_last, e.part_last = o.part_last;
    e.perm = o.sp.cur;
    e.n = o.n;
    launch(ctx, "win_emit", win_emit_kernel, dim3(unsigned(stream_grid(ctx, o.n, WIN_THREADS))), dim3(WIN_THREADS), 0, e);
}

// the input's column dtypes, as the analysis sees a table (none for a null table: the analysis refuses it first)
std::vector<int> win_dtypes(const nqe_table *in) {
    std::vector<int> dtypes;
    if (in)
        for (const DevColumn &c : in->cols) dtypes.push_back(c.dtype);
    return dtypes;
}

// The one body of a window call: the output table of `plan` over `funcs` (what plan_window_ex, or plan_window over the widened list, accepted)
std::unique_ptr<nqe_table> win_execute(nqe_ctx *ctx, const nqe_table *in, int32_t num_partition, const nqe_window_spec_ex *funcs, int32_t num_funcs, const WindowExPlan &plan) {
    const int64_t n = in->rows;

    auto t = std::make_unique<nqe_table>();
    t->ctx = ctx;
    t->rows = n;
    for (int32_t f = 0; f < num_funcs; ++f) {
        t->cols.push_back(make_word_column(ctx, plan.out_dtype[size_t(f)], n, n > 0 && winx_is_value(funcs[f].func)));
        if (n == 0) t->cols.back().null_count = 0;
    }
    if (n == 0) return t;
    WinOrder o;
    win_order(ctx, in, plan.sort_keys, num_partition, plan.positions, o);
    const dim3 block(WIN_THREADS);
    const dim3 row_grid(unsigned(stream_grid(ctx, n, WIN_THREADS)));

    // the partition's forward scans, and the emit of the functions 0..7 over the frames 0..2
    WinEmitArgs e;
    std::memset(&e, 0, sizeof(e));
    std::vector<BufRef> keep;
    std::vector<WinGathered> gathered;
    win_partition_states(ctx, in, o, plan.val_cols, plan.val_ops, e.val, keep, plan.any_frame ? &gathered : nullptr);
    if (plan.any_old) {
        for (int32_t f = 0; f < num_funcs; ++f)
            if (winx_is_old(funcs[f].func, plan.frame[size_t(f)]))
                e.f[e.num_funcs++] = WinEmitFunc{funcs[f].func, plan.frame[size_t(f)].frame, plan.slot[size_t(f)], t->cols[size_t(f)].values->ptr};
        win_emit_old(ctx, o, e);
    }

    // the aggregates over half-unbounded and bounded frames
    if (plan.any_frame) {
        // every column some group scans: gathered (unless the forward scans gathered it already) and reversed, once
        std::vector<WinGathered> reversed;
        for (int32_t column : plan.rev_cols) {
            size_t j = 0;
            while (j < gathered.size() && gathered[j].column != column) ++j;
            if (j == gathered.size()) gathered.push_back(win_gather(ctx, in, o, column));
            const WinGathered &g = gathered[j];
            WinGathered r{column, dev_alloc(ctx, size_t(o.padded) * 8), g.vbits ? dev_alloc(ctx, size_t(o.padded) / 8) : nullptr};
            launch(ctx, "win_reverse", win_reverse_kernel, o.wave_grid, block, 0, static_cast<const double *>(g.x->ptr), g.vbits ? static_cast<const uint8_t *>(g.vbits->ptr) : nullptr, n,
                   static_cast<double *>(r.x->ptr), r.vbits ? static_cast<uint64_t *>(r.vbits->ptr) : nullptr);
            reversed.push_back(r);
        }
        // per width one pair of flag bitmaps, whatever the column; per (column, width) the two scans
        std::vector<int64_t> widths;
        std::vector<BufRef> fwd_flags, rev_flags;
        std::vector<WinEmitVal> pre(plan.groups.size()), suf(plan.groups.size());
        for (size_t g = 0; g < plan.groups.size(); ++g) {
            const WinExGroup &grp = plan.groups[g];
            size_t k = 0;
            while (k < widths.size() && widths[k] != grp.w) ++k;
            if (k == widths.size()) {
                widths.push_back(grp.w);
                fwd_flags.push_back(grp.w ? dev_alloc(ctx, size_t(o.padded) / 8) : nullptr);
                rev_flags.push_back(dev_alloc(ctx, size_t(o.padded) / 8));
                launch(ctx, "win_flags", win_flags_kernel, o.wave_grid, block, 0, static_cast<const uint8_t *>(o.part_start->ptr), n, win_block_width(grp.w),
                       fwd_flags[k] ? static_cast<uint64_t *>(fwd_flags[k]->ptr) : nullptr, static_cast<uint64_t *>(rev_flags[k]->ptr));
            }
            size_t j = 0, r = 0;
            while (gathered[j].column != grp.column) ++j;
            while (reversed[r].column != grp.column) ++r;
            if (grp.w) pre[g] = win_scan_states(ctx, o, gathered[j].x, gathered[j].vbits, fwd_flags[k], grp.ops, keep);
            suf[g] = win_scan_states(ctx, o, reversed[r].x, reversed[r].vbits, rev_flags[k], grp.ops, keep);
        }
        WinFrameArgs a;
        std::memset(&a, 0, sizeof(a));
        for (int32_t f = 0; f < num_funcs; ++f) {
            const WinFrameEx &fr = plan.frame[size_t(f)];
            if (!winx_is_aggregate(funcs[f].func) || fr.cls == WIN_FC_OLD) continue;
            WinFrameFunc &d = a.f[a.num_funcs++];
            d.func = funcs[f].func, d.cls = fr.cls, d.w = fr.cls == WIN_FC_BOUNDED ? win_block_width(fr.w) : 1u;
            d.start = fr.start, d.end = fr.end;
            if (fr.cls == WIN_FC_UP_END) d.pre = e.val[plan.slot[size_t(f)]];
            else d.pre = pre[size_t(plan.group[size_t(f)])], d.suf = suf[size_t(plan.group[size_t(f)])];
            d.out = t->cols[size_t(f)].values->ptr;
        }
        a.perm = o.sp.cur;
        a.part_first = o.part_first, a.part_last = o.part_last;
        a.n = n;
        launch(ctx, "win_frame_emit", win_emit_frame_kernel, row_grid, block, 0, a);
    }

    // LAG / LEAD / FIRST_VALUE / LAST_VALUE / NTILE: one thread per INPUT row
    if (plan.any_value) {
        BufRef pos, nulls = dev_alloc_zero(ctx, size_t(num_funcs) * 8);
        if (o.sp.cur) {
            pos = dev_alloc(ctx, size_t(n) * 4);
            launch(ctx, "win_inverse", win_inverse_kernel, row_grid, block, 0, o.sp.cur, n, static_cast<uint32_t *>(pos->ptr));
        }
        WinValueArgs a;
        std::memset(&a, 0, sizeof(a));
        std::vector<int32_t> which;
        for (int32_t f = 0; f < num_funcs; ++f) {
            const nqe_window_spec_ex &s = funcs[f];
            if (!winx_is_value(s.func) && s.func != NQE_WINX_NTILE) continue;
            const WinFrameEx &fr = plan.frame[size_t(f)];
            WinValueFunc &d = a.f[a.num_funcs++];
            d.func = s.func, d.cls = fr.cls, d.frame = fr.frame, d.has_default = s.has_default;
            d.start = fr.start, d.end = fr.end, d.param = plan.param[size_t(f)];
            d.default_word = s.default_value.u64;
            DevColumn &oc = t->cols[size_t(f)];
            d.out = static_cast<uint64_t *>(oc.values->ptr);
            if (s.func != NQE_WINX_NTILE) {
                const DevColumn &c = in->cols[size_t(s.column)];
                d.words = c.words();
                d.valid = c.null_count == 0 ? nullptr : c.valid();
                d.out_valid = static_cast<uint64_t *>(oc.validity->ptr);
                d.nulls = static_cast<unsigned long long *>(nulls->ptr) + which.size();
                which.push_back(f);
            }
        }
        a.perm = o.sp.cur;
        a.pos = pos ? static_cast<const uint32_t *>(pos->ptr) : nullptr;
        a.part_first = o.part_first, a.part_last = o.part_last, a.peer_last = o.peer_last;
        a.n = n;
        launch(ctx, "win_value_emit", win_emit_value_kernel, o.wave_grid, block, 0, a);
        if (!which.empty()) { // the exact null counts: the call's one wait
            std::vector<unsigned long long> h(which.size());
            NQE_HIP_CHECK(hipMemcpyAsync(h.data(), nulls->ptr, which.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
            sync(ctx);
            for (size_t k = 0; k < which.size(); ++k) {
                DevColumn &oc = t->cols[size_t(which[k])];
                oc.null_count = int64_t(h[k]);
                if (oc.null_count == 0) oc.validity.reset();
            }
        }
    }
    return t;
}

} // namespace

} // namespace nqe

using namespace nqe;

// the first entry is the adapter: plan_window checks its narrower limits through the one analysis, the widened specs go through the one body
nqe_status nqe_window_execute(nqe_ctx *ctx, const nqe_table *in, const int32_t *partition_cols, int32_t num_partition, const nqe_sort_key *order_keys,
                              int32_t num_order, const nqe_window_spec *funcs, int32_t num_funcs, nqe_table **out) {
    NQE_API_BEGIN(ctx)
    const std::vector<int> dtypes = win_dtypes(in);
    const WindowPlan plan = plan_window(ctx != nullptr, in != nullptr, out != nullptr, dtypes.data(), int32_t(dtypes.size()), in ? in->rows : 0, partition_cols, num_partition,
                                        order_keys, num_order, funcs, num_funcs);
    *out = win_execute(ctx, in, num_partition, win_widen(funcs, num_funcs).data(), num_funcs, plan).release();
    NQE_API_END()
}

nqe_status nqe_window_execute_ex(nqe_ctx *ctx, const nqe_table *in, const int32_t *partition_cols, int32_t num_partition, const nqe_sort_key *order_keys,
                                 int32_t num_order, const nqe_window_spec_ex *funcs, int32_t num_funcs, nqe_table **out) {
    NQE_API_BEGIN(ctx)
    const std::vector<int> dtypes = win_dtypes(in);
    const WindowExPlan plan = plan_window_ex(ctx != nullptr, in != nullptr, out != nullptr, dtypes.data(), int32_t(dtypes.size()), in ? in->rows : 0, partition_cols,
                                             num_partition, order_keys, num_order, funcs, num_funcs);
    *out = win_execute(ctx, in, num_partition, funcs, num_funcs, plan).release();
    NQE_API_END()
}

// No NQE_MODULE_PROBE here: like order_by.hip and nested_loop_join.hip, this unit's code object is loaded by the first window call of a
// process, not by nqe_ctx_create (an eagerly loaded unit cost the headline aggregate 1.3 %: profiles/nested_loop_join/README.md).
