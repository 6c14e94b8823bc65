// window.hip — window functions as an operator (quirk Q23; the reference has no window expression, logical_plan/expression.rs:22-46):
// f(...) OVER (PARTITION BY ... ORDER BY ...) for ROW_NUMBER / RANK / DENSE_RANK and Q10's count / sum / min / max / avg over the frames
// PARTITION, ROWS ... CURRENT ROW and RANGE ... CURRENT ROW.  All functions of a call share one window.
//
//   sort         build_sort_permutation (order_by.hip) by (partition keys, order keys): the u32 permutation; no keys, no sort
//   win_bounds   row perm[i] against row perm[i - 1] on every key: the partition-start and peer-start bitmaps
//   win_pos_*    reduce / carry / apply over the bitmaps (integer scans, exact): per position the first position of its partition
//                and of its peer group, the running count of peer starts, and — the same scan from the other end — the last position
//                of its peer group and of its partition; only the arrays the function list reads
//   win_gather   per distinct value column: the column through the permutation as f64, plus its valid bits
//   win_scan_*   reduce / carry / apply: the scan of (sum, count, min, max — those the column's functions need) segmented by the
//                partition-start bitmap; the state at every position
//   win_emit     ONE launch for every output column: picks the state at i (ROWS), the peer group's last position (RANGE) or the
//                partition's last position (PARTITION), finishes avg and the ranks, and stores to row perm[i] — the only scatter
//
// Out of scope: frames with offsets (n PRECEDING, FOLLOWING); LAG / LEAD / FIRST_VALUE / NTILE; several different windows in one call
// (callers call once per window); SQL parsing.
#include <string>

#include "device_utils.hpp"
#include "nqe_internal.hpp"
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

} // namespace

} // namespace nqe

using namespace nqe;

nqe_status nqe_window_execute(nqe_ctx *ctx, const nqe_table *in, const int32_t *partition_cols, int32_t num_partition, const nqe_sort_key *order_keys,
                              int32_t num_order, const nqe_window_spec *funcs, int32_t num_funcs, nqe_table **out) {
    NQE_API_BEGIN(ctx)
    std::vector<int> dtypes;
    if (in)
        for (const DevColumn &c : in->cols) dtypes.push_back(c.dtype);
    const WindowPlan plan = plan_window(ctx != nullptr, in != nullptr, out != nullptr, dtypes.data(), int32_t(dtypes.size()), in ? in->rows : 0, partition_cols, num_partition,
                                        order_keys, num_order, funcs, num_funcs);
    const int64_t n = in->rows, padded = win_padded_rows(n), tiles = win_tiles(n);

    auto t = std::make_unique<nqe_table>();
    t->ctx = ctx;
    t->rows = n;
    for (int32_t f = 0; f < num_funcs; ++f)
        t->cols.push_back(make_word_column(ctx, win_is_ranking(funcs[f].func) || funcs[f].func == NQE_WIN_COUNT ? NQE_UINT64 : NQE_FLOAT64, n, false));
    if (n == 0) {
        *out = t.release();
        return NQE_OK;
    }

    // the sorted order
    SortPermutation sp;
    const int32_t num_keys = int32_t(plan.sort_keys.size());
    if (n > 1 && num_keys > 0) {
        build_sort_permutation(ctx, in, plan.sort_keys.data(), num_keys, &sp);
        sp.keys_in.reset();
        sp.keys_out.reset();
    }
    const dim3 block(WIN_THREADS);
    const dim3 wave_grid(unsigned(stream_grid(ctx, (n + 63) / 64, WIN_THREADS / 64)));

    // partition starts and peer starts (bitmaps of whole tiles: a tile reads its pieces without a guard)
    BufRef part_start = dev_alloc(ctx, size_t(padded) / 8), peer_start = dev_alloc(ctx, size_t(padded) / 8);
    {
        WinBoundsArgs a;
        std::memset(&a, 0, sizeof(a));
        for (int32_t k = 0; k < num_keys; ++k) {
            const DevColumn &c = in->cols[size_t(plan.sort_keys[size_t(k)].column)];
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
        a.part_start = static_cast<uint64_t *>(part_start->ptr);
        a.peer_start = static_cast<uint64_t *>(peer_start->ptr);
        launch(ctx, "win_bounds", win_bounds_kernel, wave_grid, block, 0, a);
    }

    // positions from the bitmaps
    BufRef pos[5], pos_carry;
    WinEmitArgs e;
    std::memset(&e, 0, sizeof(e));
    if (plan.positions) {
        WinPosArgs a;
        std::memset(&a, 0, sizeof(a));
        a.part_start = static_cast<const uint16_t *>(part_start->ptr);
        a.peer_start = static_cast<const uint16_t *>(peer_start->ptr);
        a.n = n;
        a.tiles = tiles;
        uint32_t **want[5] = {&a.part_first, &a.peer_first, &a.peers, &a.peer_last, &a.part_last};
        for (int b = 0; b < 5; ++b) {
            if (!(plan.positions & (1 << b))) continue;
            pos[b] = dev_alloc(ctx, size_t(padded) * 4);
            *want[b] = static_cast<uint32_t *>(pos[b]->ptr);
        }
        if (tiles > 1) {
            pos_carry = dev_alloc(ctx, size_t(tiles) * sizeof(WinPosCarry));
            a.carry = static_cast<WinPosCarry *>(pos_carry->ptr);
            launch(ctx, "win_pos_reduce", win_pos_reduce_kernel, dim3(unsigned(tiles)), block, 0, a);
            launch(ctx, "win_pos_carry", win_pos_carry_kernel, dim3(1), block, 0, a);
        }
        launch(ctx, "win_pos_apply", win_pos_apply_kernel, dim3(unsigned(tiles)), block, 0, a);
        e.part_first = a.part_first, e.peer_first = a.peer_first, e.peers = a.peers, e.peer_last = a.peer_last, e.part_last = a.part_last;
    }

    // every distinct value column: gathered once, scanned once for all the operators its functions need
    std::vector<BufRef> keep;
    for (size_t j = 0; j < plan.val_cols.size(); ++j) {
        const DevColumn &c = in->cols[size_t(plan.val_cols[j])];
        const uint8_t *valid = c.null_count == 0 ? nullptr : c.valid();
        BufRef x = dev_alloc(ctx, size_t(padded) * 8), vbits = valid ? dev_alloc(ctx, size_t(padded) / 8) : nullptr;
        launch(ctx, "win_gather", win_gather_kernel, wave_grid, block, 0, c.words(), valid, c.dtype, sp.cur, n, static_cast<double *>(x->ptr),
               vbits ? static_cast<uint64_t *>(vbits->ptr) : nullptr);
        WinScanArgs a;
        std::memset(&a, 0, sizeof(a));
        a.x = static_cast<const double *>(x->ptr);
        a.valid = vbits ? static_cast<const uint16_t *>(vbits->ptr) : nullptr;
        a.part_start = static_cast<const uint16_t *>(part_start->ptr);
        a.n = n;
        a.tiles = tiles;
        const int ops = plan.val_ops[j];
        auto state = [&](int op, size_t width) -> void * {
            if (!(ops & op)) return nullptr;
            keep.push_back(dev_alloc(ctx, size_t(padded) * width));
            return keep.back()->ptr;
        };
        a.sum = static_cast<double *>(state(WIN_OP_SUM, 8));
        a.mn = static_cast<double *>(state(WIN_OP_MIN, 8));
        a.mx = static_cast<double *>(state(WIN_OP_MAX, 8));
        a.count = static_cast<uint32_t *>(state(WIN_OP_COUNT, 4));
        win_scan(ctx, ops, a);
        e.val[j] = WinEmitVal{a.sum, a.mn, a.mx, a.count};
    }

    for (int32_t f = 0; f < num_funcs; ++f) e.f[f] = WinEmitFunc{funcs[f].func, funcs[f].frame, plan.slot[size_t(f)], t->cols[size_t(f)].values->ptr};
    e.num_funcs = num_funcs;
    e.perm = sp.cur;
    e.n = n;
    launch(ctx, "win_emit", win_emit_kernel, dim3(unsigned(stream_grid(ctx, n, WIN_THREADS))), block, 0, e);
    *out = t.release();
    NQE_API_END()
}

// No NQE_MODULE_PROBE here: like order_by.hip and nested_loop_join.hip, this unit's code object is loaded by the first window call of a
// process, not by nqe_ctx_create (an eagerly loaded unit cost the headline aggregate 1.3 %: profiles/nested_loop_join/README.md).
