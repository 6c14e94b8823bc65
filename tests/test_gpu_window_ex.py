"""nqe_window_execute_ex on the device (csrc/window.hip, window_ex_kernels.hpp; quirk Q23): LAG / LEAD / FIRST_VALUE / LAST_VALUE / NTILE
and ROWS BETWEEN frames.

The yardstick is tests/window_ex_util.py (checked against sqlite3, window_util and itself in tests/test_window_ex_model.py): ranking,
count, min, max and ntile must be equal; sum and avg must lie within the derived bound n_frame * 2^-52 * sum|x| of the frame's OWN finite
values — a value outside the frame has no part in the bound, so an implementation that subtracts prefixes fails next to an infinity or
a 1e300; value functions must be bit-equal with equal validity and the table must report the exact null_count.  Every input is
shuffled by a seeded permutation.  T is the scan's tile, read from csrc/window_plan.hpp.  A call takes at most 16 functions: `check`
computes the model once and sends the functions in calls of 16."""
import ctypes as C
import json
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import agg_value_util as avu  # noqa: E402
import order_by_util as obu  # noqa: E402
import window_ex_util as wx  # noqa: E402
import window_util as wu  # noqa: E402
from naive_query_engine_amd import (Column, ColumnExpr, DType, ErrorCode, Field, Operator, PhysicalBinaryExpr, PhysicalLiteralExpr, RecordBatch, ScalarValue, Status,  # noqa: E402
                                    WindowFrame as F, WindowFrameEx as FX, WindowFunc as W, WindowFuncEx as WX)

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(ROOT, "tests", "golden")
T = int(re.search(r"constexpr int64_t WIN_TILE = (\d+);", open(os.path.join(ROOT, "naive_query_engine_amd", "csrc", "window_plan.hpp")).read()).group(1))
I64_MIN, I64_MAX = -(2 ** 63), 2 ** 63 - 1
NEW_LABELS = ("win_flags", "win_reverse", "win_frame_emit", "win_inverse", "win_value_emit")


@pytest.fixture(scope="module")
def pp():
    from naive_query_engine_amd import physical_plan

    return physical_plan


@pytest.fixture(scope="module")
def ctx():
    from naive_query_engine_amd import capi

    return capi.default_context()


class Launches:
    """the kernel launches of the context while the block runs"""

    def __init__(self, ctx):
        self.ctx = ctx

    def __enter__(self):
        self.ctx.timing_enable(True)
        self.ctx.timing_reset()
        return self

    def count(self, name=""):
        return self.ctx.timing_query(name)[1]

    def __exit__(self, *exc):
        self.ctx.timing_enable(False)
        self.ctx.timing_reset()


def shuffled(cols, seed):
    n = cols[0].length
    return obu.take(cols, np.random.default_rng(seed).permutation(n)) if n else cols


def run(ctx, cols, parts, order, funcs):
    """the device's columns and the null counts its table reports"""
    t = ctx.window_ex(ctx.table_from_host(cols), parts, order, funcs)
    return t.to_host(), [int(t.column_info(i).null_count) for i in range(t.num_columns)]


def check(ctx, cols, parts, order, funcs, what="", model=wx.window_ex):
    m = model(cols, parts, order, funcs)
    got = []
    for lo in range(0, len(funcs), 16):
        hi = min(lo + 16, len(funcs))
        g, nulls = run(ctx, cols, parts, order, funcs[lo:hi])
        part = wx.ModelEx(m.funcs[lo:hi], m.cols[lo:hi], m.valids[lo:hi], m.tols[lo:hi], m.dtypes[lo:hi])
        wx.assert_matches_ex(g, part, what=f"{what} partition by {parts} order by {order} functions {lo}..{hi - 1}", null_counts=nulls)
        got += g
    return got


def i64(a):
    return Column.from_numpy(np.asarray(a, dtype=np.int64))


FIVE_FRAMES = [(-2, 0), (0, 2), (-1, 1), (-3, -1), (1, 3)]


# ----------------------------------------------------------------------------- row counts
@pytest.mark.parametrize("n", sorted({0, 1, 2, T - 1, T, T + 1, 3 * T + 5}))
def test_row_counts_at_the_tiles_edges(ctx, n):
    rng = np.random.default_rng(n)
    cols = shuffled([i64(rng.integers(0, 5, n)), i64(rng.integers(0, 40, n)), Column.from_numpy(np.round(rng.normal(0, 1e3, n), 3), rng.random(n) > 0.15),
                     Column.from_numpy(rng.integers(-10 ** 15, 10 ** 15, n).astype(np.int64), rng.random(n) > 0.15)], n + 1)
    funcs = [f for s, e in FIVE_FRAMES for f in wx.all_aggs(2, s, e)] + [wx.lag(3, 1), wx.lead(2, 2), wx.first(3, -1, 1), wx.last(2, -1, 1), wx.ntile(3)]
    got = check(ctx, cols, [0], [1], funcs, what=f"n={n}")
    assert len(got) == len(funcs) and all(c.length == n for c in got)  # zero rows: a 0-row table with every column
    check(ctx, cols, [], [1], funcs, what=f"n={n} one partition")


# ----------------------------------------------------------------------------- widths against block, tile and partition edges
LENGTHS = [T - 1, 1, 2 * T + 3, T, 5]  # starts on a tile's last row and first row; one partition whose middle tile has no start


def _built_table(seed, special=False):
    n = sum(LENGTHS)
    assert n == 4 * T + 8
    rng = np.random.default_rng(seed)
    x = rng.integers(-wu.NP_VALUE_LIMIT + 1, wu.NP_VALUE_LIMIT, n).astype(np.float64)
    if special:
        x[rng.integers(0, n, 40)], x[rng.integers(0, n, 40)], x[rng.integers(0, n, 40)] = np.inf, -np.inf, np.nan
    # the order key is the built position: the sorted order is the built order, so the partitions start where the lengths put them
    cols = [i64(np.repeat(np.arange(len(LENGTHS)), LENGTHS)), i64(np.arange(n)), Column.from_numpy(rng.integers(-wu.NP_VALUE_LIMIT + 1, wu.NP_VALUE_LIMIT, n).astype(np.int64), rng.random(n) > 0.1),
            Column.from_numpy(x, rng.random(n) > 0.1)]
    return n, shuffled(cols, seed + 1)


def _placements(w):
    return [(-(w - 1), 0), (0, w - 1), (-(w // 2), w - 1 - w // 2)]  # trailing, leading, centred


@pytest.mark.parametrize("w", [1, 2, 3, 16, 17, T - 1, T, T + 1, 2 * T + 3, 4 * T + 8, 2 * (4 * T + 8) + 1])
def test_widths_against_block_tile_and_partition_edges(ctx, w):
    n, cols = _built_table(w % 1000, special=True)
    funcs = [f for s, e in _placements(w) for c in (2, 3) for f in wx.all_aggs(c, s, e)] + [f for s, e in _placements(w) for f in (wx.first(2, s, e), wx.last(3, s, e))]
    check(ctx, cols, [0], [1], funcs, what=f"w={w}", model=wx.window_ex_np)


def test_half_unbounded_frames_and_offsets_at_the_edges_of_int64(ctx):
    n, cols = _built_table(77, special=True)
    frames = [(None, 5), (-5, None), (None, None), (None, -5), (5, None), (I64_MIN + 1, 5), (-5, I64_MAX - 1), (I64_MIN + 1, I64_MAX - 1), (I64_MAX - 1, I64_MAX - 1), (I64_MIN + 1, I64_MIN + 1),
              (-n, n), (-n - 1, n + 1), (n, n), (-n, -n)]
    funcs = [f for s, e in frames for f in wx.all_aggs(3, s, e)] + [f for s, e in frames for f in (wx.first(2, s, e), wx.last(2, s, e))]
    check(ctx, cols, [0], [1], funcs, what="half-unbounded", model=wx.window_ex_np)
    check(ctx, cols, [], [1], funcs[:16], what="half-unbounded, one partition", model=wx.window_ex_np)


# ----------------------------------------------------------------------------- the cancellation trap
def test_values_outside_the_frame_have_no_influence(ctx):
    lengths = [T + 37, 9, 50]
    n = sum(lengths)
    rng = np.random.default_rng(5)
    v = rng.uniform(-1.0, 1.0, n)
    special = {10: np.inf, 200: -np.inf, 1000: np.nan, 2000: 1e300, 2001: -1e300, T - 1: 1e300, T: np.inf, T + 20: np.nan, T + 40: -np.inf}
    for p, s in special.items():
        v[p] = s
    cols = shuffled([i64(np.repeat(np.arange(3), lengths)), i64(np.arange(n)), Column.from_numpy(v)], 6)
    funcs = wx.all_aggs(2, -2, 0) + wx.all_aggs(2, -1, 1) + [wx.agg(WX.Sum, 2, 0, 2), wx.agg(WX.Sum, 2, -7, -1), wx.agg(WX.Sum, 2, -500, 500)]
    got = check(ctx, cols, [0], [1], funcs, what="trap")  # the bound of a frame without a special value is about 1e-15
    pos = cols[1].to_numpy()
    clean = np.ones(n, dtype=bool)
    for p in special:
        clean &= ~((pos >= p) & (pos <= p + 2))  # frame (-2, 0) of position q holds q - 2 .. q
    s = got[1].to_numpy()
    assert np.isfinite(s[clean]).all() and (np.abs(s[clean]) <= 3.0).all()
    assert np.isinf(s[pos == 11]).all() and np.isnan(s[pos == 1002]).all() and np.isnan(got[3].to_numpy()[pos == 1001]).all()  # max becomes NaN, sum of a frame with one too
    assert (got[2].to_numpy()[pos == 1001] <= 1.0).all()  # min ignores it


def test_empty_frames_and_frames_of_nothing_but_nulls_give_the_start_values(ctx):
    n = T + 9
    rng = np.random.default_rng(3)
    key = rng.integers(0, 3, n)
    mask = key != 1  # partition 1: nothing but NULL
    cols = shuffled([i64(key), i64(np.arange(n)), Column.from_numpy(rng.normal(0, 1, n), mask), Column.from_numpy(rng.integers(0, 9, n).astype(np.uint64), np.zeros(n, dtype=bool))], 4)
    funcs = wx.all_aggs(2, -3, -1) + wx.all_aggs(3, -1, 1) + wx.all_aggs(2, n, n) + [wx.first(2, -3, -1), wx.last(2, -3, -1), wx.first(3, -1, 1), wx.last(2, n, n)]
    got = check(ctx, cols, [0], [1], funcs, what="empty and all-NULL frames")
    m = wx.window_ex(cols, [0], [1], [wx.old(W.RowNumber)])
    first_row = m.cols[0] == 1  # (-3, -1) of a partition's first row: empty
    all_null = cols[0].to_numpy() == 1
    for base, rows in ((0, first_row | all_null), (5, np.ones(n, dtype=bool)), (10, np.ones(n, dtype=bool))):  # count, sum, min, max, avg
        assert (got[base].to_numpy()[rows] == 0).all() and (got[base + 1].to_numpy()[rows] == 0.0).all()
        assert (got[base + 2].to_numpy()[rows] == avu.F64_MAX).all() and (got[base + 3].to_numpy()[rows] == -avu.F64_MAX).all() and np.isnan(got[base + 4].to_numpy()[rows]).all()
    assert not got[15].valid_mask()[first_row | all_null].any() and not got[16].valid_mask()[first_row | all_null].any()
    assert not got[17].valid_mask().any() and not got[18].valid_mask().any()


# ----------------------------------------------------------------------------- value functions
def _value_table(seed):
    lengths = [1, 2, 7, T + 3, 40]
    n = sum(lengths)
    rng = np.random.default_rng(seed)
    ints = rng.integers(I64_MIN, I64_MAX, n, dtype=np.int64)
    ints[::5] = (2 ** 53 + 1) * np.where(rng.random(ints[::5].size) < 0.5, 1, -1)  # beyond 2^53: a conversion to f64 would round
    uints = rng.integers(0, 2 ** 64 - 1, n, dtype=np.uint64)
    uints[::7] = np.uint64(2 ** 64 - 1)
    f = rng.normal(0, 1, n)
    f[::3] = np.concatenate([obu.NAN_BITS.view(np.float64), [-0.0, 0.0, np.inf, -np.inf]])[rng.integers(0, obu.NAN_BITS.size + 4, f[::3].size)]  # NaN payloads, -0.0
    cols = [i64(np.repeat(np.arange(len(lengths)), lengths)), i64(np.arange(n)), Column.from_numpy(ints, rng.random(n) > 0.2), Column.from_numpy(uints, rng.random(n) > 0.2),
            Column.from_numpy(f, rng.random(n) > 0.2), Column.from_numpy(f.copy())]
    return n, lengths, shuffled(cols, seed + 1)


def test_lag_and_lead_copy_the_eight_bytes(ctx):
    n, lengths, cols = _value_table(40)
    ks = sorted({0, 1, 10 * n} | {m - 1 for m in lengths} | set(lengths))
    defaults = {2: -77, 3: 2 ** 63 + 5, 4: 2.5, 5: float("-inf")}
    funcs = [fn(c, k, d) for k in ks for c in (2, 3, 4, 5) for fn in (wx.lag, wx.lead) for d in (None, defaults[c])]
    got = check(ctx, cols, [0], [1], funcs, what="lag / lead")
    same = funcs.index(wx.lag(4, 0))  # k = 0 is the row itself: the column, bit for bit, NULLs included
    assert (got[same].valid_mask() == cols[4].valid_mask()).all()
    assert (got[same].to_numpy().view(np.uint64)[cols[4].valid_mask()] == cols[4].to_numpy().view(np.uint64)[cols[4].valid_mask()]).all()
    g, nulls = run(ctx, cols, [0], [1], [wx.lag(5, 0), wx.lead(5, 1, 1.0), wx.lag(5, 10 * n)])
    assert nulls == [0, 0, n] and g[0].validity is None and g[1].validity is None and not g[2].valid_mask().any()  # no validity buffer when nothing is NULL
    check(ctx, cols, [], [], funcs[:16], what="lag / lead, no keys: the input order")


def test_first_and_last_value_over_all_four_frames(ctx):
    n, lengths, cols = _value_table(41)
    cols[1] = i64(cols[1].to_numpy() // 3)  # peer groups of three
    funcs = [fn(c, frame=fr) for c in (2, 3, 4) for fr in (FX.Partition, FX.Rows, FX.Range) for fn in (wx.first, wx.last)]
    funcs += [fn(c, s, e) for c in (2, 4) for s, e in [(-1, 1), (-3, -1), (1, 3), (None, 2), (-2, None), (0, 0), (-T, T)] for fn in (wx.first, wx.last)]
    check(ctx, cols, [0], [1], funcs, what="first / last")


def test_value_functions_over_boolean_and_utf8_are_refused(ctx):
    cols = [i64(np.arange(10)), obu.utf8_column([b"x"] * 10), Column.from_numpy(np.arange(10) % 2 == 0)]
    t = ctx.table_from_host(cols)
    for c in (1, 2):
        for f in (wx.lag(c, 1), wx.lead(c, 1), wx.first(c, -1, 1), wx.last(c, frame=FX.Rows)):
            with pytest.raises(ErrorCode) as e:
                ctx.window_ex(t, [0], [0], [f])
            assert e.value.status == Status.NotSupported and "value functions take Int64, UInt64 and Float64 columns only" in str(e.value)


# ----------------------------------------------------------------------------- ntile
def test_ntile(ctx):
    lengths = [1, 2, 7, 2 * T + 3]
    n = sum(lengths)
    cols = shuffled([i64(np.repeat(np.arange(4), lengths)), i64(np.arange(n))], 9)
    bs = sorted({1, 2, 3, 1000} | {m + d for m in lengths for d in (-1, 0, 1) if m + d >= 1})
    got = check(ctx, cols, [0], [1], [wx.ntile(b) for b in bs] + [wx.ntile(2 ** 40), wx.ntile(I64_MAX)], what="ntile")
    big = got[bs.index(2 * T + 3)].to_numpy()[cols[0].to_numpy() == 3]
    assert sorted(big.tolist()) == list(range(1, 2 * T + 4))  # as many buckets as rows: one row each
    check(ctx, cols, [], [(1, True)], [wx.ntile(b) for b in (1, 2, 3, 1000, n - 1, n, n + 1)], what="ntile, one partition, descending")


# ----------------------------------------------------------------------------- the old entry is a subset
def test_old_functions_and_frames_are_bit_identical_to_the_old_entry(ctx):
    n = 3 * T + 5
    rng = np.random.default_rng(50)
    v, mask = avu.gen_values(avu.DOMAINS[0], rng, n, True)
    cols = shuffled([i64(rng.integers(0, 6, n)), i64(rng.integers(0, 50, n)), Column.from_numpy(v, mask), Column.from_numpy(rng.normal(0, 1e6, n))], 9)
    old = [(W.RowNumber,), (W.Rank,), (W.DenseRank,)] + [(fn, c, fr) for c in (2, 3) for fr in wu.FRAMES for fn in wu.AGGREGATES]
    t = ctx.table_from_host(cols)
    for lo in range(0, len(old), 16):
        a = ctx.window(t, [0], [1], old[lo:lo + 16]).to_host()
        with Launches(ctx) as L:
            b = ctx.window_ex(t, [0], [1], [wx.old(*f) for f in old[lo:lo + 16]]).to_host()
            assert all(L.count(s) == 0 for s in NEW_LABELS) and L.count("win_emit") == 1
        for f, x, y in zip(old[lo:], a, b):
            assert x.dtype == y.dtype and y.validity is None and (x.to_numpy().view(np.uint64) == y.to_numpy().view(np.uint64)).all(), f
    # ROWS BETWEEN UNBOUNDED PRECEDING AND UNBOUNDED FOLLOWING is PARTITION: the old emit, bit for bit
    a = ctx.window(t, [0], [1], [(W.Sum, 3, F.Partition)]).to_host()[0]
    b = ctx.window_ex(t, [0], [1], [wx.agg(WX.Sum, 3, None, None)]).to_host()[0]
    assert (a.to_numpy().view(np.uint64) == b.to_numpy().view(np.uint64)).all()


@pytest.mark.parametrize("n,parts,order", [(5, [0], [1]), (T + 1, [0], [1]), (T + 1, [], [])], ids=["one_tile", "two_tiles_with_carries", "two_tiles_no_keys"])
def test_both_entries_make_the_same_launches(ctx, n, parts, order):
    """The old entry is the adapter onto the one body: the same kernels, label for label and launch for launch, as the wider entry over
    the widened list — the three ranking functions and sum / avg / min over the three frames of one nullable Float64 column."""
    rng = np.random.default_rng(51)
    cols = [i64(rng.integers(0, 3, n)), i64(rng.integers(0, max(2, n // 3), n)), Column.from_numpy(rng.normal(0, 10, n), rng.random(n) > 0.2)]
    old = [(W.RowNumber,), (W.Rank,), (W.DenseRank,)] + [(fn, 2, fr) for fr in wu.FRAMES for fn in (W.Sum, W.Avg, W.Min)]
    assert len(old) == 12
    t = ctx.table_from_host(cols)

    def launches(call):
        with Launches(ctx):
            out = call()
            report = {label: count for label, (_, count) in ctx.timing_report().items()}
        return report, out.to_host()

    a, x = launches(lambda: ctx.window(t, parts, order, old))
    b, y = launches(lambda: ctx.window_ex(t, parts, order, [wx.old(*f) for f in old]))
    assert a == b
    # and they are the launches of such a list: one value column gathered and scanned once, one emit, carries only past one tile, a sort only with keys
    assert a["win_bounds"] == 1 and a["win_gather"] == 1 and a["win_scan_apply"] == 1 and a["win_pos_apply"] == 1 and a["win_emit"] == 1 and not set(a) & set(NEW_LABELS)
    assert [a.get(s, 0) for s in ("win_pos_reduce", "win_pos_carry", "win_scan_reduce", "win_scan_carry")] == [int(n > T)] * 4
    assert any(not s.startswith("win_") for s in a) == bool(parts or order)  # (the sort's kernels are the only ones that are not the unit's own)
    for f, p, q in zip(old, x, y):
        assert p.dtype == q.dtype and q.validity is None and (p.to_numpy().view(np.uint64) == q.to_numpy().view(np.uint64)).all(), f


# ----------------------------------------------------------------------------- sharing, by launch counts
def test_scans_are_shared_by_column_and_width(ctx):
    n = 2 * T + 3
    rng = np.random.default_rng(60)
    cols = shuffled([i64(rng.integers(0, 90, n)), i64(rng.integers(0, 30, n)), Column.from_numpy(rng.normal(0, 5, n), rng.random(n) > 0.1), i64(rng.integers(-9, 9, n))], 8)
    counts = lambda L: [L.count(s) for s in ("win_gather", "win_reverse", "win_flags", "win_scan_apply", "win_scan_reduce", "win_scan_carry", "win_frame_emit", "win_emit", "win_value_emit", "win_inverse")]
    with Launches(ctx) as L:  # two widths over one column: one gather, one reversal, two bitmaps pairs, 2 x 2 scans
        check(ctx, cols, [0], [1], [wx.agg(WX.Sum, 2, -2, 0), wx.agg(WX.Avg, 2, -3, 3)], what="two widths")
        assert counts(L) == [1, 1, 2, 4, 4, 4, 1, 0, 0, 0]
    with Launches(ctx) as L:  # one width over two columns: the bitmaps are shared
        check(ctx, cols, [0], [1], [wx.agg(WX.Sum, 2, -2, 0), wx.agg(WX.Max, 3, -2, 0)], what="two columns")
        assert counts(L) == [2, 2, 1, 4, 4, 4, 1, 0, 0, 0]
    with Launches(ctx) as L:  # equal width, another start, other operators: no scan more
        check(ctx, cols, [0], [1], [wx.agg(WX.Sum, 2, -2, 0), wx.agg(WX.Min, 2, 0, 2), wx.agg(WX.Count, 2, -1, 1), wx.agg(WX.Avg, 2, 5, 7)], what="one width, four starts")
        assert counts(L) == [1, 1, 1, 2, 2, 2, 1, 0, 0, 0]
    with Launches(ctx) as L:  # UNBOUNDED PRECEDING .. 5 reads the partition's forward scan; -5 .. UNBOUNDED FOLLOWING the same scan from the other end
        check(ctx, cols, [0], [1], [wx.agg(WX.Sum, 2, None, 5), wx.old(W.Sum, 2, F.Rows), wx.agg(WX.Sum, 2, -5, None)], what="half-unbounded")
        assert counts(L) == [1, 1, 1, 2, 2, 2, 1, 1, 0, 0]
    with Launches(ctx) as L:  # value functions scan nothing
        check(ctx, cols, [0], [1], [wx.lag(2, 1), wx.first(3, -1, 1), wx.ntile(4)], what="value functions")
        assert counts(L) == [0, 0, 0, 0, 0, 0, 0, 0, 1, 1]
    with Launches(ctx) as L:  # no keys: the order is the input's, nothing to invert
        check(ctx, cols, [], [], [wx.lead(2, 1)], what="no keys")
        assert L.count("win_inverse") == 0 and L.count("win_value_emit") == 1 and L.count("ob_") == 0 and L.count("radix_") == 0


def test_sixteen_functions_mixed(ctx):
    n = 2 * T + 3
    rng = np.random.default_rng(20)
    cols = shuffled([i64(rng.integers(0, 90, n)), i64(rng.integers(0, 30, n)), Column.from_numpy(rng.normal(0, 5, n), rng.random(n) > 0.1), i64(rng.integers(-9, 9, n)),
                     Column.from_numpy(rng.integers(0, 2 ** 63, n, dtype=np.uint64) * np.uint64(2))], 8)
    funcs = [wx.old(W.RowNumber), wx.old(W.Rank), wx.old(W.DenseRank), wx.old(W.Sum, 2, F.Rows), wx.old(W.Avg, 3, F.Range), wx.old(W.Max, 4, F.Partition), wx.agg(WX.Sum, 2, -6, 0),
             wx.agg(WX.Avg, 2, -6, 0), wx.agg(WX.Min, 3, -1, 1), wx.agg(WX.Count, 2, None, 3), wx.agg(WX.Max, 4, -2, None), wx.lag(4, 1), wx.lead(3, 2, -1), wx.first(2, frame=FX.Range),
             wx.last(4, -1, 1), wx.ntile(4)]
    assert len(funcs) == 16
    with Launches(ctx) as L:
        check(ctx, cols, [0], [1], funcs, what="sixteen functions")
        assert L.count("win_emit") == 1 and L.count("win_frame_emit") == 1 and L.count("win_value_emit") == 1 and L.count("win_bounds") == 1


# ----------------------------------------------------------------------------- past the first chunk of the carry scans
def test_past_the_first_chunk_of_the_carry_scans(ctx):
    n = 256 * T + T + 5
    rng = np.random.default_rng(70)
    lengths = wu.layout_lengths("random_lengths", n, T, 256 * T, rng, longest=40 * T)
    lengths = [3, 1, 256 * T - 40] + lengths  # a long partition up to just in front of the first chunk edge, then long and short ones
    total, keep = 0, []
    for length in lengths:
        length = min(length, n - total)
        if length > 0:
            keep.append(length)
            total += length
    cols, parts, order = wu.layout_table(keep, rng, False)
    cols = shuffled(cols, 71)
    funcs = wx.all_aggs(3, -3, 3) + wx.all_aggs(2, -(3 * T), 0) + [wx.agg(WX.Sum, 3, 0, 3 * T), wx.lag(2, 1), wx.lead(3, T, 0.5), wx.ntile(5)]
    check(ctx, cols, parts, order, funcs, what="257 tiles", model=wx.window_ex_np)


# ----------------------------------------------------------------------------- the mirror
def _mem(pp, ctx, fields, batches):
    return pp.ScanPlan.create(pp.MemTable.try_create(fields, [RecordBatch(fields, b) for b in batches], ctx), None)


def _col(name):
    return ColumnExpr.try_create(name, None)


def test_three_batches_one_of_them_empty_through_the_mirror(pp, ctx):
    fields = [Field("k", DType.INT64, True), Field("o", DType.FLOAT64, False), Field("v", DType.INT64, True)]
    rng = np.random.default_rng(21)
    batches = []
    for n in (700, 0, T):
        b = [obu.random_column(rng, DType.INT64, n, True, 5), obu.random_column(rng, DType.FLOAT64, n, False, 5), Column.from_numpy(rng.integers(-99, 99, n).astype(np.int64), rng.random(n) > 0.2)]
        for c in (b[0], b[2]):
            if c.validity is None:
                c.validity = obu.pack_bits(np.ones(c.length, dtype=bool))
        batches.append(b)
    X = pp.WindowFunctionEx
    funcs = [X(WX.RowNumber), X(WX.Sum, _col("v"), FX.RowsBetween, start=-6, end=0), X(WX.Lag, _col("v"), offset=2), X(WX.Lead, _col("v"), offset=1, default=ScalarValue.Int64(-5)),
             X(WX.FirstValue, _col("v"), FX.RowsBetween, start=-1, end=None), X(WX.Ntile, buckets=4), X(WX.Count, _col("v"))]
    plan = pp.PhysicalWindowPlanEx.create(_mem(pp, ctx, fields, batches), [_col("k")], [pp.PhysicalSortExpr(_col("o"), descending=True)], funcs)
    names = ["k", "o", "v", "row_number()", "sum(v)", "lag(v, 2)", "lead(v, 1)", "first_value(v)", "ntile(4)", "count(v)"]
    assert [f.name for f in plan.schema()] == names
    assert [(f.dtype, f.nullable) for f in plan.schema()[3:]] == [(DType.UINT64, False), (DType.FLOAT64, False), (DType.INT64, True), (DType.INT64, True), (DType.INT64, True), (DType.UINT64, False),
                                                                 (DType.UINT64, False)]
    out = plan.execute()
    assert len(out) == 1 and [f.name for f in out[0].fields] == names
    whole = obu.concat_columns(batches)
    host = out[0].table.to_host()
    obu.assert_same_rows(host[:3], whole, what="the input's columns, in input order")
    model = wx.window_ex(whole, [0], [(1, True, True)], [wx.old(W.RowNumber), wx.agg(WX.Sum, 2, -6, 0), wx.lag(2, 2), wx.lead(2, 1, -5), wx.first(2, -1, None), wx.ntile(4), wx.old(W.Count, 2, F.Range)])
    wx.assert_matches_ex(host[3:], model, what="three batches")


def test_expression_argument_through_the_mirror(pp, ctx):
    n = T + 5
    rng = np.random.default_rng(31)
    v = np.round(rng.uniform(0, 100, n), 0)
    fields = [Field("id", DType.INT64, False), Field("v", DType.FLOAT64, False)]
    cols = [i64(rng.integers(0, 40, n)), Column.from_numpy(v)]
    lit = lambda x: PhysicalLiteralExpr.create(x)
    part = PhysicalBinaryExpr.create(_col("id"), Operator.Modulos, lit(ScalarValue.Int64(7)))
    arg = PhysicalBinaryExpr.create(_col("v"), Operator.Multiply, lit(ScalarValue.Float64(2.0)))
    X = pp.WindowFunctionEx
    plan = pp.PhysicalWindowPlanEx.create(_mem(pp, ctx, fields, [cols]), [part], [pp.PhysicalSortExpr(_col("v"))],
                                          [X(WX.Avg, arg, FX.RowsBetween, start=-2, end=2), X(WX.Lag, arg, offset=1, default=ScalarValue.Float64(-1.0)), X(WX.LastValue, arg, FX.Rows)])
    out = plan.execute()
    assert len(out) == 1 and out[0].num_columns == 5 and [f.name for f in out[0].fields][:2] == ["id", "v"]  # the temporaries never reach the output
    with_temps = cols + [i64(cols[0].to_numpy() % 7), Column.from_numpy(v * 2.0)]
    host = out[0].table.to_host()
    obu.assert_same_rows(host[:2], cols, what="input columns")
    wx.assert_matches_ex(host[2:], wx.window_ex(with_temps, [2], [1], [wx.agg(WX.Avg, 3, -2, 2), wx.lag(3, 1, -1.0), wx.last(3, frame=FX.Rows)]), what="expression argument")
    with pytest.raises(ErrorCode) as e:  # Q6: no coercion of the default
        pp.PhysicalWindowPlanEx.create(_mem(pp, ctx, fields, [cols]), [], [], [X(WX.Lag, _col("v"), offset=1, default=ScalarValue.Int64(1))]).execute()
    assert e.value.status == Status.IntervalError


def test_golden_queries_through_the_python_mirror(pp, ctx):
    from naive_query_engine_amd.rewrite import NaiveDB, plan_shape, rewrite

    with open(os.path.join(GOLDEN, "window_ex_expected.json")) as f:
        queries = json.load(f)["queries"]
    db = NaiveDB()
    db.create_csv_table("employee", os.path.join(GOLDEN, "employee.csv"))
    db.create_csv_table("rank", os.path.join(GOLDEN, "rank.csv"))
    for q in queries:
        plan = wx.plan_from_golden(pp, db.scan(q["table"]), q)
        assert plan_shape(rewrite(plan)) == ["PhysicalWindowPlanEx", "ScanPlan"]
        for out in (plan.execute(), db.run_plan(plan)):
            assert len(out) == 1 and [f.name for f in out[0].fields] == q["columns"], q["name"]
            rows = [list(r) for r in zip(*[c.to_list() for c in out[0].table.to_host()])]
            assert rows == q["rows"], q["name"]


# ----------------------------------------------------------------------------- errors
def test_errors_launch_nothing(pp, ctx):
    from naive_query_engine_amd import capi

    cols = [i64(np.arange(10)), obu.utf8_column([b"x"] * 10), Column.from_numpy(np.arange(10) % 2 == 0), Column.from_numpy(np.arange(10.0))]
    t = ctx.table_from_host(cols)

    def refused(status, text, *args):
        with pytest.raises(ErrorCode) as e:
            ctx.window_ex(t, *args)
        assert e.value.status == status and text in str(e.value), (args, str(e.value))

    S = capi.NqeWindowSpecEx
    with Launches(ctx) as L:
        fn = capi.lib().nqe_window_execute_ex
        h = C.c_void_p()
        one = (S * 1)(S(0, 0, 0, 0, 0, 0, 0))
        ints = (C.c_int32 * 1)(0)
        key = (capi.NqeSortKey * 1)(capi.NqeSortKey(0, 0, 1))
        for args in ((None, t.handle, None, 0, None, 0, one, 1, C.byref(h)), (ctx.handle, None, None, 0, None, 0, one, 1, C.byref(h)),
                     (ctx.handle, t.handle, None, 0, None, 0, one, 1, None), (ctx.handle, t.handle, None, 1, None, 0, one, 1, C.byref(h)),
                     (ctx.handle, t.handle, ints, 1, None, 1, one, 1, C.byref(h)), (ctx.handle, t.handle, ints, 1, key, 1, None, 1, C.byref(h))):
            assert fn(*args) == Status.InvalidArgument and not h.value
        for bad in ([S(13, 0, 0)], [S(-1, 0, 0)], [S(4, 0, 4)], [S(10, 0, -1)], [S(0, 0, 0)] * 17 + [S(7, 0, 7)]):  # the enum check comes before the limits
            refused(Status.InvalidArgument, "window: unknown", [0], [0], bad)
        refused(Status.InvalidArgument, "cannot start at UNBOUNDED FOLLOWING", [0], [0], [S(4, 99, 3, 0, I64_MAX, I64_MAX)])
        refused(Status.InvalidArgument, "cannot end at UNBOUNDED PRECEDING", [0], [0], [S(11, 99, 3, 0, I64_MIN, I64_MIN)])
        refused(Status.InvalidArgument, "start lies behind its end", [0], [0], [wx.agg(WX.Sum, 99, 1, 0)])
        refused(Status.InvalidArgument, "offset of lag / lead is negative", [0], [0], [wx.lag(99, -1)])
        refused(Status.InvalidArgument, "ntile needs at least one bucket", [0], [0], [wx.ntile(0)])
        refused(Status.PlanError, "the list of window functions is empty", [0], [0], [])
        refused(Status.NotSupported, "at most 8 partition keys", [0] * 9, [], [wx.ntile(2)])
        refused(Status.NotSupported, "at most 8 partition keys", [], [0] * 9, [wx.ntile(2)])
        refused(Status.NotSupported, "at most 16 window functions", [0], [0], [wx.ntile(2)] * 17)
        for parts, order in (([4], []), ([-1], []), ([], [4]), ([0], [(0, True), -1])):
            refused(Status.NotSupported, "window: key column index out of range", parts, order, [wx.lag(0, 1)])
        for c in (4, -1):
            refused(Status.NotSupported, "aggregate column index out of range", [0], [0], [wx.ntile(2), wx.agg(WX.Sum, c, -1, 1)])
            refused(Status.NotSupported, "window: value column index out of range", [0], [0], [wx.ntile(2), S(8, c, 0, 0, 0, 0, 1)])
        for f in wx.AGGREGATES:
            for c in (1, 2):  # Utf8, Boolean
                refused(Status.NotSupported, "aggregate func for this column type is not supported", [0], [0], [wx.agg(f, c, -1, 1)])
        assert L.count("") == 0  # nothing was launched
    assert ctx.window_ex(t, [0], [0], [S(12, 99, 99, 0, 5, -5, 3)]).num_columns == 1  # NTILE reads neither column nor frame
    assert ctx.window_ex(t, [0] * 8, [0] * 8, [wx.lag(3, 1)] * 16).num_columns == 16  # the limits themselves are fine
    fields = [Field("a", DType.INT64, False), Field("s", DType.UTF8, False), Field("b", DType.BOOLEAN, False), Field("f", DType.FLOAT64, False)]
    with pytest.raises(ErrorCode) as e:
        pp.PhysicalWindowPlanEx.create(pp.ScanPlan.create(pp.MemTable(fields, []), None), [], [], [pp.WindowFunctionEx(WX.Rank)]).execute()
    assert e.value.status == Status.NotSupported
    with pytest.raises(ErrorCode) as e:
        pp.PhysicalWindowPlanEx.create(_mem(pp, ctx, fields, [cols]), [], [], []).execute()
    assert e.value.status == Status.PlanError
