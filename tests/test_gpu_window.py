"""Window functions on the device (nqe_window_execute, csrc/window.hip; quirk Q23).

The yardstick is the row-at-a-time model of tests/window_util.py (checked against agg_value_util's per-group state and against
sqlite3 in tests/test_window_model.py).  Ranking functions, count, min and max must be equal; sum and avg must lie within the derived
bound n_frame * 2^-52 * sum|x| of the frame's finite values.  Every input is shuffled by a seeded permutation, so the scatter back to
input order is exercised everywhere.  T is the scan's tile, read from csrc/window_plan.hpp.

Not run here: the 2^32-row bound needs a 32 GB table; it is checked on the CPU (tests/cpp/test_window_plan.cpp)."""
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
import window_util as wu  # noqa: E402
from naive_query_engine_amd import (Column, ColumnExpr, DType, ErrorCode, Field, Operator, PhysicalBinaryExpr, PhysicalLiteralExpr, PhysicalUnaryExpr,  # noqa: E402
                                    RecordBatch, ScalarValue, Status, UnaryOperator, WindowFrame as F, WindowFunc as W)

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(ROOT, "tests", "golden")
T = int(re.search(r"constexpr int64_t WIN_TILE = (\d+);", open(os.path.join(ROOT, "naive_query_engine_amd", "csrc", "window_plan.hpp")).read()).group(1))
RANKS = [(W.RowNumber,), (W.Rank,), (W.DenseRank,)]
SCAN_LABELS = ("win_scan_reduce", "win_scan_carry", "win_scan_apply")


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


def check(ctx, cols, parts, order, funcs, what=""):
    """device against model; returns the device's columns"""
    model = wu.window(cols, parts, order, funcs)
    got = ctx.window(ctx.table_from_host(cols), parts, order, funcs).to_host()
    wu.assert_matches_window(got, model, what=f"{what} partition by {parts} order by {order}")
    return got


def i64(a):
    return Column.from_numpy(np.asarray(a, dtype=np.int64))


# ----------------------------------------------------------------------------- row counts
ROW_COUNTS = sorted({0, 1, 2, 4096, 4097, T - 1, T, T + 1, 3 * T + 5})  # the sort's two paths, the tile's edges, several tiles


@pytest.mark.parametrize("n", ROW_COUNTS)
def test_row_counts_at_the_sort_paths_and_the_tiles_edges(ctx, n):
    rng = np.random.default_rng(n)
    cols = shuffled([i64(rng.integers(0, 5, n)), obu.random_column(rng, DType.FLOAT64, n, True, 5), Column.from_numpy(rng.integers(-1000, 1000, n).astype(np.int64), rng.random(n) > 0.1)], n)
    funcs = RANKS + wu.ALL_AGGS(2, F.Rows) + [(W.Sum, 2, F.Range), (W.Sum, 2, F.Partition)]
    got = check(ctx, cols, [0], [(1, True, False)], funcs, what=f"n={n}")
    assert len(got) == len(funcs) and all(c.length == n for c in got)  # zero rows: a 0-row table with every column
    check(ctx, cols, [], [1], funcs, what=f"n={n} one partition")


def test_two_hundred_thousand_rows(ctx):
    n = 200_000
    rng = np.random.default_rng(7)
    v = np.round(rng.normal(0, 1e3, n), 2)
    cols = shuffled([i64(rng.integers(0, 1000, n)), Column.from_numpy(v), Column.from_numpy(rng.integers(-10 ** 12, 10 ** 12, n).astype(np.int64), rng.random(n) > 0.1)], 8)
    with Launches(ctx) as L:
        check(ctx, cols, [0], [1], RANKS + [(W.Sum, 1, F.Rows), (W.Count, 2, F.Range), (W.Max, 2, F.Partition), (W.Avg, 2, F.Rows), (W.Min, 1, F.Range)], what="2e5 rows")
        assert [L.count(s) for s in SCAN_LABELS] == [2, 2, 2] and L.count("win_gather") == 2 and L.count("win_emit") == 1 and L.count("win_bounds") == 1


# ----------------------------------------------------------------------------- partition layouts by explicit lengths
def _layout_case(name):
    n = 3 * T + 5
    if name == "one_partition":
        return n, None
    if name == "every_row_its_own":
        return n, np.arange(n)
    lengths = [T - 1, 1, 2 * T + 3, T, 5]  # starts on a tile's last row (T - 1) and first row (T); rows T .. 3T + 2 are one partition whose middle tile has no start
    assert sum(lengths) == 4 * T + 8
    return sum(lengths), np.repeat(np.arange(len(lengths)), lengths)


@pytest.mark.parametrize("layout", ["one_partition", "every_row_its_own", "lengths"])
def test_partition_layouts(ctx, layout):
    n, key = _layout_case(layout)
    rng = np.random.default_rng(len(layout))
    # the order key is the built position: the sorted order is the built order, so the partitions start where the lengths put them
    cols = [i64(np.zeros(n) if key is None else key), i64(np.arange(n)), Column.from_numpy(rng.normal(0, 100, n), rng.random(n) > 0.1), i64(rng.integers(-50, 50, n))]
    cols = shuffled(cols, 3)
    funcs = RANKS + wu.ALL_AGGS(2, F.Rows) + wu.ALL_AGGS(2, F.Partition) + [(W.Sum, 3, F.Range), (W.Max, 3, F.Rows)]
    with Launches(ctx) as L:
        check(ctx, cols, [] if key is None else [0], [1], funcs, what=layout)
        assert [L.count(s) for s in SCAN_LABELS] == [2, 2, 2]  # more than one tile: reduce, carry, apply — once per value column
        assert [L.count(s) for s in ("win_pos_reduce", "win_pos_carry", "win_pos_apply")] == [1, 1, 1]
        assert L.count("win_gather") == 2 and L.count("win_emit") == 1


def test_a_single_tile_runs_the_apply_pass_alone(ctx):
    cols = shuffled([i64(np.arange(T) % 7), i64(np.arange(T))], 1)
    with Launches(ctx) as L:
        check(ctx, cols, [0], [1], [(W.Sum, 1, F.Rows)], what="one tile")
        assert [L.count(s) for s in SCAN_LABELS] == [0, 0, 1]


# ----------------------------------------------------------------------------- peers
def test_peer_groups_straddle_tile_edges(ctx):
    n = 2 * T + 1
    rng = np.random.default_rng(2)
    cols = shuffled([i64(rng.integers(0, 3, n)), Column.from_numpy(rng.normal(0, 10, n), rng.random(n) > 0.2)], 4)  # three peer groups over two tiles and a row
    funcs = RANKS + wu.ALL_AGGS(1, F.Range) + wu.ALL_AGGS(1, F.Rows)
    got = check(ctx, cols, [], [0], funcs, what="three peer groups")
    assert sorted(set(got[2].to_numpy().tolist())) == [1, 2, 3]
    check(ctx, cols, [], [(0, True)], funcs, what="three peer groups, descending")


def test_no_order_keys_all_rows_of_a_partition_are_peers(ctx):
    n = T + 77
    rng = np.random.default_rng(6)
    key = rng.integers(0, 4, n)
    cols = [i64(key), Column.from_numpy(rng.normal(0, 10, n))]
    got = check(ctx, cols, [0], [], RANKS + [(W.Sum, 1, F.Range), (W.Sum, 1, F.Partition), (W.Sum, 1, F.Rows), (W.Count, 1, F.Range), (W.Count, 1, F.Partition)], what="no order keys")
    assert (got[1].to_numpy() == 1).all() and (got[2].to_numpy() == 1).all()
    rn = got[0].to_numpy()
    for k in range(4):
        assert rn[key == k].tolist() == list(range(1, int((key == k).sum()) + 1))  # ROW_NUMBER in input order
    assert (got[3].to_numpy().view(np.uint64) == got[4].to_numpy().view(np.uint64)).all() and (got[6].to_numpy() == got[7].to_numpy()).all()  # RANGE = PARTITION
    got = check(ctx, cols, [], [], RANKS + [(W.Sum, 1, F.Rows)], what="no keys at all")
    assert got[0].to_numpy().tolist() == list(range(1, n + 1))


def test_no_keys_at_all_launches_no_sort(ctx):
    cols = [Column.from_numpy(np.random.default_rng(1).normal(0, 1, 2 * T))]
    with Launches(ctx) as L:
        check(ctx, cols, [], [], [(W.RowNumber,), (W.Avg, 0, F.Rows)], what="no keys")
        assert L.count("ob_") == 0 and L.count("radix_") == 0 and L.count("bitonic_small") == 0 and L.count("win_emit") == 1


# ----------------------------------------------------------------------------- the cancellation trap
def test_infinities_and_nan_of_the_first_partition_do_not_reach_the_later_ones(ctx):
    lengths = [T + 3, 5, 2 * T, 40]
    n = sum(lengths)
    rng = np.random.default_rng(12)
    key = np.repeat(np.arange(len(lengths)), lengths)
    v = rng.uniform(-1e6, 1e6, n)
    first = np.nonzero(key == 0)[0]
    v[first[::3]], v[first[1::3]], v[first[2::3]] = np.inf, -np.inf, np.nan
    cols = shuffled([i64(key), i64(np.arange(n)), Column.from_numpy(v)], 5)
    funcs = [(f, 2, fr) for fr in wu.FRAMES for f in (W.Sum, W.Avg, W.Max, W.Min, W.Count)]
    got = check(ctx, cols, [0], [1], funcs, what="trap")
    later = cols[0].to_numpy() > 0
    for i, (f, _, fr) in enumerate(funcs):
        if f in (W.Sum, W.Avg, W.Max):
            assert np.isfinite(got[i].to_numpy()[later]).all(), (f, fr)  # "global prefix minus the prefix at the start" would give NaN here
    assert np.isnan(got[0].to_numpy()[(cols[0].to_numpy() == 0)]).all()  # sum over the whole first partition


# ----------------------------------------------------------------------------- Q10's value domains
@pytest.mark.parametrize("domain,nullable", avu.VARIANTS, ids=avu.VARIANT_IDS)
def test_value_domains_through_all_aggregates_and_frames(ctx, domain, nullable):
    n = 3 * T + 5
    rng = np.random.default_rng(100 + avu.DOMAINS.index(domain) * 2 + nullable)
    v, mask = avu.gen_values(domain, rng, n, nullable)
    cols = shuffled([i64(rng.integers(0, 6, n)), i64(rng.integers(0, 50, n)), Column.from_numpy(v, mask)], 9)
    check(ctx, cols, [0], [1], [(f, 2, fr) for fr in wu.FRAMES for f in wu.AGGREGATES], what=f"{domain} nullable={nullable}")


def test_frames_of_nothing_but_nulls_give_the_start_values(ctx):
    n = T + 9
    rng = np.random.default_rng(3)
    key = rng.integers(0, 3, n)
    mask = key != 1  # partition 1: nothing but NULL
    cols = [i64(key), i64(rng.integers(0, 4, n)), Column.from_numpy(rng.normal(0, 1, n), mask), Column.from_numpy(rng.integers(0, 9, n).astype(np.uint64), np.zeros(n, dtype=bool))]
    got = check(ctx, cols, [0], [1], wu.ALL_AGGS(2, F.Rows) + wu.ALL_AGGS(3, F.Partition) + wu.ALL_AGGS(2, F.Range), what="all-NULL frames")
    empty = key == 1
    for base, rows in ((0, empty), (5, np.ones(n, dtype=bool))):  # count, sum, min, max, avg
        assert (got[base].to_numpy()[rows] == 0).all() and (got[base + 1].to_numpy()[rows] == 0.0).all()
        assert (got[base + 2].to_numpy()[rows] == avu.F64_MAX).all() and (got[base + 3].to_numpy()[rows] == -avu.F64_MAX).all() and np.isnan(got[base + 4].to_numpy()[rows]).all()


# ----------------------------------------------------------------------------- keys
def test_null_partition_keys_form_one_partition(ctx):
    n = T + 100
    rng = np.random.default_rng(14)
    cols = shuffled([obu.random_column(rng, DType.INT64, n, True, 5), obu.random_column(rng, DType.UTF8, n, True, 4), i64(rng.integers(0, 100, n))], 2)
    for parts in ([0], [1], [0, 1]):
        got = check(ctx, cols, parts, [2], RANKS + [(W.Count, 2, F.Partition), (W.Sum, 2, F.Rows)], what="NULL partition keys")
    nulls = ~cols[0].valid_mask() & ~cols[1].valid_mask()
    assert nulls.sum() > 1 and len(set(got[3].to_numpy()[nulls].tolist())) == 1 and got[3].to_numpy()[nulls][0] == nulls.sum()


@pytest.mark.parametrize("descending", [False, True])
@pytest.mark.parametrize("nulls_first", [False, True])
def test_null_order_keys_are_peers(ctx, descending, nulls_first):
    n = T + 50
    rng = np.random.default_rng(15)
    cols = shuffled([i64(rng.integers(0, 3, n)), obu.random_column(rng, DType.INT64, n, True, 5), obu.random_column(rng, DType.FLOAT64, n, True, 5), i64(rng.integers(0, 100, n))], 3)
    for k in (1, 2):
        got = check(ctx, cols, [0], [(k, descending, nulls_first)], RANKS + [(W.Sum, 3, F.Range), (W.Count, 3, F.Range), (W.Sum, 3, F.Rows)], what=f"NULL order key {k}")
        nulls, part = ~cols[k].valid_mask(), cols[0].to_numpy()
        for p in range(3):
            assert len(set(got[1].to_numpy()[nulls & (part == p)].tolist())) == 1  # one rank for all the partition's NULLs


def test_float64_keys_zeros_and_nan_bit_patterns_fall_into_one_partition(ctx):
    n = T + 300
    rng = np.random.default_rng(16)
    pool = np.concatenate([np.array([0.0, -0.0, 1.5, -2.5, np.inf]).view(np.uint64), obu.NAN_BITS]).view(np.float64)
    k = pool[rng.integers(0, pool.size, n)].copy()
    cols = shuffled([Column.from_numpy(k), Column.from_numpy(k.copy(), rng.random(n) > 0.2), i64(rng.integers(0, 10, n))], 4)
    got = check(ctx, cols, [0], [2], RANKS + [(W.Count, 2, F.Partition)], what="Float64 partition key")
    kk = cols[0].to_numpy()
    assert set(got[3].to_numpy()[np.isnan(kk)].tolist()) == {int(np.isnan(kk).sum())} and set(got[3].to_numpy()[kk == 0.0].tolist()) == {int((kk == 0.0).sum())}
    check(ctx, cols, [], [1, 2], RANKS + [(W.Sum, 2, F.Range)], what="Float64 order key with NULLs")
    check(ctx, cols, [1], [(0, True, False)], RANKS + [(W.Max, 0, F.Range), (W.Min, 1, F.Rows)], what="Float64 keys as values")


def test_utf8_keys(ctx):
    n = T + 200
    rng = np.random.default_rng(17)
    cols = shuffled([obu.random_column(rng, DType.UTF8, n, True), obu.random_column(rng, DType.UTF8, n, False, 6), obu.random_column(rng, DType.BOOLEAN, n, True),
                     Column.from_numpy(rng.normal(0, 5, n))], 5)
    assert set(obu.column_values(cols[0])) >= set(obu.WORDS)
    funcs = RANKS + [(W.Sum, 3, F.Range), (W.Count, 3, F.Partition)]
    check(ctx, cols, [0], [(1, True)], funcs, what="Utf8 partition and order keys")
    check(ctx, cols, [1, 2], [(0, False, False)], funcs, what="Utf8, Boolean partition keys, Utf8 order key with NULLs last")


def test_two_partition_keys_and_two_order_keys_with_heavy_ties(ctx):
    n = 2 * T + 11
    rng = np.random.default_rng(18)
    cols = shuffled([obu.random_column(rng, DType.INT64, n, True, 3), obu.random_column(rng, DType.UTF8, n, True, 3), obu.random_column(rng, DType.FLOAT64, n, True, 4),
                     obu.random_column(rng, DType.UINT64, n, False, 3), Column.from_numpy(rng.normal(0, 5, n), rng.random(n) > 0.1)], 6)
    check(ctx, cols, [0, 1], [(2, True, False), (3, False, True)], RANKS + wu.ALL_AGGS(4, F.Range) + wu.ALL_AGGS(4, F.Rows), what="2 + 2 keys")


def test_the_same_column_as_partition_key_order_key_and_value(ctx):
    n = T + 31
    rng = np.random.default_rng(19)
    cols = shuffled([obu.random_column(rng, DType.INT64, n, True, 9)], 7)
    got = check(ctx, cols, [0], [0], RANKS + wu.ALL_AGGS(0, F.Range) + [(W.Sum, 0, F.Rows)], what="one column three times")
    assert (got[1].to_numpy() == 1).all()  # inside a partition every row ties on the order key too


def test_sixteen_functions_four_over_the_same_column(ctx):
    n = 2 * T + 3
    rng = np.random.default_rng(20)
    cols = shuffled([i64(rng.integers(0, 9, n)), i64(rng.integers(0, 30, n)), Column.from_numpy(rng.normal(0, 5, n), rng.random(n) > 0.1), i64(rng.integers(-9, 9, n)),
                     Column.from_numpy(rng.integers(0, 2 ** 63, n, dtype=np.uint64) * np.uint64(2))], 8)
    funcs = RANKS + [(W.Sum, 2, F.Rows), (W.Sum, 2, F.Range), (W.Avg, 2, F.Partition), (W.Min, 2, F.Rows), (W.Count, 3, F.Rows), (W.Max, 3, F.Range), (W.Avg, 3, F.Rows),
                     (W.Sum, 4, F.Partition), (W.Max, 4, F.Rows), (W.Min, 4, F.Range), (W.Count, 4, F.Partition), (W.Sum, 1, F.Rows), (W.RowNumber,)]
    assert len(funcs) == 16
    with Launches(ctx) as L:
        check(ctx, cols, [0], [1], funcs, what="sixteen functions")
        assert L.count("win_gather") == 4 and L.count("win_scan_apply") == 4 and L.count("win_emit") == 1  # one gather and one scan per distinct column


# ----------------------------------------------------------------------------- the mirror
def _mem(pp, ctx, fields, batches):
    return pp.ScanPlan.create(pp.MemTable.try_create(fields, [RecordBatch(fields, b) for b in batches], ctx), None)


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
    funcs = [pp.WindowFunction(W.RowNumber), pp.WindowFunction(W.Sum, ColumnExpr.try_create("v", None), F.Rows), pp.WindowFunction(W.Count, ColumnExpr.try_create("v", None))]
    plan = pp.PhysicalWindowPlan.create(_mem(pp, ctx, fields, batches), [ColumnExpr.try_create("k", None)], [pp.PhysicalSortExpr(ColumnExpr.try_create("o", None), descending=True)], funcs)
    assert [f.name for f in plan.schema()] == ["k", "o", "v", "row_number()", "sum(v)", "count(v)"]
    out = plan.execute()
    assert len(out) == 1 and [f.name for f in out[0].fields] == ["k", "o", "v", "row_number()", "sum(v)", "count(v)"]
    whole = obu.concat_columns(batches)
    host = out[0].table.to_host()
    obu.assert_same_rows(host[:3], whole, what="the input's columns, in input order")
    wu.assert_matches_window(host[3:], wu.window(whole, [0], [(1, True, True)], [(W.RowNumber,), (W.Sum, 2, F.Rows), (W.Count, 2, F.Range)]), what="three batches")


def test_expression_key_and_expression_argument_through_the_mirror(pp, ctx):
    n = T + 5
    rng = np.random.default_rng(31)
    v = np.round(rng.uniform(0, 100, n), 0)
    fields = [Field("id", DType.INT64, False), Field("v", DType.FLOAT64, False)]
    cols = [i64(rng.integers(0, 40, n)), Column.from_numpy(v)]
    lit = lambda x: PhysicalLiteralExpr.create(x)
    part = PhysicalBinaryExpr.create(ColumnExpr.try_create("id", None), Operator.Modulos, lit(ScalarValue.Int64(7)))
    key = PhysicalUnaryExpr.create(PhysicalBinaryExpr.create(ColumnExpr.try_create("v", None), Operator.Minus, lit(ScalarValue.Float64(50.0))), UnaryOperator.Abs, "abs", None)
    arg = PhysicalBinaryExpr.create(ColumnExpr.try_create("v", None), Operator.Multiply, lit(ScalarValue.Float64(2.0)))
    plan = pp.PhysicalWindowPlan.create(_mem(pp, ctx, fields, [cols]), [part], [pp.PhysicalSortExpr(key)], [pp.WindowFunction(W.Rank), pp.WindowFunction(W.Sum, arg, F.Rows)])
    out = plan.execute()
    assert len(out) == 1 and out[0].num_columns == 4 and [f.name for f in out[0].fields][:3] == ["id", "v", "rank()"]  # the temporaries never reach the output
    with_temps = cols + [i64(cols[0].to_numpy() % 7), Column.from_numpy(np.abs(v - 50.0)), Column.from_numpy(v * 2.0)]
    host = out[0].table.to_host()
    obu.assert_same_rows(host[:2], cols, what="input columns")
    wu.assert_matches_window(host[2:], wu.window(with_temps, [2], [3], [(W.Rank,), (W.Sum, 4, F.Rows)]), what="expression key and argument")


def test_golden_queries_through_the_python_mirror(pp, ctx):
    from naive_query_engine_amd.rewrite import NaiveDB, plan_shape, rewrite

    with open(os.path.join(GOLDEN, "window_expected.json")) as f:
        queries = json.load(f)["queries"]
    db = NaiveDB()
    db.create_csv_table("employee", os.path.join(GOLDEN, "employee.csv"))
    db.create_csv_table("rank", os.path.join(GOLDEN, "rank.csv"))
    for q in queries:
        col = lambda name: ColumnExpr.try_create(name, None)
        funcs = [pp.WindowFunction(W[f["func"]], None if f["column"] is None else col(f["column"]), F[f["frame"]]) for f in q["funcs"]]
        plan = pp.PhysicalWindowPlan.create(db.scan(q["table"]), [col(c) for c in q["partition_by"]],
                                            [pp.PhysicalSortExpr(col(k["column"]), k["descending"], k["nulls_first"]) for k in q["order_by"]], funcs)
        assert plan_shape(rewrite(plan)) == ["PhysicalWindowPlan", "ScanPlan"]
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
            ctx.window(t, *args)
        assert e.value.status == status and text in str(e.value), (args, str(e.value))

    with Launches(ctx) as L:
        fn = capi.lib().nqe_window_execute
        h = C.c_void_p()
        one = (capi.NqeWindowSpec * 1)(capi.NqeWindowSpec(0, 0, 0))
        ints = (C.c_int32 * 1)(0)
        key = (capi.NqeSortKey * 1)(capi.NqeSortKey(0, 0, 1))
        for args in ((None, t.handle, None, 0, None, 0, one, 1, C.byref(h)), (ctx.handle, None, None, 0, None, 0, one, 1, C.byref(h)),
                     (ctx.handle, t.handle, None, 0, None, 0, one, 1, None), (ctx.handle, t.handle, None, 1, None, 0, one, 1, C.byref(h)),
                     (ctx.handle, t.handle, ints, 1, None, 1, one, 1, C.byref(h)), (ctx.handle, t.handle, ints, 1, key, 1, None, 1, C.byref(h))):
            assert fn(*args) == Status.InvalidArgument and not h.value
        for bad in ([(8,)], [(-1,)], [(W.Sum, 0, 3)], [(W.Sum, 0, -1)], [(W.RowNumber,)] * 17 + [(W.Avg, 0, 7)]):  # the enum check comes before the limits
            refused(Status.InvalidArgument, "window: unknown", [0], [0], bad)
        refused(Status.PlanError, "the list of window functions is empty", [0], [0], [])
        refused(Status.NotSupported, "at most 8 partition keys", [0] * 9, [], [(W.Rank,)])
        refused(Status.NotSupported, "at most 8 partition keys", [], [0] * 9, [(W.Rank,)])
        refused(Status.NotSupported, "at most 16 window functions", [0], [0], [(W.Rank,)] * 17)
        for parts, order in (([4], []), ([-1], []), ([], [4]), ([0], [(0, True), -1])):
            refused(Status.NotSupported, "window: key column index out of range", parts, order, [(W.Rank,)])
        for c in (4, -1):
            refused(Status.NotSupported, "aggregate column index out of range", [0], [0], [(W.Rank,), (W.Sum, c, F.Rows)])
        for f in wu.AGGREGATES:
            for c in (1, 2):  # Utf8, Boolean
                refused(Status.NotSupported, "aggregate func for this column type is not supported", [0], [0], [(f, c, F.Rows)])
        assert L.count("") == 0  # nothing was launched
    assert ctx.window(t, [0], [0], [(W.Rank, 99, 99)]).num_columns == 1  # column and frame are ignored by the ranking functions
    assert ctx.window(t, [0] * 8, [0] * 8, [(W.Rank,)] * 16).num_columns == 16  # the limits themselves are fine
    fields = [Field("a", DType.INT64, False), Field("s", DType.UTF8, False), Field("b", DType.BOOLEAN, False), Field("f", DType.FLOAT64, False)]
    empty = pp.ScanPlan.create(pp.MemTable(fields, []), None)
    with pytest.raises(ErrorCode) as e:
        pp.PhysicalWindowPlan.create(empty, [], [], [pp.WindowFunction(W.Rank)]).execute()
    assert e.value.status == Status.NotSupported
    with pytest.raises(ErrorCode) as e:
        pp.PhysicalWindowPlan.create(_mem(pp, ctx, fields, [cols]), [], [], []).execute()
    assert e.value.status == Status.PlanError
