"""ORDER BY on the device (nqe_sort_execute, csrc/order_by.hip; quirk Q18: arrow-rs' lexsort_to_indices followed by take).

The yardstick is the pure-Python model of tests/order_by_util.py (Python's stable `sorted` over per-row key tuples; checked against
pyarrow in tests/test_order_by_host.py).  Every comparison is value for value, Float64 bit for bit: the operator only orders and copies.

Not run here: the 2^32-row bound needs a 32 GB table.  It is the first statement after the key checks of nqe_sort_execute and stands in
front of every allocation; that is left to code reading."""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import order_by_util as obu  # noqa: E402
from naive_query_engine_amd import (Column, ColumnExpr, DType, ErrorCode, Field, Operator, PhysicalBinaryExpr, PhysicalLiteralExpr,  # noqa: E402
                                    PhysicalUnaryExpr, RecordBatch, ScalarValue, Status, UnaryOperator)

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
I64 = np.iinfo(np.int64)


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


def rownum(n):
    return Column.from_numpy(np.arange(n, dtype=np.int64))


def check(ctx, cols, keys, fetch=None, what=""):
    """device against model; returns the device's columns"""
    t = ctx.table_from_host(cols)
    got = ctx.order_by(t, keys, fetch).to_host()
    obu.assert_same_rows(got, obu.order_by(cols, keys, fetch), what=f"{what} keys {keys} fetch {fetch}")
    return got


ROW_COUNTS = [0, 1, 2, 4096, 4097, 6143, 6144, 6145]  # sort.hip: one-workgroup sort up to 4096 rows, 2048-key radix tiles above


# ----------------------------------------------------------------------------- row counts and key types
@pytest.mark.parametrize("n", ROW_COUNTS)
def test_row_counts_at_the_sort_paths_edges(ctx, n):
    rng = np.random.default_rng(n)
    cols = [Column.from_numpy(rng.integers(-50, 50, n).astype(np.int64)), obu.random_column(rng, DType.FLOAT64, n, True, 5), rownum(n)]
    check(ctx, cols, [0], what=f"n={n} one key")
    check(ctx, cols, [(1, True, False), (0, False, True)], what=f"n={n} two keys")  # later passes read through the permutation


def test_two_hundred_thousand_rows(ctx):
    n = 200_003
    rng = np.random.default_rng(7)
    cols = [Column.from_numpy(rng.integers(I64.min, I64.max, n, dtype=np.int64)), Column.from_numpy(rng.integers(0, 1000, n).astype(np.int64)),
            Column.from_numpy(rng.normal(0, 1, n), rng.random(n) > 0.1), rownum(n)]
    check(ctx, cols, [1, (2, True, False)], what="2e5 rows, two keys")
    check(ctx, cols, [0], what="2e5 rows, full-range key")


@pytest.mark.parametrize("n", [4096, 6145])
def test_int64_full_range_uint64_above_2p63_and_small_keys(ctx, n):
    rng = np.random.default_rng(n + 1)
    full = rng.integers(I64.min, I64.max, n, dtype=np.int64, endpoint=True)
    full[[0, 1, n // 2, n - 1]] = [I64.max, I64.min, I64.min, I64.max]  # all eight digit passes
    big = rng.integers(2 ** 63 - 5, 2 ** 64 - 1, n, dtype=np.uint64, endpoint=True)
    big[[0, n - 1]] = [2 ** 64 - 1, 0]
    small = rng.integers(0, 256, n).astype(np.int64)  # seven of eight digit passes are one bucket
    cols = [Column.from_numpy(full), Column.from_numpy(big), Column.from_numpy(small), rownum(n)]
    for k in range(3):
        check(ctx, cols, [k], what=f"n={n} column {k}")
        check(ctx, cols, [(k, True)], what=f"n={n} column {k} descending")


@pytest.mark.parametrize("n", [300, 5000])
def test_float64_zeros_infinities_subnormals_and_nans(ctx, n):
    rng = np.random.default_rng(n)
    pool = np.concatenate([obu.SPECIAL_F64.view(np.uint64), obu.NAN_BITS]).view(np.float64)
    v = pool[rng.integers(0, pool.size, n)].copy()
    mask = rng.random(n) > 0.15
    cols = [Column.from_numpy(v), Column.from_numpy(v.copy(), mask), rownum(n)]
    for desc in (False, True):
        got = check(ctx, cols, [(0, desc)], what=f"n={n} desc={desc}")
        assert np.isnan(got[0].to_numpy()[0 if desc else -1])  # NaN is greater than +inf
        for nf in (False, True):
            check(ctx, cols, [(1, desc, nf)], what=f"n={n} nullable desc={desc} nulls_first={nf}")


def test_two_distinct_values_over_ten_thousand_rows_is_stable(ctx):
    n = 10_000
    k = (np.random.default_rng(3).random(n) < 0.5).astype(np.int64) * 7 - 3
    for col in (Column.from_numpy(k), Column.from_numpy(k == 4), Column.from_numpy(k.astype(np.float64))):
        for desc in (False, True):
            got = check(ctx, [col, rownum(n)], [(0, desc)], what=f"{col.dtype} desc={desc}")
            r, first = got[1].to_numpy(), int((k == (4 if desc else -3)).sum())
            assert (np.diff(r[:first]) > 0).all() and (np.diff(r[first:]) > 0).all()  # input order inside each value


@pytest.mark.parametrize("n", [67, 4097])
@pytest.mark.parametrize("descending", [False, True])
@pytest.mark.parametrize("nulls_first", [False, True])
def test_null_keys_at_word_edges_in_all_four_placements(ctx, n, descending, nulls_first):
    rng = np.random.default_rng(n)
    mask = np.ones(n, dtype=bool)
    mask[[0, 63, 64, 65, n - 1]] = False
    full = rng.integers(I64.min, I64.max, n, dtype=np.int64, endpoint=True)  # no spare bit for the flag
    full[[1, 2]] = [I64.min, I64.max]
    strs = [obu.WORDS[i] for i in rng.integers(0, len(obu.WORDS), n)]
    cols = [Column.from_numpy(full, mask), Column.from_numpy(rng.integers(0, 3, n).astype(np.uint64), mask), Column.from_numpy(rng.random(n) < 0.5, mask),
            obu.utf8_column([s if ok else None for s, ok in zip(strs, mask)], null_bytes=b"hidden"), rownum(n)]
    for k in range(4):
        got = check(ctx, cols, [(k, descending, nulls_first)], what=f"n={n} column {k}")
        nulls = got[4].to_numpy()[:5] if nulls_first else got[4].to_numpy()[-5:]
        assert nulls.tolist() == [0, 63, 64, 65, n - 1]  # NULLs tie among themselves: input order


# ----------------------------------------------------------------------------- Utf8 keys
def test_utf8_lengths_embedded_nul_long_prefixes_and_a_null_with_bytes(ctx):
    base = [b"", b"a", b"a\0", b"ab", b"b", b"abcdefg", b"abcdefgh", b"abcdefghi", b"abcdefghijklmnop", b"abcdefghijklmnopq", b"abcdefgh\0", b"abcdefgh\0\0",
            b"abcdefghijklX", b"abcdefghijklY", b"abcdefghijkl", "é".encode(), "ÿ".encode(), b"\x7f", None, b"a", b"", None, b"abcdefghijklmnopq"]
    assert {len(s) for s in base if s is not None} >= {0, 1, 7, 8, 9, 16, 17}
    col = obu.utf8_column(base, null_bytes=b"zzzzzzzzzzzz")  # a NULL whose offsets span twelve bytes
    cols = [col, rownum(len(base))]
    for desc in (False, True):
        for nf in (False, True):
            check(ctx, cols, [(0, desc, nf)], what="utf8")
    got = check(ctx, [obu.utf8_column([b"b", b"ab", b"a\0", b"a", b""]), rownum(5)], [0])
    assert got[1].to_numpy().tolist() == [4, 3, 2, 1, 0]  # "" < "a" < "a\0" < "ab" < "b"
    rng = np.random.default_rng(11)
    n = 5000  # the radix path, with ties
    many = [base[i] for i in rng.integers(0, len(base), n)]
    check(ctx, [obu.utf8_column(many, null_bytes=b"q"), rownum(n)], [(0, True, False)], what="utf8 5000")
    check(ctx, [obu.utf8_column([b"", b"", b""]), rownum(3)], [0], what="only empty strings")


def test_three_mixed_keys_with_heavy_ties(ctx):
    n = 6145
    rng = np.random.default_rng(5)
    cols = [obu.random_column(rng, DType.UTF8, n, True, 4), obu.random_column(rng, DType.FLOAT64, n, True, 5), obu.random_column(rng, DType.BOOLEAN, n, False),
            rownum(n)]
    check(ctx, cols, [(0, True, False), (1, False, True), (2, False, True)], what="Utf8 desc, Float64, Boolean")
    check(ctx, cols, [(2, True), (1, True, False), 0], what="Boolean desc, Float64 desc, Utf8")


def test_the_same_column_named_twice(ctx):
    n = 4500
    rng = np.random.default_rng(9)
    cols = [obu.random_column(rng, DType.INT64, n, True, 17), rownum(n)]
    a = check(ctx, cols, [(0, True, False), (0, False, True)], what="twice")  # the second naming can break no tie the first left
    b = check(ctx, cols, [(0, True, False)], what="once")
    obu.assert_same_rows(a, b, what="twice against once")


# ----------------------------------------------------------------------------- payload columns
@pytest.mark.parametrize("n", [257, 4200])
def test_payload_columns_of_every_dtype_with_validity(ctx, n):
    rng = np.random.default_rng(n)
    pool = np.concatenate([obu.SPECIAL_F64.view(np.uint64), obu.NAN_BITS]).view(np.float64)
    cols = [Column.from_numpy(rng.integers(0, 40, n).astype(np.int64))]
    for dt in obu.ALL_DTYPES:
        for nullable in (False, True):
            cols.append(obu.random_column(rng, dt, n, nullable))
    cols.append(Column.from_numpy(pool[rng.integers(0, pool.size, n)].copy(), rng.random(n) > 0.3))  # NaN payloads survive the take bit for bit
    got = check(ctx, cols, [0], what=f"payloads n={n}")
    assert [c.validity is not None for c in got] == [c.validity is not None for c in cols]


# ----------------------------------------------------------------------------- batches and the mirror
def _mem(pp, ctx, fields, batches):
    return pp.ScanPlan.create(pp.MemTable.try_create(fields, [RecordBatch(fields, b) for b in batches], ctx), None)


def test_three_batches_one_of_them_empty(pp, ctx):
    fields = [Field("k", DType.INT64, True), Field("s", DType.UTF8, True), Field("f", DType.FLOAT64, False), Field("row", DType.INT64, False)]
    rng = np.random.default_rng(21)
    batches, start = [], 0
    for n in (700, 0, 4000):
        batches.append([obu.random_column(rng, DType.INT64, n, True, 5), obu.random_column(rng, DType.UTF8, n, True, 6), obu.random_column(rng, DType.FLOAT64, n, False, 5),
                        Column.from_numpy(np.arange(start, start + n, dtype=np.int64))])
        start += n
    # (a batch without NULLs may carry no bitmap: give every nullable column one so that the concatenation's columns do)
    for b in batches:
        for c in b[:2]:
            if c.validity is None:
                c.validity = obu.pack_bits(np.ones(c.length, dtype=bool))
    keys = [pp.PhysicalSortExpr(ColumnExpr.try_create("s", None), descending=True, nulls_first=False), pp.PhysicalSortExpr(ColumnExpr.try_create("k", None))]
    out = pp.PhysicalSortPlan.create(_mem(pp, ctx, fields, batches), keys).execute()
    assert len(out) == 1 and [f.name for f in out[0].fields] == ["k", "s", "f", "row"]
    whole = obu.concat_columns(batches)
    obu.assert_same_rows(out[0].table.to_host(), obu.order_by(whole, [(1, True, False), (0, False, True)]), what="three batches")  # ties: batch order, then row order


def test_expression_key_through_the_mirror(pp, ctx):
    n = 5000
    rng = np.random.default_rng(31)
    v = np.round(rng.uniform(0, 100, n), 0)
    fields = [Field("id", DType.INT64, False), Field("v", DType.FLOAT64, False), Field("name", DType.UTF8, True)]
    cols = [rownum(n), Column.from_numpy(v), obu.random_column(rng, DType.UTF8, n, True)]
    expr = PhysicalUnaryExpr.create(PhysicalBinaryExpr.create(ColumnExpr.try_create("v", None), Operator.Minus, PhysicalLiteralExpr.create(ScalarValue.Float64(50.0))),
                                    UnaryOperator.Abs, "abs", None)
    plan = pp.PhysicalSortPlan.create(_mem(pp, ctx, fields, [cols]), [pp.PhysicalSortExpr(expr, descending=True), pp.PhysicalSortExpr(ColumnExpr.try_create("name", None))])
    out = plan.execute()
    assert len(out) == 1 and out[0].num_columns == 3  # the temporary key column is dropped again
    with_key = cols + [Column.from_numpy(np.abs(v - 50.0))]
    obu.assert_same_rows(out[0].table.to_host(), obu.order_by(with_key, [(3, True, True), (2, False, True)])[:3], what="abs(v - 50.0) desc, name")


# ----------------------------------------------------------------------------- fetch
def test_fetch_through_the_c_abi_and_the_limit_plan_fused_and_unfused(pp, ctx):
    from naive_query_engine_amd.rewrite import plan_shape, rewrite

    n = 5000
    rng = np.random.default_rng(41)
    fields = [Field("k", DType.INT64, True), Field("s", DType.UTF8, True), Field("b", DType.BOOLEAN, False), Field("row", DType.INT64, False)]
    cols = [obu.random_column(rng, DType.INT64, n, True, 17), obu.random_column(rng, DType.UTF8, n, True), obu.random_column(rng, DType.BOOLEAN, n, False), rownum(n)]
    keys = [(0, True, False)]
    table = ctx.table_from_host(cols)
    scan = _mem(pp, ctx, fields, [cols])
    sort_exprs = [pp.PhysicalSortExpr(ColumnExpr.try_create("k", None), descending=True, nulls_first=False)]
    for fetch in (0, 1, n - 1, n, n + 5):
        exp = obu.order_by(cols, keys, fetch)
        assert exp[0].length == min(fetch, n)
        with Launches(ctx) as L:
            got = ctx.order_by(table, keys, fetch)
            takes = L.count("take")
            covered = L.count(f"ob_positions:{min(fetch, n)}")
            positions = L.count("ob_positions")
        obu.assert_same_rows(got.to_host(), exp, what=f"C ABI fetch {fetch}")
        if fetch == 0:
            assert positions == 0
        else:
            assert positions == 1 and covered == 1 and takes >= 4  # the takes' row list holds min(fetch, n) rows, not n
        tree = pp.PhysicalLimitPlan.create(pp.PhysicalSortPlan.create(scan, sort_exprs), fetch)
        unfused = tree.execute()
        fused_plan = rewrite(tree)
        assert plan_shape(fused_plan) == ["PhysicalSortPlan", "ScanPlan"] and fused_plan.fetch == fetch
        with Launches(ctx) as L:
            fused = fused_plan.execute()
            covered, positions = L.count(f"ob_positions:{min(fetch, n)}"), L.count("ob_positions")
        assert (positions, covered) == ((0, 0) if fetch == 0 else (1, 1))  # the fused form's takes cover `fetch` rows
        assert len(fused) == 1
        obu.assert_same_rows(fused[0].table.to_host(), exp, what=f"fused fetch {fetch}")
        if fetch == 0:
            assert unfused == []  # limit.rs:38 stops before the first batch
        else:
            assert len(unfused) == 1
            obu.assert_same_rows(unfused[0].table.to_host(), exp, what=f"unfused fetch {fetch}")


# ----------------------------------------------------------------------------- seeded sweep
def _sweep_seeds():
    return list(range(30)) + [1000 + i for i in range(int(os.environ.get("NQE_ORDER_BY_FUZZ_EXTRA_SEEDS", "0")))]


@pytest.mark.parametrize("seed", _sweep_seeds())
def test_seeded_sweep_against_the_model(ctx, seed):
    cols, keys = obu.random_table(seed)
    n = cols[0].length
    fetch = [None, None, 0, 3, n, n + 1][seed % 6]
    check(ctx, cols, keys, fetch, what=f"seed {seed} n={n}")


# ----------------------------------------------------------------------------- errors
def test_errors_launch_nothing(pp, ctx):
    cols = [Column.from_numpy(np.arange(10, dtype=np.int64)), obu.utf8_column([b"x"] * 10)]
    t = ctx.table_from_host(cols)
    with Launches(ctx) as L:
        with pytest.raises(ErrorCode) as e:
            ctx.order_by(t, [])
        assert e.value.status == Status.PlanError
        for bad in ([2], [-1], [0, (5, True)]):
            with pytest.raises(ErrorCode) as e:
                ctx.order_by(t, bad)
            assert e.value.status == Status.NotSupported and "order by: key column index out of range" in str(e.value)
        assert L.count("") == 0  # nothing was launched
    fields = [Field("a", DType.INT64, False), Field("s", DType.UTF8, False)]
    empty = pp.ScanPlan.create(pp.MemTable(fields, []), None)
    with pytest.raises(ErrorCode) as e:
        pp.PhysicalSortPlan.create(empty, [pp.PhysicalSortExpr(ColumnExpr.try_create("a", None))]).execute()
    assert e.value.status == Status.NotSupported
    with pytest.raises(ErrorCode) as e:
        pp.PhysicalSortPlan.create(_mem(pp, ctx, fields, [cols]), []).execute()
    assert e.value.status == Status.PlanError


# ----------------------------------------------------------------------------- golden queries
def test_golden_queries_through_the_mirrors(pp, ctx):
    from naive_query_engine_amd.rewrite import NaiveDB

    with open(os.path.join(GOLDEN, "order_by_expected.json")) as f:
        queries = json.load(f)["queries"]
    db = NaiveDB()
    db.create_csv_table("employee", os.path.join(GOLDEN, "employee.csv"))
    funcs = {"sum": pp.Sum, "max": pp.Max}
    for q in queries:
        plan = db.scan(q["table"])
        if "aggregates" in q:
            plan = pp.PhysicalAggregatePlan.create([ColumnExpr.try_create(q["group_by"], None)], [funcs[f].create(ColumnExpr.try_create(c, None)) for f, c in q["aggregates"]], plan)
            sort_exprs = [pp.PhysicalSortExpr(ColumnExpr.try_create(None, q["columns"].index(k["column"])), k["descending"], k["nulls_first"]) for k in q["keys"]]
        else:
            sort_exprs = [pp.PhysicalSortExpr(ColumnExpr.try_create(k["column"], None), k["descending"], k["nulls_first"]) for k in q["keys"]]
        plan = pp.PhysicalSortPlan.create(plan, sort_exprs)
        if q["fetch"] is not None:
            plan = pp.PhysicalLimitPlan.create(plan, q["fetch"])
        for out in (plan.execute(), db.run_plan(plan)):
            assert len(out) == 1 and [f.name for f in out[0].fields] == q["columns"], q["name"]
            host = out[0].table.to_host()
            rows = [list(r) for r in zip(*[c.to_list() for c in host])]
            assert rows == q["rows"], q["name"]
