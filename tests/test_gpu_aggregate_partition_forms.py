"""The partitioned aggregate's exact form (count -> scan -> scatter -> one workgroup per partition) and its two-level form with
one AND two value columns, every predicate variant and both inline key kinds of the count / scatter kernels, against the CPU
oracle; each case also reads the timing report for the kernel it is about.  (The other suites reach these two forms with one
value column only.)"""
import numpy as np
import pytest

from naive_query_engine_amd import AggregateFunc, Column, Operator
from naive_query_engine_amd.expression import binop, col, lit_i64
from oracle import oracle as orc
from tests.helpers import assert_rows_multiset_equal, fields

pytestmark = pytest.mark.gpu

RTOL = 1e-9
ALL_AGGS = lambda c: [(AggregateFunc.Count, c), (AggregateFunc.Sum, c), (AggregateFunc.Avg, c), (AggregateFunc.Min, c), (AggregateFunc.Max, c)]
F3 = fields("k", "v", "w")


@pytest.fixture(scope="module")
def ctx():
    from naive_query_engine_amd import capi

    c = capi.Context(0)
    yield c
    c.close()


def _timed_aggregate(ctx, t, aggs, key, pred):
    ctx.timing_enable(True)
    ctx.timing_reset()
    try:
        got = ctx.aggregate(t, aggs, group_nodes=key, pred_nodes=pred).to_host()
    finally:
        ctx.timing_enable(False)
    return got, set(ctx.timing_report())


# ---- (a) the exact form: 300 000 rows (the partitioned path starts at 2^18) over about 45 000 groups
ROWS, GROUPS = 300_000, 45_000


@pytest.fixture(scope="module")
def exact_inputs(ctx):
    rng = np.random.default_rng(45)
    # `col`: 45 000 keys on both sides of zero; `col % m`: a wide column whose remainders by 45 000 are (-m, m) — about the same count
    k = rng.integers(-GROUPS // 2, GROUPS // 2, ROWS).astype(np.int64)
    v = rng.random(ROWS) * 200 - 100
    w = rng.integers(-1000, 1000, ROWS).astype(np.int64)
    wide = rng.integers(0, 1 << 40, ROWS).astype(np.int64)
    cols = {"col": [Column.from_numpy(k), Column.from_numpy(v), Column.from_numpy(w)],
            "col_mod": [Column.from_numpy(wide), Column.from_numpy(v), Column.from_numpy(w)]}
    return {name: (c, ctx.table_from_host(c)) for name, c in cols.items()}


@pytest.mark.parametrize("key_kind", ["col", "col_mod"])
@pytest.mark.parametrize("pred_kind", ["none", "key_range", "other_column", "chain"])
@pytest.mark.parametrize("nv", [1, 2])
def test_aggregate_exact_form(ctx, exact_inputs, monkeypatch, nv, pred_kind, key_kind):
    """the slab allocation "fails" (NQE_TEST_SLAB_OOM, read per call), so the query takes agg_partition_count -> scan ->
    agg_partition_scatter -> agg_segments; one and two value columns (Float64 and Int64 values)"""
    monkeypatch.setenv("NQE_TEST_SLAB_OOM", "1")
    cols, t = exact_inputs[key_kind]
    key = (col(0) if key_kind == "col" else binop(col(0), Operator.Modulos, lit_i64(GROUPS))).flatten(F3)
    lo = -GROUPS // 4 if key_kind == "col" else 1 << 38
    pred = {"none": None, "key_range": binop(col(0), Operator.GtEq, lit_i64(lo)), "other_column": binop(col(2), Operator.Lt, lit_i64(500)),
            "chain": binop(binop(col(2), Operator.Modulos, lit_i64(7)), Operator.NotEq, lit_i64(3))}[pred_kind]
    pn = pred.flatten(F3) if pred is not None else None
    aggs = ALL_AGGS(1) + (ALL_AGGS(2) if nv == 2 else [])
    exp = orc.aggregate([cols], aggs, group_nodes=key, pred_nodes=pn)[0]
    for rep in range(2):  # the second execution starts from the plan hint (exact form)
        got, names = _timed_aggregate(ctx, t, aggs, key, pn)
        assert_rows_multiset_equal(got, exp, RTOL, exact_cols=[0, 5][:nv], what=f"exact form, {nv} value columns, predicate {pred_kind}, key {key_kind}, run {rep}")
        assert "agg_partition_count" in names, names


# ---- (b) the two-level form
TWO_LEVEL_KEYS = 960_000


def test_aggregate_two_level_form_two_value_columns(ctx):
    """two value columns: a workgroup table of 2048 slots, 512 partitions — once a partition holds more distinct keys than its table
    takes, every partition is split into 64 sub-partitions (agg_subpartition).  Every key occurs once, so rows == keys.  Measured
    with these keys on the library before the kernels were rebuilt from shared pieces, in steps of 20 000: 940 000 keys still fit
    the 512 tables (agg_partition_scatter 1, agg_segments 1), from 960 000 on the query runs agg_partition_count 1,
    agg_partition_scatter 2, agg_subpartition 1, agg_segments 2."""
    rng = np.random.default_rng(2)
    n = TWO_LEVEL_KEYS
    k = (rng.permutation(n).astype(np.int64) - n // 2) * 3
    v = rng.random(n) * 200 - 100
    w = rng.integers(-1000, 1000, n).astype(np.int64)
    cols = [Column.from_numpy(k), Column.from_numpy(v), Column.from_numpy(w)]
    t = ctx.table_from_host(cols)
    key = col(0).flatten(F3)
    aggs = ALL_AGGS(1) + ALL_AGGS(2)
    exp = orc.aggregate([cols], aggs, group_nodes=key)[0]
    got, names = _timed_aggregate(ctx, t, aggs, key, None)
    assert_rows_multiset_equal(got, exp, RTOL, exact_cols=[0, 5], what="two-level form, two value columns")
    assert "agg_subpartition" in names, names
