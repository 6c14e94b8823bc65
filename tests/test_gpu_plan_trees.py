"""Differential tests of multi-batch plan trees: the mirror operators (physical_plan.py) and the rewrite pass (rewrite.py) against
the oracle's operators chained through raw handles, on tables of 2-5 batches whose lengths sit on the edges of the bitmap word,
the 256-thread block and the 4096-row tile.  What exists only because a table has several batches is what is under test here: the
predicate of batch 0 zipped against every batch (Q3) and the fused operators' fall-back to it, nqe_table_concat behind the grouped
aggregate and the join build, nqe_table_slice behind Limit / Offset, the un-grouped state kept between executes (Q9), the join
re-execution (Q11).  Unless a test says otherwise a result is a list of batches that must match the oracle's in number, in lengths
and, with no tolerance, in values, validity and strings.  Seeds are fixed: a failure names its case."""
import os

import numpy as np
import pytest

from naive_query_engine_amd import AggregateFunc as A, Column, DType, ErrorCode, Field, Operator
from naive_query_engine_amd.expression import binop, col, lit_f64, lit_i64
from oracle import oracle as orc
from tests.helpers import assert_batches_equal
from tests.plan_tree_util import (assert_aggregate_equal, assert_same_batches, batch_lengths, make_batch, make_batches, mem_table, np_take, random_tree, schema,
                                  to_oracle, to_plan, FUZZ_FIELDS)

pytestmark = pytest.mark.gpu
EXTRA = int(os.environ.get("NQE_PLAN_FUZZ_EXTRA_SEEDS", "0"))  # a longer hunt: NQE_PLAN_FUZZ_EXTRA_SEEDS=200 pytest tests/test_gpu_plan_trees.py
BASE = int(os.environ.get("NQE_PLAN_FUZZ_SEED_BASE", "0"))      # ... and NQE_PLAN_FUZZ_SEED_BASE=100000 for fresh cases
FLD = schema()
# batch 0 longer than / equal to / shorter than the others / in between; a batch without nulls (no bitmap on the device) between
# nullable ones, a zero-row batch
LENGTH_SETS = {"longer": [20000, 4097, 0, 8193, 63], "equal": [4096, 4096, 4096], "shorter": [1000, 4095, 257, 20000, 65], "mixed": [64, 127, 255, 1, 8193]}
NULLS = [0.2, 0.0, 0.3, 0.0, 0.5]


@pytest.fixture(scope="module")
def ctx():
    from naive_query_engine_amd import capi

    c = capi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def pp():
    from naive_query_engine_amd import physical_plan

    return physical_plan


@pytest.fixture(scope="module")
def tables(ctx, pp):
    """name -> (host batches, MemTable), built once and never modified"""
    out = {}
    for i, (name, lengths) in enumerate(LENGTH_SETS.items()):
        host = make_batches(100 + i, lengths, NULLS[: len(lengths)], nan_frac=0.02)
        out[name] = (host, mem_table(pp, FLD, host, ctx))
    return out


def host_of(batches):
    return [b.table.to_host() for b in batches]


def db_with(table):
    from naive_query_engine_amd.rewrite import NaiveDB

    db = NaiveDB()
    db.catalog.tables["t"] = table  # registered as built: on this module's context
    return db


PREDICATES = {
    "int64": binop(col("k"), Operator.Lt, lit_i64(10)),                                      # NULL where k is NULL (Q4)
    "float64_nan": binop(col("v"), Operator.Gt, lit_f64(120.0)),                             # NaN rows compare false
    "boolean": col("b"),
    "tree": binop(binop(binop(col("id"), Operator.Modulos, lit_i64(3)), Operator.Eq, lit_i64(1)), Operator.Or,
                  binop(col("b"), Operator.And, binop(col(2), Operator.LtEq, lit_f64(60.0)))),
}


# ----------------------------------------------------------------------------- 1. Selection over several batches (Q3 / Q4)
@pytest.mark.parametrize("pred", list(PREDICATES))
@pytest.mark.parametrize("shape", list(LENGTH_SETS))
def test_selection_over_several_batches(pp, tables, shape, pred):
    host, table = tables[shape]
    expr = PREDICATES[pred]
    exp = orc.selection(host, expr.flatten(FLD))
    assert len(exp) == len(host)
    plain = pp.SelectionPlan.create(pp.ScanPlan.create(table, None), expr).execute()
    assert_same_batches(host_of(plain), exp, f"{shape} / {pred} [plain]")
    db = db_with(table)
    assert_same_batches(host_of(db.run_plan(pp.SelectionPlan.create(db.scan("t"), expr))), exp, f"{shape} / {pred} [run_plan]")


# ----------------------------------------------------------------------------- 2. Projection over Selection: fused and fall-back
@pytest.mark.parametrize("shape", ["single", "two", "longer", "shorter", "mixed"])
def test_projection_over_selection_fused_and_fallback(ctx, pp, tables, shape):
    from naive_query_engine_amd.rewrite import plan_shape, rewrite

    if shape in ("single", "two"):
        host = make_batches(7, [20000] if shape == "single" else [4097, 1000], [0.2, 0.0], nan_frac=0.02)
        table = mem_table(pp, FLD, host, ctx)
    else:
        host, table = tables[shape]
    pred = PREDICATES["tree"] if shape != "shorter" else PREDICATES["int64"]
    exprs = [col("s"), col("b"), binop(col("v"), Operator.Multiply, lit_f64(2.0)), binop(binop(col("id"), Operator.Plus, lit_i64(1)), Operator.Modulos, lit_i64(7)), col(3)]
    out_schema = [Field("s", DType.UTF8, True), Field("b", DType.BOOLEAN, True), Field("v2", DType.FLOAT64, True), Field("m", DType.INT64, True), Field("u", DType.UINT64, True)]
    exp = orc.projection(orc.selection(host, pred.flatten(FLD), raw=True), [e.flatten(FLD) for e in exprs])
    tree = pp.ProjectionPlan.create(pp.SelectionPlan.create(pp.ScanPlan.create(table, None), pred), out_schema, exprs)
    fused = rewrite(tree)
    assert plan_shape(fused) == ["FusedSelectionProjectionPlan", "ScanPlan"]
    plain, rewritten = host_of(tree.execute()), host_of(fused.execute())
    assert_same_batches(plain, exp, f"{shape} [plain]")
    assert_same_batches(rewritten, exp, f"{shape} [rewritten]")
    assert_same_batches(rewritten, plain, f"{shape} [rewritten vs plain]")


# ----------------------------------------------------------------------------- 3. Limit over Offset, swept over boundaries
@pytest.fixture(scope="module")
def selected(ctx, pp):
    """a multi-batch selection output: irregular batch lengths, produced once on the device and once by the oracle"""
    host = make_batches(31, [4097, 257, 1000, 65, 0, 300], [0.2, 0.0, 0.3, 0.0, 0.0, 0.5])
    pred = PREDICATES["boolean"]
    dev = pp.SelectionPlan.create(pp.ScanPlan.create(mem_table(pp, FLD, host, ctx), None), pred).execute()
    handle = orc.selection(host, pred.flatten(FLD), raw=True)
    lengths = batch_lengths(handle)
    assert [b.num_rows for b in dev] == lengths and lengths[0] + 65 < sum(lengths) and len(set(lengths)) > 2
    return pp.MemTable.from_device(FLD, [b.table for b in dev]), handle, lengths


def boundary_values(lengths):
    first, total = lengths[0], sum(lengths)
    return [0, 1, first - 1, first, first + 1, first + 63, first + 64, first + 65, total - 1, total, total + 5]


@pytest.mark.parametrize("which", range(11))
def test_limit_over_offset_swept_over_boundaries(pp, selected, which):
    table, handle, lengths = selected
    off = boundary_values(lengths)[which]
    below = orc.offset(handle, off, raw=True)
    for n in boundary_values(lengths):
        got = pp.PhysicalLimitPlan.create(pp.PhysicalOffsetPlan.create(pp.ScanPlan.create(table, None), off), n).execute()
        assert_same_batches(host_of(got), orc.limit(below, n), f"limit {n} over offset {off} of {lengths}")


# ----------------------------------------------------------------------------- 4. grouped aggregate over several batches
def agg_ops(pp):
    funcs = [(A.Count, "v"), (A.Min, "v"), (A.Max, "v"), (A.Sum, "v"), (A.Avg, "v"), (A.Count, "s"), (A.Count, "b")]
    cls = {A.Count: pp.Count, A.Min: pp.Min, A.Max: pp.Max, A.Sum: pp.Sum, A.Avg: pp.Avg}
    return [cls[f].create(col(c)) for f, c in funcs], [(f, [x.name for x in FLD].index(c)) for f, c in funcs], [f for f, _ in funcs]


GROUP_KEYS = {"k": col("k"), "id%3": binop(col("id"), Operator.Modulos, lit_i64(3)), "id%1000": binop(col("id"), Operator.Modulos, lit_i64(1000)),
              "id%5000": binop(col("id"), Operator.Modulos, lit_i64(5000))}


@pytest.fixture(scope="module")
def agg_table(ctx, pp):
    host = make_batches(41, [1000, 4095, 257, 20000, 0, 65], [0.3, 0.0, 0.05, 0.2, 0.0, 0.5])  # no NaN: min / max compare with ==
    return host, mem_table(pp, FLD, host, ctx)


@pytest.mark.parametrize("above_selection", [False, True], ids=["alone", "above_selection"])
@pytest.mark.parametrize("key", list(GROUP_KEYS))
def test_grouped_aggregate_over_several_batches(pp, agg_table, key, above_selection):
    from naive_query_engine_amd.rewrite import plan_shape, rewrite

    host, table = agg_table
    ops, aggs, funcs = agg_ops(pp)
    pred = PREDICATES["tree"] if above_selection else None
    exp = orc.aggregate(host, aggs, group_nodes=GROUP_KEYS[key].flatten(FLD), pred_nodes=pred.flatten(FLD) if pred is not None else None)
    assert len(exp) == 1 and exp[0][0].length >= 3
    below = pp.ScanPlan.create(table, None)
    tree = pp.PhysicalAggregatePlan.create([GROUP_KEYS[key]], ops, pp.SelectionPlan.create(below, pred) if above_selection else below)
    plans = {"plain": tree, "rewritten": rewrite(tree)}
    if above_selection:
        assert plan_shape(plans["rewritten"]) == ["FusedSelectionAggregatePlan", "ScanPlan"]
    for name, plan in plans.items():
        got = plan.execute()
        assert len(got) == 1
        assert_aggregate_equal(got[0].table.to_host(), exp[0], funcs, f"group by {key} [{name}]")


# ----------------------------------------------------------------------------- 5. un-grouped aggregate, executed again (Q9)
@pytest.mark.parametrize("with_nan", [False, True], ids=["finite", "nan_in_one_batch"])
@pytest.mark.parametrize("mode", ["plain", "plain_above_selection", "rewritten_above_selection"])
def test_ungrouped_aggregate_reexecuted(ctx, pp, mode, with_nan):
    from naive_query_engine_amd.rewrite import plan_shape, rewrite

    rng = np.random.default_rng(51)
    host = [make_batch(rng, 4097, 0.2), make_batch(rng, 1000, 0.1, v_all_null=True), make_batch(rng, 0), make_batch(rng, 8193, 0.0, nan_frac=0.01 if with_nan else 0.0),
            make_batch(rng, 63, 0.5)]
    assert host[1][2].null_count == 1000 and bool(np.isnan(host[3][2].to_numpy()).any()) == with_nan
    table = mem_table(pp, FLD, host, ctx)
    ops, aggs, funcs = agg_ops(pp)
    pred = None if mode == "plain" else PREDICATES["int64"]
    below = pp.ScanPlan.create(table, None)
    plan = pp.PhysicalAggregatePlan.create([], ops, below if pred is None else pp.SelectionPlan.create(below, pred))
    if mode == "rewritten_above_selection":
        plan = rewrite(plan)
        assert plan_shape(plan) == ["FusedSelectionAggregatePlan", "ScanPlan"]
    for k in (1, 2, 3):  # the same plan object: its state is never cleared
        exp = orc.aggregate(host, aggs, pred_nodes=pred.flatten(FLD) if pred is not None else None, executions=k)
        got = plan.execute()
        assert len(got) == len(exp) == 1 and got[0].num_rows == 1
        assert int(exp[0][0].to_numpy()[0]) > 0
        assert_aggregate_equal(got[0].table.to_host(), exp[0], funcs, f"{mode} execute() #{k}")


# ----------------------------------------------------------------------------- 6. HashJoin over several batches, executed again (Q11)
def join_host(unique):
    rng = np.random.default_rng(61 + int(unique))
    # unique: disjoint id ranges per build batch; otherwise every batch holds 0..n-1, so a key has up to three build rows
    left = [make_batch(rng, n, nf, nan_frac=0.02, id_base=base if unique else None, id_nulls=False) for n, nf, base in [(1000, 0.2, 0), (65, 0.0, 5000), (4097, 0.3, 10000)]]
    right = [make_batch(rng, n, nf, nan_frac=0.02, id_base=base, id_nulls=False) for n, nf, base in [(4097, 0.3, 0), (63, 0.0, 970), (1000, 0.1, 3500)]]
    return left, right


def join_tables(ctx, pp, unique):
    left, right = join_host(unique)
    lf, rf = schema(), schema("r_")
    return left, right, lf, rf, mem_table(pp, lf, left, ctx), mem_table(pp, rf, right, ctx)


@pytest.mark.parametrize("unique", [True, False], ids=["unique_keys", "duplicate_keys"])
def test_hash_join_over_several_batches_reexecuted(ctx, pp, unique):
    left, right, lf, rf, lt, rt = join_tables(ctx, pp, unique)
    join = pp.HashJoin.create(pp.ScanPlan.create(lt, None), pp.ScanPlan.create(rt, None), [(pp.ColumnRef(None, "id"), pp.ColumnRef(None, "r_id"))], pp.JoinType.Inner, lf + rf)
    once = sum(batch_lengths(orc.hash_join(left, right, 0, 0, raw=True)))
    assert once > 1000
    for k in (1, 2, 3):
        exp = orc.hash_join(left, right, 0, 0, executions=k)
        assert len(exp) == 3 and sum(b[0].length for b in exp) == k * once
        assert_same_batches(host_of(join.execute()), exp, f"unique={unique} execute() #{k}")


@pytest.mark.parametrize("unique", [True, False], ids=["unique_keys", "duplicate_keys"])
def test_hash_join_above_selection_below_limit(ctx, pp, unique):
    """both inputs are multi-batch selections (Q3); their NULL predicate rows (Q4) arrive as NULL keys, which the reference joins by
    the value under the NULL"""
    from naive_query_engine_amd.rewrite import rewrite

    left, right, lf, rf, lt, rt = join_tables(ctx, pp, unique)
    lpred = binop(col("k"), Operator.Lt, lit_i64(20))
    rpred = binop(binop(col("r_id"), Operator.Modulos, lit_i64(5)), Operator.NotEq, lit_i64(0))
    hl, hr = orc.selection(left, lpred.flatten(lf), raw=True), orc.selection(right, rpred.flatten(rf), raw=True)
    joined = orc.hash_join(hl, hr, 0, 0, raw=True)
    lengths = batch_lengths(joined)
    assert len(lengths) == 3 and lengths[0] > 65 and lengths[1] > 0
    mk = lambda n: pp.PhysicalLimitPlan.create(
        pp.HashJoin.create(pp.SelectionPlan.create(pp.ScanPlan.create(lt, None), lpred), pp.SelectionPlan.create(pp.ScanPlan.create(rt, None), rpred),
                           [(pp.ColumnRef(None, "id"), pp.ColumnRef(None, "r_id"))], pp.JoinType.Inner, lf + rf), n)
    for n in (lengths[0] - 1, lengths[0] + 65, sum(lengths) + 1):
        exp = orc.limit(joined, n)
        assert_same_batches(host_of(mk(n).execute()), exp, f"unique={unique} limit {n} [plain]")
        assert_same_batches(host_of(rewrite(mk(n)).execute()), exp, f"unique={unique} limit {n} [rewritten]")


# ----------------------------------------------------------------------------- 7. seeded random trees
@pytest.mark.parametrize("seed", range(16 + EXTRA))
def test_random_plan_trees(ctx, pp, seed):
    from naive_query_engine_amd.rewrite import rewrite

    host, tree, _ = random_tree(BASE + seed)
    what = f"seed {BASE + seed}: batches a={[b[0].length for b in host['a']]} b={[b[0].length for b in host['b']]} tree={tree!r}"
    tables = {name: mem_table(pp, FUZZ_FIELDS[name], batches, ctx) for name, batches in host.items()}
    try:
        exp = to_oracle(tree, host).to_python()
    except ErrorCode as e:
        for name, plan in (("plain", to_plan(tree, pp, tables)), ("rewritten", rewrite(to_plan(tree, pp, tables)))):
            with pytest.raises(ErrorCode) as g:
                plan.execute()
            assert g.value.status == e.status, f"{what} [{name}]"
        return
    plain = host_of(to_plan(tree, pp, tables).execute())
    rewritten = host_of(rewrite(to_plan(tree, pp, tables)).execute())
    if tree.op == "agg":
        funcs = [f for f, _ in tree.kw["aggs"]]
        assert len(plain) == len(rewritten) == len(exp) == 1, what
        assert_aggregate_equal(plain[0], exp[0], funcs, what + " [plain]")
        assert_aggregate_equal(rewritten[0], exp[0], funcs, what + " [rewritten]")
        assert_aggregate_equal(rewritten[0], plain[0], funcs, what + " [rewritten vs plain]")
    else:
        assert_same_batches(plain, exp, what + " [plain]")
        assert_same_batches(rewritten, exp, what + " [rewritten]")
        assert_same_batches(rewritten, plain, what + " [rewritten vs plain]")


# ----------------------------------------------------------------------------- 8. the table utilities at size, against numpy
def check_table_and_one_operator_more(ctx, got, exp, what):
    """the table itself, then a selection on its Boolean column and a count of every column over it: bits left beyond `length` in
    a last bitmap word, or a wrong null_count, would show there"""
    assert got.num_rows == exp[0].length, what
    assert_batches_equal(got.to_host(), exp, what=what)
    b = exp[4]
    bv, bm = b.to_numpy(), b.valid_mask()
    rows = np.nonzero(~bm | bv)[0]  # kept, or NULL predicate -> NULL row (Q4)
    assert_batches_equal(ctx.selection(got, col(4).flatten(FLD)).to_host(), [np_take(c, rows, bm[rows]) for c in exp], what=what + " [selection on b]")
    counts = ctx.aggregate(got, [(A.Count, i) for i in range(6)]).to_host()
    assert [int(c.to_numpy()[0]) for c in counts] == [int(c.valid_mask().sum()) for c in exp], what + " [count of every column]"


@pytest.fixture(scope="module")
def big(ctx):
    cols = make_batch(np.random.default_rng(81), 70001, 0.2, nan_frac=0.01)
    return cols, ctx.table_from_host(cols)


@pytest.mark.parametrize("offset", [1, 63, 64, 65, 4097, 33333])
def test_slice_at_size(ctx, big, offset):
    cols, table = big
    w = 4096 + (-offset) % 64  # offset + w is a multiple of 64: the slice ends on a word boundary of the source
    for length in sorted({w - 1, w, w + 1, 639, 640, 641, 70001 - offset}):  # ... one short, one past; the same for the output's own last word; to the end
        exp = [np_take(c, np.arange(offset, offset + length)) for c in cols]
        check_table_and_one_operator_more(ctx, ctx.slice(table, offset, length), exp, f"slice({offset}, {length})")


def test_concat_at_size(ctx):
    rng = np.random.default_rng(82)
    parts = [make_batch(rng, n, nf, nan_frac=0.01) for n, nf in [(4097, 0.2), (63, 0.3), (0, 0.0), (20000, 0.0), (1, 0.5), (64, 0.1), (8191, 0.4)]]
    assert all(c.validity is None for c in parts[3])
    got = ctx.concat([ctx.table_from_host(p) for p in parts])
    exp = []
    for ci in range(6):
        if parts[0][ci].dtype == DType.UTF8:
            exp.append(Column.from_list([x for p in parts for x in p[ci].to_list()], DType.UTF8))
        else:
            exp.append(Column.from_numpy(np.concatenate([p[ci].to_numpy() for p in parts]), np.concatenate([p[ci].valid_mask() for p in parts])))
    check_table_and_one_operator_more(ctx, got, exp, "concat of 4097 + 63 + 0 + 20000 (no nulls) + 1 + 64 + 8191 rows")
    # a part without a bitmap first and last, and parts that are all of one kind
    for order in ([3, 0, 3], [3, 3], [1, 5, 4, 2]):
        got = ctx.concat([ctx.table_from_host(parts[i]) for i in order])
        exp = []
        for ci in range(6):
            if parts[0][ci].dtype == DType.UTF8:
                exp.append(Column.from_list([x for i in order for x in parts[i][ci].to_list()], DType.UTF8))
            else:
                exp.append(Column.from_numpy(np.concatenate([parts[i][ci].to_numpy() for i in order]), np.concatenate([parts[i][ci].valid_mask() for i in order])))
        check_table_and_one_operator_more(ctx, got, exp, f"concat of parts {order}")


def test_take_at_size(ctx, big):
    cols, table = big
    idx = np.random.default_rng(83).integers(0, 70001, 70001).astype(np.int64)
    got = ctx.take(table, ctx.table_from_host([Column.from_numpy(idx)]))
    check_table_and_one_operator_more(ctx, got, [np_take(c, idx) for c in cols], "take of 70001 random rows")
