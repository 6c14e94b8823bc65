"""GROUP BY on several keys (quirk Q20) on the host: the C ABI's declaration and its binding, the plan mirrors and their rewrite arm, the
model the GPU tests compare against (tests/group_keys_util.py) checked by hand and against the oracle's single-key aggregate, and the
committed golden.  Nothing here needs a GPU."""
import ctypes as C
import inspect
import json
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import group_keys_util as gku  # noqa: E402
from naive_query_engine_amd import AggregateFunc, Column, ColumnExpr, DType, ErrorCode, Field, Operator, PhysicalBinaryExpr, PhysicalLiteralExpr, ScalarValue, Status, read_csv  # noqa: E402
from naive_query_engine_amd import physical_plan as pp  # noqa: E402
from naive_query_engine_amd.arrow_host import node_column  # noqa: E402
from naive_query_engine_amd.rewrite import plan_shape, rewrite  # noqa: E402
from tools import check_rust_shim as crs  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
DATA = [Field("id", DType.INT64), Field("name", DType.UTF8), Field("age", DType.INT64), Field("score", DType.FLOAT64)]


class _Stub:
    def __init__(self, schema):
        self._schema = schema

    def schema(self):
        return self._schema

    def scan(self, projection):
        raise AssertionError("a stub source is never scanned here")


def _keys():
    return [PhysicalBinaryExpr.create(ColumnExpr.try_create("id", None), Operator.Modulos, PhysicalLiteralExpr.create(ScalarValue.Int64(3))), ColumnExpr.try_create("age", None)]


def _ops():
    return [pp.Count.create(ColumnExpr.try_create("score", None)), pp.Sum.create(ColumnExpr.try_create("score", None))]


# ----------------------------------------------------------------------------- the C ABI
def test_header_declares_the_entry_point_and_q20():
    hdr = open(os.path.join(ROOT, "include", "nqe.h")).read()
    assert re.search(r"nqe_status\s+nqe_group_aggregate_execute\s*\(\s*nqe_ctx\s*\*\s*ctx\s*,\s*const nqe_table\s*\*\s*in\s*,\s*const nqe_expr_node\s*\*\s*pred\s*,\s*int32_t\s+pred_nodes\s*,\s*"
                     r"const nqe_expr_node\s*\*\s*group_nodes\s*,\s*const int32_t\s*\*\s*group_offsets\s*,\s*int32_t\s+num_keys\s*,\s*const nqe_aggregate\s*\*\s*aggs\s*,\s*"
                     r"int32_t\s+num_aggs\s*,\s*nqe_table\s*\*\*\s*out\s*\)\s*;", hdr)
    assert "#define NQE_MAX_GROUP_KEYS 8" in hdr and "#define NQE_ABI_VERSION 1" in hdr
    assert "quirk Q20" in hdr
    for doc in ("SURVEY.md", "DESIGN.md"):
        assert re.search(r"\bQ20\b", open(os.path.join(ROOT, doc)).read()), doc


def test_binding_matches_the_header():
    from naive_query_engine_amd import capi

    assert "nqe_group_aggregate_execute" in capi.SYMBOLS and capi.MAX_GROUP_KEYS == 8
    fn = capi.lib().nqe_group_aggregate_execute
    assert fn.restype is C.c_int32 and len(fn.argtypes) == 10 and fn.argtypes[3] is C.c_int32 and fn.argtypes[6] is C.c_int32 and fn.argtypes[8] is C.c_int32
    assert list(inspect.signature(capi.Context.group_aggregate).parameters) == ["self", "table", "keys", "aggs", "pred_nodes"]
    assert inspect.signature(capi.Context.group_aggregate).parameters["pred_nodes"].default is None


# ----------------------------------------------------------------------------- the Python mirror
def test_grouped_plan_schema_children_and_the_empty_key_list():
    scan = pp.ScanPlan.create(_Stub(DATA))
    plan = pp.GroupedAggregatePlan.create(_keys(), _ops(), scan)
    assert plan.children() == [scan]
    # group fields, then aggregate fields (Q13's logical order); a bare column keeps its name, an expression is group_<i>
    assert [(f.name, f.dtype) for f in plan.schema()] == [("group_0", DType.INT64), ("age", DType.INT64), ("count(score)", DType.UINT64), ("sum(score)", DType.FLOAT64)]
    by_name = pp.GroupedAggregatePlan.create([ColumnExpr.try_create("name", None), ColumnExpr.try_create(None, 0)], _ops(), scan)
    assert [(f.name, f.dtype) for f in by_name.schema()][:2] == [("name", DType.UTF8), ("id", DType.INT64)]
    with pytest.raises(ErrorCode) as e:
        pp.GroupedAggregatePlan.create([], _ops(), scan)
    assert e.value.status == Status.PlanError
    # the reference's operator is as it was: the INPUT schema, every group expression kept, only the first one read (Q8)
    old = pp.PhysicalAggregatePlan.create(_keys(), _ops(), scan)
    assert old.schema() == DATA and len(old.group_expr) == 2


def test_rewrite_fuses_a_selection_below_a_grouped_plan_and_leaves_the_old_operator_alone():
    from naive_query_engine_amd.rewrite import FusedSelectionAggregatePlan, FusedSelectionGroupedAggregatePlan

    pred = PhysicalBinaryExpr.create(ColumnExpr.try_create("age", None), Operator.Gt, PhysicalLiteralExpr.create(ScalarValue.Int64(19)))
    scan = pp.ScanPlan.create(_Stub(DATA))
    keys, ops = _keys(), _ops()
    tree = pp.GroupedAggregatePlan.create(keys, ops, pp.SelectionPlan.create(scan, pred))
    assert plan_shape(tree) == ["GroupedAggregatePlan", "SelectionPlan", "ScanPlan"]
    out = rewrite(tree)
    assert plan_shape(out) == ["FusedSelectionGroupedAggregatePlan", "ScanPlan"]
    assert isinstance(out, FusedSelectionGroupedAggregatePlan) and out.predicate is pred and out.group_expr == keys and out.aggr_ops == ops and out is not tree
    assert plan_shape(tree) == ["GroupedAggregatePlan", "SelectionPlan", "ScanPlan"]  # the input tree is left as it was
    assert plan_shape(out.unfused(scan)) == plan_shape(tree) and out.schema() == tree.schema()
    assert rewrite(out) is out
    # no selection below: the operator stays, its child is rewritten
    proj = pp.ProjectionPlan.create(pp.SelectionPlan.create(scan, pred), DATA, [ColumnExpr.try_create(f.name, None) for f in DATA])
    assert plan_shape(rewrite(pp.GroupedAggregatePlan.create(keys, ops, proj))) == ["GroupedAggregatePlan", "FusedSelectionProjectionPlan", "ScanPlan"]
    # PhysicalAggregatePlan is unchanged by all this: its own fusion, its own class, never the grouped one
    old = rewrite(pp.PhysicalAggregatePlan.create(keys, ops, pp.SelectionPlan.create(scan, pred)))
    assert type(old) is FusedSelectionAggregatePlan and not isinstance(old, pp.GroupedAggregatePlan) and old.schema() == DATA
    assert plan_shape(rewrite(pp.PhysicalAggregatePlan.create(keys, ops, scan))) == ["PhysicalAggregatePlan", "ScanPlan"]
    # a grouped plan below other operators is reached by the pass
    lim = rewrite(pp.PhysicalLimitPlan.create(tree, 3))
    assert plan_shape(lim) == ["PhysicalLimitPlan", "FusedSelectionGroupedAggregatePlan", "ScanPlan"]


# ----------------------------------------------------------------------------- the other mirrors
def test_cpp_mirror_has_the_grouped_plan_and_the_rewrite_arm():
    hpp = open(os.path.join(ROOT, "naive_query_engine_amd", "host", "naive_db.hpp")).read()
    assert "struct GroupedAggregatePlan : PhysicalPlan" in hpp and "struct FusedSelectionGroupedAggregatePlan : GroupedAggregatePlan" in hpp
    assert "nqe_group_aggregate_execute(" in hpp
    arm = hpp[hpp.index("inline PhysicalPlanRef rewrite("):]
    assert "std::dynamic_pointer_cast<GroupedAggregatePlan>(plan)" in arm[:600]
    # the reference's operator still reads group_expr[0] alone
    assert "group_expr[0]->flatten(batches[0].schema(), key); // only group_expr[0] (Q8)" in hpp


def test_rust_shim_declares_the_entry_point_and_a_grouped_plan():
    path = os.path.join(ROOT, "integration", "rust", "gpu.rs")
    src = crs.strip_rust(open(path).read())
    assert "nqe_group_aggregate_execute" in crs.extern_functions(src)
    assert "pub struct GpuGroupedAggregatePlan" in src and "impl GpuExec for GpuGroupedAggregatePlan" in src and "impl PhysicalPlan for GpuGroupedAggregatePlan" in src
    assert crs.check(path)[0] == []


# ----------------------------------------------------------------------------- the model
def test_model_by_hand():
    a = Column.from_list([1, 2, 1, None, 2, 1], DType.INT64)
    s = gku.utf8_column([b"x", b"", b"x", b"x", b"", b"y"], [True, True, True, True, False, True])
    v = Column.from_list([1.0, 2.0, None, 8.0, 16.0, 32.0], DType.FLOAT64)
    aggs = [(AggregateFunc.Count, 2), (AggregateFunc.Sum, 2), (AggregateFunc.Avg, 2), (AggregateFunc.Min, 2), (AggregateFunc.Max, 2)]
    tuples, out, dense = gku.model([gku.key_values(a), gku.key_values(s)], [a, s, v], aggs)
    assert tuples == [(1, b"x"), (1, b"y"), (2, b"")]  # rows 3 and 4 have a NULL key; the empty string is a key of its own
    assert dense.tolist() == [0, 2, 0, -1, -1, 1]
    assert out[0].tolist() == [1, 1, 1] and out[1].tolist() == [1.0, 32.0, 2.0] and out[3].tolist() == [1.0, 32.0, 2.0]
    tuples, out, _ = gku.model([gku.key_values(a), gku.key_values(s)], [a, s, v], aggs, keep=np.array([0, 1, 1, 1, 1, 0], dtype=bool))
    assert tuples == [(1, b"x"), (2, b"")]  # (1, "y") lost its only row
    assert out[0].tolist() == [0, 1] and out[1][0] == 0.0 and np.isnan(out[2][0]) and out[3][0] == gku.F64_MAX and out[4][0] == -gku.F64_MAX
    # UInt64 keys sort unsigned, Int64 signed
    u = Column.from_numpy(np.array([2**63 + 1, 5, 2**63 + 1], dtype=np.uint64))
    i = Column.from_numpy(np.array([-1, 3, -1], dtype=np.int64))
    assert gku.model([gku.key_values(u), gku.key_values(i)], [u, i], [])[0] == [(5, 3), (2**63 + 1, -1)]
    assert gku.model([gku.key_values(i), gku.key_values(u)], [u, i], [])[0] == [(-1, 2**63 + 1), (3, 5)]


def test_model_agrees_with_the_oracle_through_dense_ids():
    from oracle import oracle as orc

    rng = np.random.default_rng(1)
    n = 3000
    a = Column.from_numpy(rng.integers(-3, 3, n).astype(np.int64), mask=rng.random(n) > 0.1)
    s = gku.utf8_column([b"s%d" % x for x in rng.integers(0, 4, n)], rng.random(n) > 0.1)
    v = Column.from_numpy(rng.integers(-9, 9, n).astype(np.float64), mask=rng.random(n) > 0.2)
    w = Column.from_numpy(rng.integers(0, 10, n).astype(np.int64), mask=rng.random(n) > 0.2)
    cols = [a, s, v, w]
    aggs = [(f, 2) for f in (AggregateFunc.Count, AggregateFunc.Sum, AggregateFunc.Avg, AggregateFunc.Min, AggregateFunc.Max)]
    pred = PhysicalBinaryExpr.create(ColumnExpr.try_create(None, 3), Operator.Lt, PhysicalLiteralExpr.create(ScalarValue.Int64(5))).flatten([Field(f"c{i}", c.dtype) for i, c in enumerate(cols)])
    keep = w.valid_mask() & (w.to_numpy() < 5)  # a NULL predicate emits a NULL row: nothing of it is counted (Q4)
    tuples, exp, dense = gku.model([gku.key_values(a), gku.key_values(s)], cols, aggs, keep)
    idc = Column.from_numpy(np.where(dense < 0, 0, dense), mask=dense >= 0)
    ref = orc.aggregate([cols + [idc]], aggs + [(AggregateFunc.Min, 4)], group_nodes=[node_column(4)], pred_nodes=pred)[0]
    order = np.argsort(ref[-1].to_numpy(), kind="stable")
    assert len(tuples) == ref[0].length == 24
    for j in range(len(aggs)):
        g, e = exp[j], ref[j].to_numpy()[order]
        assert ((g == e) | (np.isnan(g.astype(np.float64)) & np.isnan(e.astype(np.float64)))).all(), j


def test_golden_is_what_the_model_gives_for_the_committed_csv():
    with open(os.path.join(GOLDEN, "group_keys_expected.json")) as f:
        doc = json.load(f)
    b = read_csv(os.path.join(GOLDEN, "test_data.csv"))
    ids, age = b.columns[0], b.columns[2]
    keys = [[int(x) % 3 for x in ids.to_numpy()], gku.key_values(age)]
    aggs = [(AggregateFunc.Count, 3), (AggregateFunc.Sum, 3), (AggregateFunc.Min, 0), (AggregateFunc.Max, 3)]
    for q in doc["queries"]:
        keep = age.to_numpy() > 19 if "where" in q["sql"] else None
        tuples, out, _ = gku.model(keys, b.columns, aggs, keep)
        rows = [list(t) + [o[g].item() for o in out] for g, t in enumerate(tuples)]
        assert rows == q["rows"] and len(q["columns"]) == 6, q["name"]
