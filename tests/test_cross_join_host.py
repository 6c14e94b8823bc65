"""CPU-only: the CrossJoin operator (cross_join.rs:26-192, quirk Q15) exists in every layer — the Python mirror and its rewrite arm,
the C ABI header and its binding list, the Rust shim's declaration and rewrite arm.  No device is touched: the stub sources below are
never executed."""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from naive_query_engine_amd import ColumnExpr, DType, Field, Operator, PhysicalBinaryExpr, PhysicalLiteralExpr, ScalarValue  # noqa: E402
from naive_query_engine_amd import physical_plan as pp  # noqa: E402
from naive_query_engine_amd.rewrite import plan_shape, rewrite  # noqa: E402
from tools import check_rust_shim as crs  # noqa: E402

EMP = [Field("id", DType.INT64), Field("name", DType.UTF8), Field("department_id", DType.INT64), Field("rank", DType.INT64)]
RANK = [Field("id", DType.INT64), Field("rank_name", DType.UTF8)]


class _Stub:
    def __init__(self, schema):
        self._schema = schema

    def schema(self):
        return self._schema

    def scan(self, projection):
        raise AssertionError("a stub source is never scanned here")


def test_cross_join_builds_and_reports_schema_and_children():
    left, right = pp.ScanPlan.create(_Stub(EMP)), pp.ScanPlan.create(_Stub(RANK))
    cj = pp.CrossJoin.create(left, right, pp.JoinType.Cross, EMP + RANK)
    assert [f.name for f in cj.schema()] == ["id", "name", "department_id", "rank", "id", "rank_name"]
    assert cj.children() == [left, right]
    assert cj.join_type == pp.JoinType.Cross


def _select_star(child):
    # the planner resolves `select *` by name, first match (Q12): the second `id` is column 0
    schema = EMP + RANK
    return pp.ProjectionPlan.create(child, schema, [ColumnExpr.try_create(f.name, None) for f in schema])


def test_rewrite_substitutes_below_a_cross_join_and_is_idempotent():
    pred = PhysicalBinaryExpr.create(ColumnExpr.try_create("id", None), Operator.Gt, PhysicalLiteralExpr.create(ScalarValue.Int64(0)))
    left = pp.ScanPlan.create(_Stub(EMP))
    right = pp.SelectionPlan.create(pp.ScanPlan.create(_Stub(RANK)), pred)
    tree = _select_star(pp.CrossJoin.create(left, right, pp.JoinType.Cross, EMP + RANK))
    shape = ["ProjectionPlan", "CrossJoin", "ScanPlan", "SelectionPlan", "ScanPlan"]
    assert plan_shape(tree) == shape
    out = rewrite(tree)
    assert plan_shape(out) == shape
    cj = out.input
    assert isinstance(cj, pp.CrossJoin) and cj is not tree.input  # a new node over rewritten children
    assert cj.left is left and cj.right is not right and cj.right.input is right.input
    assert [f.name for f in cj.schema()] == [f.name for f in EMP + RANK]
    assert plan_shape(rewrite(out)) == shape
    # Projection∘Selection above the join still fuses; the join's children are rewritten
    above = pp.ProjectionPlan.create(pp.SelectionPlan.create(pp.CrossJoin.create(left, right, pp.JoinType.Cross, EMP + RANK), pred), EMP[:1],
                                     [ColumnExpr.try_create("id", None)])
    assert plan_shape(rewrite(above)) == ["FusedSelectionProjectionPlan", "CrossJoin", "ScanPlan", "SelectionPlan", "ScanPlan"]


def test_header_declares_the_entry_point_and_capi_binds_it():
    from naive_query_engine_amd import capi

    hdr = open(os.path.join(ROOT, "include", "nqe.h")).read()
    assert re.search(r"nqe_status\s+nqe_cross_join_execute\s*\(\s*nqe_ctx\s*\*\s*ctx\s*,\s*const nqe_table\s*\*\s*left\s*,\s*"
                     r"const nqe_table\s*\*\s*right\s*,\s*nqe_table\s*\*\*\s*out\s*\)\s*;", hdr)
    assert "#define NQE_ABI_VERSION 1" in hdr
    assert "nqe_cross_join_execute" in capi.SYMBOLS
    assert hasattr(capi.Context, "cross_join")


def test_rust_shim_declares_and_rewrites_cross_join():
    path = os.path.join(ROOT, "integration", "rust", "gpu.rs")
    src = crs.strip_rust(open(path).read())
    assert "nqe_cross_join_execute" in crs.extern_functions(src)
    body = src[src.index("pub fn rewrite_sharded"):]
    assert "downcast_ref::<CrossJoin>()" in body
    arm = body[body.index("downcast_ref::<CrossJoin>()"):]
    assert "comm.is_none()" in arm[:200]  # sharded plans keep the CPU operator
    assert crs.check(path)[0] == []


def test_cpp_mirror_has_cross_join():
    hpp = open(os.path.join(ROOT, "naive_query_engine_amd", "host", "naive_db.hpp")).read()
    assert "struct CrossJoin : PhysicalPlan" in hpp
    assert "std::dynamic_pointer_cast<CrossJoin>(plan)" in hpp
