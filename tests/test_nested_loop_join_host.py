"""CPU-only: the NestedLoopJoin operator (nested_loop_join.rs:30-184, quirk Q17) exists in every layer — the C ABI header and its
binding, the Python mirror and its rewrite arm, the C++ mirror, the Rust shim's declaration and rewrite arm.  No device is touched:
the stub sources below are never executed."""
import ctypes as C
import inspect
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
ON = [(pp.ColumnRef("employee", "rank"), pp.ColumnRef("rank", "id"))]


class _Stub:
    def __init__(self, schema):
        self._schema = schema

    def schema(self):
        return self._schema

    def scan(self, projection):
        raise AssertionError("a stub source is never scanned here")


def test_header_declares_the_entry_point():
    hdr = open(os.path.join(ROOT, "include", "nqe.h")).read()
    assert re.search(r"nqe_status\s+nqe_nested_loop_join_execute\s*\(\s*nqe_ctx\s*\*\s*ctx\s*,\s*const nqe_table\s*\*\s*left\s*,\s*"
                     r"const nqe_table\s*\*\s*right\s*,\s*int32_t\s+left_key\s*,\s*int32_t\s+right_key\s*,\s*nqe_table\s*\*\*\s*out\s*\)\s*;", hdr)
    assert "#define NQE_ABI_VERSION 1" in hdr


def test_capi_binds_the_symbol_with_its_signature():
    from naive_query_engine_amd import capi

    assert "nqe_nested_loop_join_execute" in capi.SYMBOLS
    fn = capi.lib().nqe_nested_loop_join_execute
    assert fn.restype is C.c_int32
    assert [a for a in fn.argtypes[3:5]] == [C.c_int32, C.c_int32] and len(fn.argtypes) == 6
    assert list(inspect.signature(capi.Context.nested_loop_join).parameters) == ["self", "left", "right", "left_key", "right_key"]


def test_mirror_class_constructor_order_and_children():
    left, right = pp.ScanPlan.create(_Stub(EMP)), pp.ScanPlan.create(_Stub(RANK))
    assert list(inspect.signature(pp.NestedLoopJoin.create).parameters) == ["left", "right", "on", "join_type", "schema"]
    j = pp.NestedLoopJoin.create(left, right, ON, pp.JoinType.Inner, EMP + RANK)
    assert isinstance(j, pp.PhysicalPlan)
    assert [f.name for f in j.schema()] == ["id", "name", "department_id", "rank", "id", "rank_name"]
    assert j.children() == [left, right] and j.on == ON and j.join_type == pp.JoinType.Inner
    import naive_query_engine_amd

    assert naive_query_engine_amd.physical_plan.NestedLoopJoin is pp.NestedLoopJoin  # reached like CrossJoin


def test_rewrite_substitutes_below_a_nested_loop_join_and_is_idempotent():
    pred = PhysicalBinaryExpr.create(ColumnExpr.try_create("id", None), Operator.Gt, PhysicalLiteralExpr.create(ScalarValue.Int64(0)))
    left = pp.ScanPlan.create(_Stub(EMP))
    right = pp.SelectionPlan.create(pp.ScanPlan.create(_Stub(RANK)), pred)
    proj = pp.ProjectionPlan.create(pp.SelectionPlan.create(pp.ScanPlan.create(_Stub(EMP)), pred), EMP, [ColumnExpr.try_create(f.name, None) for f in EMP])
    tree = pp.SelectionPlan.create(pp.NestedLoopJoin.create(proj, right, ON, pp.JoinType.Inner, EMP + RANK), pred)
    assert plan_shape(tree) == ["SelectionPlan", "NestedLoopJoin", "ProjectionPlan", "SelectionPlan", "ScanPlan", "SelectionPlan", "ScanPlan"]
    out = rewrite(tree)
    shape = ["SelectionPlan", "NestedLoopJoin", "FusedSelectionProjectionPlan", "ScanPlan", "SelectionPlan", "ScanPlan"]
    assert plan_shape(out) == shape  # the children are rewritten, the operator is kept
    j = out.input
    assert isinstance(j, pp.NestedLoopJoin) and j is not tree.input and j.on == ON and j.join_type == pp.JoinType.Inner
    assert j.right is not right and j.right.input is right.input
    assert [f.name for f in j.schema()] == [f.name for f in EMP + RANK]
    assert plan_shape(rewrite(out)) == shape
    del left


def test_rust_shim_declares_and_rewrites_nested_loop_join():
    path = os.path.join(ROOT, "integration", "rust", "gpu.rs")
    src = crs.strip_rust(open(path).read())
    assert "nqe_nested_loop_join_execute" in crs.extern_functions(src)
    assert "pub struct GpuNestedLoopJoin" in src and "impl GpuExec for GpuNestedLoopJoin" in src and "impl PhysicalPlan for GpuNestedLoopJoin" in src
    body = src[src.index("pub fn rewrite_sharded"):]
    assert "downcast_ref::<NestedLoopJoin>()" in body
    arm = body[body.index("downcast_ref::<NestedLoopJoin>()"):]
    assert "comm.is_none()" in arm[:200]  # sharded plans keep the CPU operator
    assert crs.check(path)[0] == []


def test_cpp_mirror_has_nested_loop_join():
    hpp = open(os.path.join(ROOT, "naive_query_engine_amd", "host", "naive_db.hpp")).read()
    assert "struct NestedLoopJoin : PhysicalPlan" in hpp
    assert "std::dynamic_pointer_cast<NestedLoopJoin>(plan)" in hpp
    assert "nqe_nested_loop_join_execute(" in hpp
