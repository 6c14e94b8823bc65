"""CPU-only: DISTINCT and the set operators (quirk Q24) in every host layer — the Python mirrors and their rewrite arms over stub
sources, the ctypes signatures and the enum against the header, the C++ mirror, the Rust shim, and the golden file against the model of
tests/set_ops_util.py and against sqlite3.  No device is touched: the stub sources below are never executed."""
import ctypes as C
import inspect
import os
import re
import sqlite3
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import set_ops_util as su  # noqa: E402
import naive_query_engine_amd as nqe  # noqa: E402
from naive_query_engine_amd import ColumnExpr, DType, Field, Operator, PhysicalBinaryExpr, PhysicalLiteralExpr, ScalarValue, SetOp  # noqa: E402
from naive_query_engine_amd import physical_plan as pp  # noqa: E402
from naive_query_engine_amd.rewrite import plan_shape, rewrite  # noqa: E402
from tools import check_rust_shim as crs  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
CSRC = os.path.join(ROOT, "naive_query_engine_amd", "csrc")
EMP = [Field("id", DType.INT64), Field("name", DType.UTF8), Field("department_id", DType.INT64), Field("rank", DType.INT64)]
HDR = open(os.path.join(ROOT, "include", "nqe.h")).read()


class _Stub:
    def __init__(self, schema):
        self._schema = schema

    def schema(self):
        return self._schema

    def scan(self, projection):
        raise AssertionError("a stub source is never scanned here")


def col(name):
    return ColumnExpr.try_create(name, None)


# ----------------------------------------------------------------------------- the Python mirrors
def test_mirror_construction_schema_children():
    scan, other = pp.ScanPlan.create(_Stub(EMP)), pp.ScanPlan.create(_Stub(EMP[:2]))
    assert list(inspect.signature(pp.PhysicalDistinctPlan.create).parameters) == ["input", "on"]
    assert list(inspect.signature(pp.PhysicalSetOpPlan.create).parameters) == ["left", "right", "op"]
    star = pp.PhysicalDistinctPlan.create(scan)
    assert isinstance(star, pp.PhysicalPlan) and star.on is None and star.children() == [scan] and star.schema() == scan.schema()
    expr = PhysicalBinaryExpr.create(col("id"), Operator.Modulos, PhysicalLiteralExpr.create(ScalarValue.Int64(2)))
    on = pp.PhysicalDistinctPlan.create(scan, [col("rank"), expr])
    assert on.on == [on.on[0], expr] and on.schema() == scan.schema()  # the temporary column of the expression is no field
    for op in SetOp:
        s = pp.PhysicalSetOpPlan.create(scan, other, op)
        assert isinstance(s, pp.PhysicalPlan) and s.op is op and s.children() == [scan, other] and s.schema() == scan.schema()  # left's schema
    assert pp.PhysicalSetOpPlan.create(scan, other, 2).op is SetOp.Except
    with pytest.raises(ValueError):
        pp.PhysicalSetOpPlan.create(scan, other, 3)


def test_rewrite_keeps_the_nodes_and_rewrites_their_children():
    pred = PhysicalBinaryExpr.create(col("id"), Operator.Gt, PhysicalLiteralExpr.create(ScalarValue.Int64(0)))
    proj = lambda: pp.ProjectionPlan.create(pp.SelectionPlan.create(pp.ScanPlan.create(_Stub(EMP)), pred), EMP, [col(f.name) for f in EMP])
    d = pp.PhysicalDistinctPlan.create(proj(), [col("rank")])
    assert plan_shape(d) == ["PhysicalDistinctPlan", "ProjectionPlan", "SelectionPlan", "ScanPlan"]
    out = rewrite(d)
    assert plan_shape(out) == ["PhysicalDistinctPlan", "FusedSelectionProjectionPlan", "ScanPlan"]
    assert isinstance(out, pp.PhysicalDistinctPlan) and out is not d and out.on == d.on
    assert plan_shape(d) == ["PhysicalDistinctPlan", "ProjectionPlan", "SelectionPlan", "ScanPlan"]  # the input tree is left as it was
    assert rewrite(pp.PhysicalDistinctPlan.create(proj())).on is None
    s = pp.PhysicalSetOpPlan.create(proj(), pp.PhysicalDistinctPlan.create(proj()), SetOp.Except)
    assert plan_shape(s) == ["PhysicalSetOpPlan", "ProjectionPlan", "SelectionPlan", "ScanPlan", "PhysicalDistinctPlan", "ProjectionPlan", "SelectionPlan", "ScanPlan"]
    out = rewrite(s)
    assert plan_shape(out) == ["PhysicalSetOpPlan", "FusedSelectionProjectionPlan", "ScanPlan", "PhysicalDistinctPlan", "FusedSelectionProjectionPlan", "ScanPlan"]
    assert isinstance(out, pp.PhysicalSetOpPlan) and out.op is SetOp.Except and plan_shape(rewrite(out)) == plan_shape(out)
    # a limit above either node stays a limit
    assert plan_shape(rewrite(pp.PhysicalLimitPlan.create(d, 3)))[:2] == ["PhysicalLimitPlan", "PhysicalDistinctPlan"]


# ----------------------------------------------------------------------------- the C ABI
def test_header_declares_the_enum_the_limit_and_the_entry_points():
    assert re.search(r"nqe_status\s+nqe_distinct_execute\s*\(\s*nqe_ctx\s*\*\s*ctx\s*,\s*const nqe_table\s*\*\s*in\s*,\s*const int32_t\s*\*\s*cols\s*,\s*int32_t\s+num_cols\s*,\s*nqe_table\s*\*\*\s*out\s*\)\s*;", HDR)
    assert re.search(r"nqe_status\s+nqe_set_op_execute\s*\(\s*nqe_ctx\s*\*\s*ctx\s*,\s*const nqe_table\s*\*\s*left\s*,\s*const nqe_table\s*\*\s*right\s*,\s*int32_t\s+op\s*,\s*nqe_table\s*\*\*\s*out\s*\)\s*;", HDR)
    assert "#define NQE_MAX_SET_KEYS 32" in HDR and "#define NQE_ABI_VERSION 1" in HDR
    body = re.search(r"typedef enum nqe_set_op\s*\{(.*?)\}\s*nqe_set_op\s*;", HDR, flags=re.S).group(1)
    values = {n[len("NQE_SET_"):].lower(): int(v) for n, v in re.findall(r"(NQE_\w+)\s*=\s*(\d+)", body)}
    assert values == {m.name.lower(): int(m) for m in SetOp} == {"union": 0, "intersect": 1, "except": 2}
    assert nqe.SetOp is SetOp and "SetOp" in nqe.__all__
    text = " ".join(HDR[HDR.index("DISTINCT and the set operators"):HDR.index("#define NQE_MAX_SET_KEYS")].replace("*", " ").split())
    for words in ("INTERSECT ALL and EXCEPT ALL", "count(distinct x)", "DISTINCT over expressions", "SQL parsing", "sharded forms"):  # out of scope, said so
        assert words in text, words
    for words in ("a NULL equals a NULL", "-0.0 = +0.0", "every NaN equals every NaN", "the empty string is a value", "smallest row index", "quirk Q24"):
        assert words in text, words
    unit = " ".join(open(os.path.join(CSRC, "set_ops.hip")).read().replace("//", " ").split())
    for words in ("INTERSECT ALL and EXCEPT ALL", "count(distinct x)", "DISTINCT over expressions", "SQL parsing", "sharded forms"):
        assert words in unit, words


def test_bindings_match_the_header():
    from naive_query_engine_amd import capi

    assert "nqe_distinct_execute" in capi.SYMBOLS and "nqe_set_op_execute" in capi.SYMBOLS
    d, s = capi.lib().nqe_distinct_execute, capi.lib().nqe_set_op_execute
    assert d.restype is C.c_int32 and d.argtypes == [C.c_void_p, C.c_void_p, C.POINTER(C.c_int32), C.c_int32, C.POINTER(C.c_void_p)]
    assert s.restype is C.c_int32 and s.argtypes == [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_void_p)]
    assert list(inspect.signature(capi.Context.distinct).parameters) == ["self", "table", "cols"]
    assert inspect.signature(capi.Context.distinct).parameters["cols"].default is None
    assert list(inspect.signature(capi.Context.set_op).parameters) == ["self", "left", "right", "op"]


def test_the_unit_is_built_and_its_plan_header_is_plain_cpp():
    unit = open(os.path.join(CSRC, "set_ops.hip")).read()
    assert re.search(r"^SRCS := .*\bset_ops\.hip\b", open(os.path.join(CSRC, "Makefile")).read(), flags=re.M)
    assert re.search(r'^UNITS=".*\bset_ops\b', open(os.path.join(ROOT, "tools", "build_variant.sh")).read(), flags=re.M)
    plan = open(os.path.join(CSRC, "set_ops_plan.hpp")).read()
    assert "hip/hip_runtime.h" not in plan and "nqe_internal.hpp" not in plan
    for label in ("set_table_init", "set_insert", "set_find", "set_keep"):
        assert f'"{label}"' in unit, label
    kernels = open(os.path.join(CSRC, "set_ops_kernels.hpp")).read()
    assert "asm" not in re.sub(r"//.*", "", kernels) and "asm" not in re.sub(r"//.*", "", unit)  # plain HIP C++ throughout
    assert "finish_mask(" in unit and "compact_column(" in unit and "nqe_table_concat(" in unit
    # with 2^32 slots every u32 is a slot index: no slot is ever compared with the empty-row sentinel; found / not found travels apart
    code = re.sub(r"//.*", "", kernels)
    assert not re.search(r"\bs(lot)?\s*[!=]=\s*setop::EMPTY", code) and "bool set_probe(" in code and "bool found" in code
    assert "getenv" not in re.sub(r"//.*", "", unit)  # no run-time switch in the operator's path
    assert "count_nulls_exact(" in unit and "count_nulls_exact(" in open(os.path.join(CSRC, "nqe_internal.hpp")).read()  # the join's helper, not a copy


# ----------------------------------------------------------------------------- the other mirrors
def test_cpp_mirror_has_both_plans_and_the_rewrite_arms():
    hpp = open(os.path.join(ROOT, "naive_query_engine_amd", "host", "naive_db.hpp")).read()
    assert "struct PhysicalDistinctPlan : PhysicalPlan" in hpp and "struct PhysicalSetOpPlan : PhysicalPlan" in hpp
    assert "nqe_distinct_execute(" in hpp and "nqe_set_op_execute(" in hpp
    arm = hpp[hpp.index("inline PhysicalPlanRef rewrite("):]
    assert "std::dynamic_pointer_cast<PhysicalDistinctPlan>(plan)" in arm and "PhysicalDistinctPlan::create(rewrite(d->input), d->on)" in arm
    assert "std::dynamic_pointer_cast<PhysicalSetOpPlan>(plan)" in arm and "PhysicalSetOpPlan::create(rewrite(so->left), rewrite(so->right), so->op)" in arm


def test_rust_shim_declares_the_entry_points_and_both_plans():
    path = os.path.join(ROOT, "integration", "rust", "gpu.rs")
    src = crs.strip_rust(open(path).read())
    fns = crs.extern_functions(src)
    assert "nqe_distinct_execute" in fns and "nqe_set_op_execute" in fns
    assert "pub const NQE_SET_UNION: i32 = 0; pub const NQE_SET_INTERSECT: i32 = 1; pub const NQE_SET_EXCEPT: i32 = 2;" in src
    for name in ("GpuDistinctPlan", "GpuSetOpPlan"):
        assert f"pub struct {name}" in src and f"impl GpuExec for {name}" in src and f"impl PhysicalPlan for {name}" in src and f"downcast_ref::<{name}>()" in src
    assert crs.check(path)[0] == []


# ----------------------------------------------------------------------------- the golden file
def test_golden_file_holds_the_models_results_and_sqlite_agrees():
    doc, tables = su.golden_load(GOLDEN)
    qs = doc["queries"]
    assert len(qs) == 13 and {q["kind"] for q in qs} == {"distinct", "set_op"} and {q["op"] for q in qs if q["kind"] == "set_op"} == {m.name for m in SetOp}
    assert any(q["kind"] == "distinct" and q["on"] is None for q in qs) and any(q["kind"] == "distinct" and q["on"] for q in qs)
    db = sqlite3.connect(":memory:")
    for name, (fields, cols) in tables.items():
        db.execute(f"create table {name} ({', '.join(f.name for f in fields)})")
        db.executemany(f"insert into {name} values ({', '.join('?' * len(fields))})", [tuple(r) for r in zip(*[c.to_list() for c in cols])])
    for q in qs:
        columns, rows = su.golden_model(tables, q)
        assert q["columns"] == columns and q["rows"] == rows, q["name"]
        if q["sql"]:  # SQLite picks its own order: the same rows as sets, and as many
            got = db.execute(q["sql"]).fetchall()
            assert len(got) == len(rows) and set(got) == {tuple(r) for r in rows}, q["name"]
