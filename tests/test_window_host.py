"""CPU-only: window functions (quirk Q23) in every host layer — the Python mirror and its rewrite arm over stub sources, the
nqe_window_spec binding and the enums against the header, the C++ mirror, the Rust shim, and the golden queries against the model of
tests/window_util.py and against sqlite3.  No device is touched: the stub sources below are never executed."""
import ctypes as C
import inspect
import json
import os
import re
import sqlite3
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import order_by_util as obu  # noqa: E402
import window_util as wu  # noqa: E402
import naive_query_engine_amd as nqe  # noqa: E402
from naive_query_engine_amd import (ColumnExpr, DType, ErrorCode, Field, Operator, PhysicalBinaryExpr, PhysicalLiteralExpr, ScalarValue, Status, WindowFrame as F,  # noqa: E402
                                    WindowFunc as W, read_csv)
from naive_query_engine_amd import physical_plan as pp  # noqa: E402
from naive_query_engine_amd.rewrite import plan_shape, rewrite  # noqa: E402
from tools import check_rust_shim as crs  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
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


# ----------------------------------------------------------------------------- the Python mirror
def test_mirror_construction_schema_children():
    scan = pp.ScanPlan.create(_Stub(EMP))
    assert list(inspect.signature(pp.WindowFunction.__init__).parameters) == ["self", "func", "expr", "frame"]
    assert list(inspect.signature(pp.PhysicalWindowPlan.__init__).parameters) == ["self", "input", "partition_by", "order_by", "funcs"]
    assert pp.WindowFunction(W.Sum, col("id")).frame == F.Range and pp.WindowFunction(W.Rank).expr is None  # RANGE: SQL's default with ORDER BY
    with pytest.raises(ErrorCode) as e:
        pp.WindowFunction(W.Avg)
    assert e.value.status == Status.PlanError
    expr = PhysicalBinaryExpr.create(col("id"), Operator.Plus, PhysicalLiteralExpr.create(ScalarValue.Int64(1)))
    funcs = [pp.WindowFunction.create(W.RowNumber), pp.WindowFunction(W.Rank), pp.WindowFunction(W.DenseRank), pp.WindowFunction(W.Count, col("name")),
             pp.WindowFunction(W.Sum, col("rank"), F.Rows), pp.WindowFunction(W.Min, ColumnExpr.try_create(None, 0), F.Partition), pp.WindowFunction(W.Max, col("id")),
             pp.WindowFunction(W.Avg, col("department_id")), pp.WindowFunction(W.Sum, expr)]
    part, order = [col("department_id"), expr], [pp.PhysicalSortExpr(col("name"), descending=True)]
    plan = pp.PhysicalWindowPlan.create(scan, part, order, funcs)
    assert isinstance(plan, pp.PhysicalPlan) and plan.children() == [scan] and plan.partition_by == part and plan.order_by == order and plan.funcs == funcs
    fields = plan.schema()
    # the input's fields, then one per function in the aggregates' naming; the temporary columns of the expressions are no fields
    assert [f.name for f in fields] == ["id", "name", "department_id", "rank", "row_number()", "rank()", "dense_rank()", "count(name)", "sum(rank)", "min(id)", "max(id)",
                                        "avg(department_id)", f"sum({expr!r})"]
    assert [f.dtype for f in fields[4:]] == [DType.UINT64] * 4 + [DType.FLOAT64] * 5 and not any(f.nullable for f in fields[4:])
    assert fields[:4] == list(scan.schema())


def test_rewrite_keeps_the_node_and_rewrites_its_input():
    pred = PhysicalBinaryExpr.create(col("id"), Operator.Gt, PhysicalLiteralExpr.create(ScalarValue.Int64(0)))
    proj = pp.ProjectionPlan.create(pp.SelectionPlan.create(pp.ScanPlan.create(_Stub(EMP)), pred), EMP, [col(f.name) for f in EMP])
    funcs = [pp.WindowFunction(W.Rank), pp.WindowFunction(W.Sum, col("id"), F.Rows)]
    win = pp.PhysicalWindowPlan.create(proj, [col("department_id")], [pp.PhysicalSortExpr(col("name"))], funcs)
    assert plan_shape(win) == ["PhysicalWindowPlan", "ProjectionPlan", "SelectionPlan", "ScanPlan"]
    out = rewrite(win)
    assert plan_shape(out) == ["PhysicalWindowPlan", "FusedSelectionProjectionPlan", "ScanPlan"]
    assert isinstance(out, pp.PhysicalWindowPlan) and out is not win and out.funcs == funcs and out.partition_by == win.partition_by and out.order_by == win.order_by
    assert plan_shape(win) == ["PhysicalWindowPlan", "ProjectionPlan", "SelectionPlan", "ScanPlan"]  # the input tree is left as it was
    assert plan_shape(rewrite(out)) == plan_shape(out)
    # a limit above a window stays a limit (every row's value depends on its whole partition); a sort above it keeps folding its own limit
    assert plan_shape(rewrite(pp.PhysicalLimitPlan.create(win, 3))) == ["PhysicalLimitPlan", "PhysicalWindowPlan", "FusedSelectionProjectionPlan", "ScanPlan"]
    top = rewrite(pp.PhysicalLimitPlan.create(pp.PhysicalSortPlan.create(win, [pp.PhysicalSortExpr(col("id"))]), 2))
    assert plan_shape(top) == ["PhysicalSortPlan", "PhysicalWindowPlan", "FusedSelectionProjectionPlan", "ScanPlan"] and top.fetch == 2


# ----------------------------------------------------------------------------- the C ABI
def test_header_declares_the_enums_the_struct_and_the_entry_point():
    assert re.search(r"nqe_status\s+nqe_window_execute\s*\(\s*nqe_ctx\s*\*\s*ctx\s*,\s*const nqe_table\s*\*\s*in\s*,\s*const int32_t\s*\*\s*partition_cols\s*,\s*int32_t\s+num_partition\s*,\s*"
                     r"const nqe_sort_key\s*\*\s*order_keys\s*,\s*int32_t\s+num_order\s*,\s*const nqe_window_spec\s*\*\s*funcs\s*,\s*int32_t\s+num_funcs\s*,\s*nqe_table\s*\*\*\s*out\s*\)\s*;", HDR)
    assert "#define NQE_MAX_WINDOW_KEYS 8" in HDR and "#define NQE_MAX_WINDOW_FUNCS 16" in HDR and "#define NQE_ABI_VERSION 1" in HDR
    for enum, py in (("nqe_window_func", W), ("nqe_window_frame", F)):
        body = re.search(r"typedef enum %s\s*\{(.*?)\}\s*%s\s*;" % (enum, enum), HDR, flags=re.S).group(1)
        values = {n: int(v) for n, v in re.findall(r"(NQE_\w+)\s*=\s*(\d+)", body)}
        squash = lambda s: s.replace("_", "").lower()
        prefix = "NQE_WIN_" if py is W else "NQE_FRAME_"
        assert {squash(n[len(prefix):]): v for n, v in values.items()} == {squash(m.name): int(m) for m in py}
    assert nqe.WindowFunc is W and nqe.WindowFrame is F and "WindowFunc" in nqe.__all__ and "WindowFrame" in nqe.__all__
    text = HDR[HDR.index("window functions"):HDR.index("nqe_status nqe_window_execute")]
    for words in ("n PRECEDING", "LAG / LEAD / FIRST_VALUE / NTILE", "several different windows", "SQL parsing"):  # out of scope, said so
        assert words in " ".join(text.replace("*", " ").split()), words


def test_window_spec_binding_matches_the_header_struct():
    from naive_query_engine_amd import capi

    m = re.search(r"typedef struct nqe_window_spec\s*\{(.*?)\}\s*nqe_window_spec\s*;", HDR, flags=re.S)
    assert m
    fields = re.findall(r"(\w+)\s+(\w+)\s*;", re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S))
    assert fields == [("int32_t", "func"), ("int32_t", "column"), ("int32_t", "frame")]
    assert [(n, t) for n, t in capi.NqeWindowSpec._fields_] == [(n, C.c_int32) for _, n in fields]
    assert C.sizeof(capi.NqeWindowSpec) == 12 and [getattr(capi.NqeWindowSpec, n).offset for _, n in fields] == [0, 4, 8]
    assert "nqe_window_execute" in capi.SYMBOLS
    fn = capi.lib().nqe_window_execute
    assert fn.restype is C.c_int32 and len(fn.argtypes) == 9 and [fn.argtypes[i] for i in (3, 5, 7)] == [C.c_int32] * 3
    assert list(inspect.signature(capi.Context.window).parameters) == ["self", "table", "partition_by", "order_by", "funcs"]


def test_the_unit_loads_on_first_use_and_the_tile_is_a_constant_of_the_plan_header():
    csrc = os.path.join(ROOT, "naive_query_engine_amd", "csrc")
    unit = open(os.path.join(csrc, "window.hip")).read()
    code = "\n".join(line.split("//")[0] for line in unit.splitlines())
    assert "NQE_MODULE_PROBE" not in code  # an eagerly loaded unit once cost the headline aggregate 1.3 %
    assert re.search(r"^SRCS := .*\bwindow\.hip\b", open(os.path.join(csrc, "Makefile")).read(), flags=re.M)
    assert re.search(r"constexpr int64_t WIN_TILE = \d+;", open(os.path.join(csrc, "window_plan.hpp")).read())
    assert "hip/hip_runtime.h" not in open(os.path.join(csrc, "window_plan.hpp")).read()
    assert "build_sort_permutation" in open(os.path.join(csrc, "nqe_internal.hpp")).read() and "build_sort_permutation(" in unit


# ----------------------------------------------------------------------------- the other mirrors
def test_cpp_mirror_has_the_window_plan_and_the_rewrite_arm():
    hpp = open(os.path.join(ROOT, "naive_query_engine_amd", "host", "naive_db.hpp")).read()
    assert "struct WindowFunction" in hpp and "struct PhysicalWindowPlan : PhysicalPlan" in hpp and "nqe_window_execute(" in hpp
    arm = hpp[hpp.index("inline PhysicalPlanRef rewrite("):]
    assert "std::dynamic_pointer_cast<PhysicalWindowPlan>(plan)" in arm and "PhysicalWindowPlan::create(rewrite(w->input)" in arm


def test_rust_shim_declares_the_entry_point_and_a_window_plan():
    path = os.path.join(ROOT, "integration", "rust", "gpu.rs")
    src = crs.strip_rust(open(path).read())
    assert "nqe_window_execute" in crs.extern_functions(src)
    assert "pub struct NqeWindowSpec { pub func: i32, pub column: i32, pub frame: i32 }" in src
    assert "pub struct GpuWindowPlan" in src and "impl GpuExec for GpuWindowPlan" in src and "impl PhysicalPlan for GpuWindowPlan" in src
    assert "downcast_ref::<GpuWindowPlan>()" in src
    assert crs.check(path)[0] == []


# ----------------------------------------------------------------------------- golden queries
def _golden():
    with open(os.path.join(GOLDEN, "window_expected.json")) as f:
        return json.load(f)["queries"]


def _rows(cols):
    vals = [[v.decode() if isinstance(v, bytes) else v for v in obu.column_values(c)] for c in cols]
    return [list(r) for r in zip(*vals)]


def test_golden_queries_match_the_model_and_sqlite():
    qs = _golden()
    assert [q["name"] for q in qs] == ["running_total_per_department", "rank_by_name_descending_beside_the_group_average", "peers_without_partition", "no_keys_at_all"]
    assert {f["func"] for q in qs for f in q["funcs"]} == {m.name for m in W}  # all eight functions
    assert {f["frame"] for q in qs for f in q["funcs"] if f["column"] is not None} == {m.name for m in F}
    for q in qs:
        batch = read_csv(os.path.join(GOLDEN, q["table"] + ".csv"))
        names = [f.name for f in batch.fields]
        funcs = [(W[f["func"]], None if f["column"] is None else names.index(f["column"]), F[f["frame"]]) for f in q["funcs"]]
        model = wu.window(batch.columns, [names.index(c) for c in q["partition_by"]], [(names.index(k["column"]), k["descending"], k["nulls_first"]) for k in q["order_by"]], funcs)
        assert q["columns"][:len(names)] == names and len(q["columns"]) == len(names) + len(funcs)
        assert q["rows"] == [a + b for a, b in zip(_rows(batch.columns), [list(r) for r in zip(*[c.tolist() for c in model.cols])])], q["name"]
        # the same query through SQLite: its rows in input order (every golden frame holds a valid row, the values are small integers)
        db = sqlite3.connect(":memory:")
        db.execute(f"create table {q['table']} ({', '.join(names)})")
        db.executemany(f"insert into {q['table']} values ({', '.join('?' * len(names))})", _rows(batch.columns))
        got = [list(r) for r in db.execute(q["sql"] + f" order by {names[0]}")]
        assert got == q["rows"], q["name"]
