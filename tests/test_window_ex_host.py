"""nqe_window_execute_ex on the host (quirk Q23's addendum): the header's enums, struct and entry point, the ctypes layout, the Python
mirror (WindowFunctionEx, PhysicalWindowPlanEx), the rewrite arm, the C++ mirror and the Rust shim, and the golden queries of
tests/golden/window_ex_expected.json against the model of tests/window_ex_util.py and against sqlite3.  The first entry's enums are
still what they were.  No device is touched: the stub sources below are never executed."""
import ctypes as C
import inspect
import json
import os
import re
import sqlite3
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import window_ex_util as wx  # noqa: E402
import naive_query_engine_amd as nqe  # noqa: E402
from naive_query_engine_amd import (ColumnExpr, DType, ErrorCode, Field, Operator, PhysicalBinaryExpr, PhysicalLiteralExpr, ScalarValue, Status, WindowFrame as F,  # noqa: E402
                                    WindowFrameEx as FX, WindowFunc as W, WindowFuncEx as WX, read_csv)
from naive_query_engine_amd import physical_plan as pp  # noqa: E402
from naive_query_engine_amd.rewrite import plan_shape, rewrite  # noqa: E402
from tools import check_rust_shim as crs  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
EMP = [Field("id", DType.INT64), Field("name", DType.UTF8), Field("department_id", DType.INT64), Field("rank", DType.INT64), Field("pay", DType.FLOAT64)]
HDR = open(os.path.join(ROOT, "include", "nqe.h")).read()
CSRC = os.path.join(ROOT, "naive_query_engine_amd", "csrc")


class _Stub:
    def __init__(self, schema):
        self._schema = schema

    def schema(self):
        return self._schema

    def scan(self, projection):
        raise AssertionError("a stub source is never scanned here")


def col(name):
    return ColumnExpr.try_create(name, None)


# ----------------------------------------------------------------------------- the C ABI
def _enum(name):
    body = re.search(r"typedef enum %s\s*\{(.*?)\}\s*%s\s*;" % (name, name), HDR, flags=re.S).group(1)
    return {n: int(v) for n, v in re.findall(r"(NQE_\w+)\s*=\s*(\d+)", re.sub(r"/\*.*?\*/", "", body, flags=re.S))}


def test_header_declares_the_enums_the_struct_and_the_entry_point():
    assert re.search(r"nqe_status\s+nqe_window_execute_ex\s*\(\s*nqe_ctx\s*\*\s*ctx\s*,\s*const nqe_table\s*\*\s*in\s*,\s*const int32_t\s*\*\s*partition_cols\s*,\s*int32_t\s+num_partition\s*,\s*"
                     r"const nqe_sort_key\s*\*\s*order_keys\s*,\s*int32_t\s+num_order\s*,\s*const nqe_window_spec_ex\s*\*\s*funcs\s*,\s*int32_t\s+num_funcs\s*,\s*nqe_table\s*\*\*\s*out\s*\)\s*;", HDR)
    assert "#define NQE_ABI_VERSION 1" in HDR and "#define NQE_FRAME_UNBOUNDED_PRECEDING INT64_MIN" in HDR and "#define NQE_FRAME_UNBOUNDED_FOLLOWING INT64_MAX" in HDR
    squash = lambda s: s.replace("_", "").lower()
    funcs, old_funcs, frames, old_frames = _enum("nqe_window_func_ex"), _enum("nqe_window_func"), _enum("nqe_window_frame_ex"), _enum("nqe_window_frame")
    assert {squash(n[len("NQE_WINX_"):]): v for n, v in funcs.items()} == {squash(m.name): int(m) for m in WX} and sorted(funcs.values()) == list(range(13))
    assert {squash(n[len("NQE_FRAMEX_"):]): v for n, v in frames.items()} == {squash(m.name): int(m) for m in FX} and sorted(frames.values()) == list(range(4))
    # 0..7 and 0..2 are the first entry's values, name for name
    assert {n[len("NQE_WIN_"):]: v for n, v in old_funcs.items()} == {n[len("NQE_WINX_"):]: v for n, v in funcs.items() if v <= 7}
    assert {n[len("NQE_FRAME_"):]: v for n, v in old_frames.items()} == {n[len("NQE_FRAMEX_"):]: v for n, v in frames.items() if v <= 2}
    assert all(int(WX[m.name]) == int(m) for m in W) and all(int(FX[m.name]) == int(m) for m in F)
    assert "WindowFuncEx" in nqe.__all__ and "WindowFrameEx" in nqe.__all__ and nqe.WindowFuncEx is WX and nqe.WindowFrameEx is FX
    assert len(W) == 8 and len(F) == 3  # the first entry's enums are untouched


def test_header_states_what_is_out_of_scope():
    text = " ".join(HDR[HDR.index("window functions, the wider entry"):HDR.index("typedef enum nqe_window_func_ex")].replace("*", " ").split())
    for words in ("RANGE and GROUPS frames with offsets", "EXCLUDE", "IGNORE NULLS", "NTH_VALUE / PERCENT_RANK / CUME_DIST", "value functions over Boolean / Utf8",
                  "several different windows in one call", "SQL parsing"):
        assert words in text, words
    head = open(os.path.join(CSRC, "window.hip")).read().split("#include")[0]
    assert "nqe_window_execute_ex" in head  # the unit's "out of scope" line points at the new entry


def test_window_spec_ex_binding_matches_the_header_struct():
    from naive_query_engine_amd import capi

    m = re.search(r"typedef struct nqe_window_spec_ex\s*\{(.*?)\}\s*nqe_window_spec_ex\s*;", HDR, flags=re.S)
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    union = re.search(r"union\s*\{(.*?)\}\s*default_value\s*;", body, flags=re.S)
    assert re.findall(r"(\w+)\s+(\w+)\s*;", union.group(1)) == [("int64_t", "i64"), ("uint64_t", "u64"), ("double", "f64")]
    plain = body[:union.start()]
    names = [n.strip() for t, ns in re.findall(r"(int32_t|int64_t)\s+([\w\s,]+);", plain) for n in ns.split(",")]
    assert names == ["func", "column", "frame", "has_default", "start", "end", "param"]
    S = capi.NqeWindowSpecEx
    assert [n for n, _ in S._fields_] == names + ["default_value"]
    assert [t for _, t in S._fields_[:7]] == [C.c_int32] * 4 + [C.c_int64] * 3 and [n for n, _ in capi.NqeWindowDefault._fields_] == ["i64", "u64", "f64"]
    assert C.sizeof(S) == 48 and [getattr(S, n).offset for n, _ in S._fields_] == [0, 4, 8, 12, 16, 24, 32, 40]
    assert capi.FRAME_UNBOUNDED_PRECEDING == -(2 ** 63) and capi.FRAME_UNBOUNDED_FOLLOWING == 2 ** 63 - 1
    assert "nqe_window_execute_ex" in capi.SYMBOLS
    fn = capi.lib().nqe_window_execute_ex
    assert fn.restype is C.c_int32 and len(fn.argtypes) == 9 and [fn.argtypes[i] for i in (3, 5, 7)] == [C.c_int32] * 3
    assert list(inspect.signature(capi.Context.window_ex).parameters) == ["self", "table", "partition_by", "order_by", "funcs"]


def test_the_new_entry_lives_in_the_window_unit():
    unit = open(os.path.join(CSRC, "window.hip")).read()
    code = "\n".join(line.split("//")[0] for line in unit.splitlines())
    assert "NQE_MODULE_PROBE" not in code
    # one body: both entries are defined here and each calls win_execute (its definition is the third mention) ...
    assert code.count("nqe_status nqe_window_execute(") == 1 and code.count("nqe_status nqe_window_execute_ex(") == 1 and code.count("win_execute(") == 3
    for entry in ("nqe_status nqe_window_execute(", "nqe_status nqe_window_execute_ex("):
        body = code[code.index(entry):].split("NQE_API_END()")[0]
        assert body.count("win_execute(") == 1 and "launch(" not in body and "make_word_column" not in body and "n == 0" not in body, entry
    assert code.count("plan_window(") == 1 and code.count("plan_window_ex(") == 1 and code.count("win_widen(") == 1  # (both defined in window_ex_plan.hpp)
    # ... and in it every stage function is defined once and called from one place, every emit launched from one place
    for stage in ("win_order(", "win_partition_states(", "win_emit_old("):
        assert code.count(stage) == 2, stage
        assert code[code.index("win_execute("):].count(stage) == 1, stage  # the call is win_execute's
    for label in ('"win_emit"', '"win_frame_emit"', '"win_value_emit"'):
        assert code.count("launch(ctx, " + label) == 1 and code.count(label) == 1, label
    make = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^window\.o:.*\bwindow_ex_kernels\.hpp\b.*\bwindow_ex_plan\.hpp\b", make, flags=re.M) and "window_ex" not in re.search(r"^SRCS := .*$", make, flags=re.M).group(0)
    plan = open(os.path.join(CSRC, "window_ex_plan.hpp")).read()
    assert "hip/hip_runtime.h" not in plan and "win_frame_pieces(" in plan and "win_frame_pieces(" in open(os.path.join(CSRC, "window_ex_kernels.hpp")).read()


# ----------------------------------------------------------------------------- the Python mirror
def test_mirror_construction_schema_children():
    scan = pp.ScanPlan.create(_Stub(EMP))
    assert list(inspect.signature(pp.WindowFunctionEx.__init__).parameters) == ["self", "func", "expr", "frame", "start", "end", "offset", "buckets", "default"]
    assert list(inspect.signature(pp.PhysicalWindowPlanEx.__init__).parameters) == ["self", "input", "partition_by", "order_by", "funcs"]
    assert pp.WindowFunctionEx(WX.Sum, col("id")).frame == FX.Range and pp.WindowFunctionEx(WX.Ntile, buckets=3).expr is None
    for fn in (WX.Avg, WX.Lag, WX.Lead, WX.FirstValue, WX.LastValue):
        with pytest.raises(ErrorCode) as e:
            pp.WindowFunctionEx(fn)
        assert e.value.status == Status.PlanError
    expr = PhysicalBinaryExpr.create(col("pay"), Operator.Multiply, PhysicalLiteralExpr.create(ScalarValue.Float64(2.0)))
    X = pp.WindowFunctionEx
    funcs = [X.create(WX.RowNumber), X(WX.Sum, col("rank"), FX.RowsBetween, start=-6, end=0), X(WX.Count, col("name"), FX.Rows), X(WX.Lag, col("id"), offset=2),
             X(WX.Lead, col("pay"), offset=1, default=ScalarValue.Float64(0.5)), X(WX.FirstValue, col("rank"), FX.RowsBetween, start=None, end=-1), X(WX.LastValue, expr, FX.Partition),
             X(WX.Ntile, buckets=4), X(WX.Avg, expr, FX.RowsBetween, start=-1, end=1)]
    part, order = [col("department_id")], [pp.PhysicalSortExpr(col("name"), descending=True)]
    plan = pp.PhysicalWindowPlanEx.create(scan, part, order, funcs)
    assert isinstance(plan, pp.PhysicalPlan) and plan.children() == [scan] and plan.partition_by == part and plan.order_by == order and plan.funcs == funcs
    fields = plan.schema()
    assert [f.name for f in fields] == ["id", "name", "department_id", "rank", "pay", "row_number()", "sum(rank)", "count(name)", "lag(id, 2)", "lead(pay, 1)", "first_value(rank)",
                                        f"last_value({expr!r})", "ntile(4)", f"avg({expr!r})"]
    # value functions: the argument's dtype, nullable; everything else as the first entry
    assert [(f.dtype, f.nullable) for f in fields[5:]] == [(DType.UINT64, False), (DType.FLOAT64, False), (DType.UINT64, False), (DType.INT64, True), (DType.FLOAT64, True), (DType.INT64, True),
                                                           (DType.FLOAT64, True), (DType.UINT64, False), (DType.FLOAT64, False)]
    assert fields[:5] == list(scan.schema())
    assert funcs[1].spec(3) == {"func": WX.Sum, "column": 3, "frame": FX.RowsBetween, "start": -6, "end": 0, "param": 1, "default": None}
    assert funcs[4].spec(4)["default"] == 0.5 and funcs[7].spec(None)["param"] == 4 and funcs[3].spec(0)["param"] == 2
    # Q6: no coercion of the default
    for bad in (ScalarValue.Int64(1), ScalarValue.UInt64(1), ScalarValue.Float64(None)):
        with pytest.raises(ErrorCode) as e:
            pp.PhysicalWindowPlanEx.create(scan, [], [], [X(WX.Lag, col("pay"), default=bad)]).schema()
        assert e.value.status == Status.IntervalError


class _StubTable:
    """a device table as a stub context sees it: its context and its column count"""

    def __init__(self, ctx, num_columns):
        self.ctx, self.num_columns = ctx, num_columns


class _StubContext:
    """the Context methods a window plan calls, recorded in `calls`; nothing is computed"""

    def __init__(self):
        self.calls = []

    def _table(self, name, num_columns, *args):
        self.calls.append((name,) + args)
        return _StubTable(self, num_columns)

    def expr_evaluate(self, table, nodes):
        return self._table("expr_evaluate", 1, table.num_columns)

    def append_columns(self, table, extra):
        return self._table("append_columns", table.num_columns + sum(t.num_columns for t in extra))

    def project(self, table, cols):
        return self._table("project", len(cols))

    def window(self, table, partition_by, order_by, funcs):
        return self._table("window", len(funcs), table.num_columns, partition_by, order_by, funcs)

    def window_ex(self, table, partition_by, order_by, funcs):
        return self._table("window_ex", len(funcs), table.num_columns, partition_by, order_by, funcs)


class _StubInput(pp.PhysicalPlan):
    """one batch of EMP's shape on a stub context"""

    def __init__(self, ctx):
        self.ctx = ctx

    def schema(self):
        return EMP

    def children(self):
        return []

    def execute(self):
        return [pp.DeviceRecordBatch(EMP, _StubTable(self.ctx, len(EMP)))]


def test_each_plan_reaches_its_own_entry_through_the_shared_body():
    key = PhysicalBinaryExpr.create(col("department_id"), Operator.Plus, PhysicalLiteralExpr.create(ScalarValue.Int64(1)))
    arg = PhysicalBinaryExpr.create(col("pay"), Operator.Multiply, PhysicalLiteralExpr.create(ScalarValue.Float64(2.0)))
    order = [pp.PhysicalSortExpr(col("name"), descending=True, nulls_first=False)]
    n = len(EMP)
    cases = (("window", pp.PhysicalWindowPlan, [pp.WindowFunction(W.Sum, arg, F.Rows), pp.WindowFunction(W.Rank), pp.WindowFunction(W.Max, col("id"))]),
             ("window_ex", pp.PhysicalWindowPlanEx, [pp.WindowFunctionEx(WX.Sum, arg, FX.Rows), pp.WindowFunctionEx(WX.Rank), pp.WindowFunctionEx(WX.Lag, col("id"), offset=3)]))
    for entry, plan_type, funcs in cases:
        ctx = _StubContext()
        (batch,) = plan_type.create(_StubInput(ctx), [key], order, funcs).execute()
        made = [c for c in ctx.calls if c[0] in ("window", "window_ex")]
        assert [c[0] for c in made] == [entry]  # its own entry, once, and not the other
        _, width, parts, keys, specs = made[0]
        # the key and the argument are temporary columns behind the input's: the call sees them, the batch that leaves does not
        assert width == n + 2 and parts == [n] and keys == [(1, True, False)]
        assert batch.table.num_columns == n + len(funcs) and [f.name for f in batch.fields] == [f.name for f in plan_type.create(_StubInput(ctx), [key], order, funcs).schema()]
        assert [c[0] for c in ctx.calls].count("expr_evaluate") == 2
        if entry == "window":  # how a function turns into a spec is the other difference
            assert specs == [(W.Sum, n + 1, F.Rows), (W.Rank, None, F.Range), (W.Max, 0, F.Range)]
        else:
            assert specs == [funcs[0].spec(n + 1), funcs[1].spec(None), funcs[2].spec(0)] and specs[2]["param"] == 3
    # a default of another dtype is refused before anything runs
    ctx = _StubContext()
    with pytest.raises(ErrorCode) as e:
        pp.PhysicalWindowPlanEx.create(_StubInput(ctx), [key], order, [pp.WindowFunctionEx(WX.Lag, col("pay"), default=ScalarValue.Int64(1))]).execute()
    assert e.value.status == Status.IntervalError and ctx.calls == []


def test_rewrite_keeps_the_node_and_rewrites_its_input():
    pred = PhysicalBinaryExpr.create(col("id"), Operator.Gt, PhysicalLiteralExpr.create(ScalarValue.Int64(0)))
    proj = pp.ProjectionPlan.create(pp.SelectionPlan.create(pp.ScanPlan.create(_Stub(EMP)), pred), EMP, [col(f.name) for f in EMP])
    funcs = [pp.WindowFunctionEx(WX.Ntile, buckets=2), pp.WindowFunctionEx(WX.Lag, col("id"))]
    win = pp.PhysicalWindowPlanEx.create(proj, [col("department_id")], [pp.PhysicalSortExpr(col("name"))], funcs)
    assert plan_shape(win) == ["PhysicalWindowPlanEx", "ProjectionPlan", "SelectionPlan", "ScanPlan"]
    out = rewrite(win)
    assert plan_shape(out) == ["PhysicalWindowPlanEx", "FusedSelectionProjectionPlan", "ScanPlan"]
    assert isinstance(out, pp.PhysicalWindowPlanEx) and out is not win and out.funcs == funcs and out.partition_by == win.partition_by and out.order_by == win.order_by
    assert plan_shape(win) == ["PhysicalWindowPlanEx", "ProjectionPlan", "SelectionPlan", "ScanPlan"]  # the input tree is left as it was
    assert plan_shape(rewrite(pp.PhysicalLimitPlan.create(win, 3))) == ["PhysicalLimitPlan", "PhysicalWindowPlanEx", "FusedSelectionProjectionPlan", "ScanPlan"]


# ----------------------------------------------------------------------------- the other mirrors
def test_cpp_mirror_has_the_plan_and_the_rewrite_arm():
    hpp = open(os.path.join(ROOT, "naive_query_engine_amd", "host", "naive_db.hpp")).read()
    assert "struct WindowFunctionEx" in hpp and "struct PhysicalWindowPlanEx : PhysicalPlan" in hpp and "nqe_window_execute_ex(" in hpp
    arm = hpp[hpp.index("inline PhysicalPlanRef rewrite("):]
    assert "std::dynamic_pointer_cast<PhysicalWindowPlanEx>(plan)" in arm and "PhysicalWindowPlanEx::create(rewrite(w->input)" in arm


def test_rust_shim_declares_the_entry_point_and_a_plan():
    path = os.path.join(ROOT, "integration", "rust", "gpu.rs")
    src = crs.strip_rust(open(path).read())
    assert "nqe_window_execute_ex" in crs.extern_functions(src) and "nqe_window_execute" in crs.extern_functions(src)
    assert "pub struct NqeWindowSpecEx { pub func: i32, pub column: i32, pub frame: i32, pub has_default: i32, pub start: i64, pub end: i64, pub param: i64, pub default_value: u64 }" in src
    assert "pub struct GpuWindowPlanEx" in src and "impl GpuExec for GpuWindowPlanEx" in src and "impl PhysicalPlan for GpuWindowPlanEx" in src
    assert "downcast_ref::<GpuWindowPlanEx>()" in src
    assert crs.check(path)[0] == []


# ----------------------------------------------------------------------------- golden queries
def test_golden_queries_match_the_model_and_sqlite():
    with open(os.path.join(GOLDEN, "window_ex_expected.json")) as f:
        qs = json.load(f)["queries"]
    assert [q["name"] for q in qs] == ["moving_sum_and_average_per_department", "lag_and_lead_with_and_without_default", "first_and_last_value_over_rows_between", "ntile_beside_a_rank"]
    assert {f["func"] for q in qs for f in q["funcs"]} >= {"Sum", "Avg", "Lag", "Lead", "FirstValue", "LastValue", "Ntile"}
    for q in qs:
        batch = read_csv(os.path.join(GOLDEN, q["table"] + ".csv"))
        names = [f.name for f in batch.fields]
        model = wx.window_ex(batch.columns, [names.index(c) for c in q["partition_by"]], [(names.index(k["column"]), k["descending"], k["nulls_first"]) for k in q["order_by"]],
                             wx.golden_funcs(q, names))
        assert q["columns"][:len(names)] == names and len(q["columns"]) == len(names) + len(q["funcs"])
        assert q["rows"] == wx.model_rows(batch.columns, model), q["name"]
        plan = wx.plan_from_golden(pp, pp.ScanPlan.create(_Stub(batch.fields)), q)
        assert [f.name for f in plan.schema()] == q["columns"]
        # the same query through SQLite: its rows in input order (every aggregate's frame holds a valid row, the values are small integers)
        db = sqlite3.connect(":memory:")
        db.execute(f"create table {q['table']} ({', '.join(names)})")
        db.executemany(f"insert into {q['table']} values ({', '.join('?' * len(names))})", [r[:len(names)] for r in q["rows"]])
        got = [list(r) for r in db.execute(q["sql"] + f" order by {names[0]}")]
        assert got == q["rows"], q["name"]
