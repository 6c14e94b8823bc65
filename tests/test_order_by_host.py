"""CPU-only: ORDER BY (quirk Q18) in every host layer — the pure-Python model of tests/order_by_util.py against pyarrow where the two
definitions coincide, the golden queries, the Python mirror and its rewrite arm, the nqe_sort_key binding against the header, the C++
mirror and the Rust shim.  No device is touched: the stub sources below are never executed."""
import ctypes as C
import inspect
import json
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import order_by_util as obu  # noqa: E402
from naive_query_engine_amd import Column, ColumnExpr, DType, Field, Operator, PhysicalBinaryExpr, PhysicalLiteralExpr, ScalarValue, read_csv  # noqa: E402
from naive_query_engine_amd import physical_plan as pp  # noqa: E402
from naive_query_engine_amd.rewrite import plan_shape, rewrite  # noqa: E402
from tools import check_rust_shim as crs  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
EMP = [Field("id", DType.INT64), Field("name", DType.UTF8), Field("department_id", DType.INT64), Field("rank", DType.INT64)]


class _Stub:
    def __init__(self, schema):
        self._schema = schema

    def schema(self):
        return self._schema

    def scan(self, projection):
        raise AssertionError("a stub source is never scanned here")


# ----------------------------------------------------------------------------- the model by hand
def test_model_on_the_cases_the_issue_spells_out():
    s = obu.utf8_column([b"b", b"ab", b"a\0", b"a", b""])
    assert obu.sort_indices([s], [0]) == [4, 3, 2, 1, 0]  # "" < "a" < "a\0" < "ab" < "b"
    assert obu.sort_indices([s], [(0, True)]) == [0, 1, 2, 3, 4]
    f = Column.from_numpy(np.array([np.nan, np.inf, -0.0, 0.0, -np.inf, -np.nan, 1.0]))
    assert obu.sort_indices([f], [0]) == [4, 2, 3, 6, 1, 0, 5]  # the zeros tie, the NaNs tie above +inf: input order inside each
    assert obu.sort_indices([f], [(0, True)]) == [0, 5, 1, 6, 2, 3, 4]  # NaN first when descending
    k = Column.from_list([3, None, 1, None, 2], DType.INT64)
    assert obu.sort_indices([k], [(0, False, True)]) == [1, 3, 2, 4, 0]
    assert obu.sort_indices([k], [(0, False, False)]) == [2, 4, 0, 1, 3]
    assert obu.sort_indices([k], [(0, True, True)]) == [1, 3, 0, 4, 2]  # NULLs stay first, the values reverse
    assert obu.sort_indices([k], [(0, True, False)]) == [0, 4, 2, 1, 3]
    u = Column.from_numpy(np.array([2 ** 63 + 1, 1, 2 ** 64 - 1], dtype=np.uint64))
    i = Column.from_numpy(np.array([-1, np.iinfo(np.int64).min, np.iinfo(np.int64).max], dtype=np.int64))
    b = Column.from_numpy(np.array([True, False, True]))
    assert obu.sort_indices([u], [0]) == [1, 0, 2] and obu.sort_indices([i], [0]) == [1, 0, 2] and obu.sort_indices([b], [0]) == [1, 0, 2]
    two = [Column.from_numpy(np.array([1, 0, 1, 0], dtype=np.int64)), Column.from_numpy(np.array([5, 7, 4, 7], dtype=np.int64))]
    assert obu.sort_indices(two, [0, (1, True)]) == [1, 3, 0, 2]  # first key most significant; the tie (0, 7) keeps input order
    assert obu.sort_indices(two, [0], fetch=3) == [1, 3, 0] and obu.sort_indices(two, [0], fetch=0) == [] and obu.sort_indices(two, [0], fetch=9) == [1, 3, 0, 2]


# ----------------------------------------------------------------------------- the model against pyarrow
def _to_arrow(col):
    import pyarrow as pa

    vals = obu.column_values(col)
    ty = {DType.INT64: pa.int64(), DType.UINT64: pa.uint64(), DType.FLOAT64: pa.float64(), DType.BOOLEAN: pa.bool_(), DType.UTF8: pa.binary()}[col.dtype]
    return pa.array(vals, type=ty)


def _pyarrow_indices(cols, keys):
    """pyarrow.compute.sort_indices takes ONE null placement for all keys: the callers below use one"""
    import pyarrow as pa
    import pyarrow.compute as pc

    keys = obu.normalise_keys(keys)
    placements = {nf for _, _, nf in keys}
    assert len(placements) == 1
    # a column named twice as a key: pyarrow wants distinct names, so every key gets its own copy of the column
    tbl = pa.table({f"k{j}": _to_arrow(cols[c]) for j, (c, _, _) in enumerate(keys)})
    opts = [(f"k{j}", "descending" if d else "ascending") for j, (_, d, _) in enumerate(keys)]
    return pc.sort_indices(tbl, sort_keys=opts, null_placement="at_start" if placements.pop() else "at_end").to_pylist()


@pytest.mark.parametrize("descending", [False, True])
@pytest.mark.parametrize("nulls_first", [False, True])
@pytest.mark.parametrize("dtype", obu.ALL_DTYPES)
def test_model_agrees_with_pyarrow_per_dtype(dtype, descending, nulls_first):
    pytest.importorskip("pyarrow")
    rng = np.random.default_rng(int(dtype) * 4 + descending * 2 + nulls_first)
    # pyarrow places NaN together with the NULLs (behind the numbers and in front of the NULLs with at_end, the mirror image with
    # at_start), so with NaNs present the two definitions agree only where "greater than +inf" lands in the same place: (ascending,
    # nulls last) and (descending, nulls first).  The other two combinations are compared on NaN-free data.
    nan_ok = descending == nulls_first
    for distinct in (None, 5):
        col = obu.random_column(rng, dtype, 300, True, distinct)
        if dtype == DType.FLOAT64 and not nan_ok:
            v = col.to_numpy().copy()
            v[np.isnan(v)] = 7.0
            col = Column(DType.FLOAT64, col.length, v, col.validity)
        keys = [(0, descending, nulls_first)]
        assert obu.sort_indices([col], keys) == _pyarrow_indices([col], keys)  # stable ties, the zeros tie, byte order


def test_model_agrees_with_pyarrow_on_several_keys():
    pytest.importorskip("pyarrow")
    for seed in range(12):
        rng = np.random.default_rng(100 + seed)
        cols = [obu.random_column(rng, dt, 400, bool(seed & 1), 5) for dt in (DType.UTF8, DType.INT64, DType.BOOLEAN, DType.UINT64)]
        nf = bool(seed & 2)
        keys = [(int(c), bool(rng.random() < 0.5), nf) for c in rng.integers(0, 4, 3)]  # (a column may be named twice)
        assert obu.sort_indices(cols, keys) == _pyarrow_indices(cols, keys), (seed, keys)


# ----------------------------------------------------------------------------- golden queries
def _golden():
    with open(os.path.join(GOLDEN, "order_by_expected.json")) as f:
        return json.load(f)["queries"]


def _golden_input(q):
    emp = read_csv(os.path.join(GOLDEN, "employee.csv"))
    if "aggregate_rows" not in q:
        assert [f.name for f in emp.fields] == q["columns"]
        return emp.columns
    # the aggregate's rows by hand: first-appearance order of the group key
    names = [f.name for f in emp.fields]
    key = emp.columns[names.index(q["group_by"])].to_numpy()
    groups = list(dict.fromkeys(key.tolist()))
    fn = {"sum": np.sum, "max": np.max}
    rows = [[float(fn[f](emp.columns[names.index(c)].to_numpy()[key == g])) for f, c in q["aggregates"]] for g in groups]
    assert rows == q["aggregate_rows"]
    return [Column.from_numpy(np.array([r[j] for r in rows], dtype=np.float64)) for j in range(len(q["aggregates"]))]


def _rows(cols):
    vals = [[v.decode() if isinstance(v, bytes) else v for v in obu.column_values(c)] for c in cols]
    return [list(r) for r in zip(*vals)]


def test_golden_queries_cover_the_four_shapes_and_match_model_and_pyarrow():
    qs = _golden()
    assert [q["name"] for q in qs] == ["utf8_key", "department_desc_rank_asc", "group_by_then_order_by_aggregate", "order_by_limit_3"]
    assert qs[3]["fetch"] == 3 and len(qs[3]["rows"]) == 3
    for q in qs:
        cols = _golden_input(q)
        keys = [(q["columns"].index(k["column"]), k["descending"], k["nulls_first"]) for k in q["keys"]]
        assert _rows(obu.order_by(cols, keys, q["fetch"])) == q["rows"], q["name"]
        try:
            import pyarrow  # noqa: F401
        except ImportError:
            continue
        idx = _pyarrow_indices(cols, keys)
        assert _rows(obu.take(cols, idx if q["fetch"] is None else idx[:q["fetch"]])) == q["rows"], q["name"]


# ----------------------------------------------------------------------------- the mirrors
def test_mirror_construction_schema_children():
    scan = pp.ScanPlan.create(_Stub(EMP))
    assert list(inspect.signature(pp.PhysicalSortExpr.__init__).parameters) == ["self", "expr", "descending", "nulls_first"]
    assert list(inspect.signature(pp.PhysicalSortPlan.__init__).parameters) == ["self", "input", "sort_exprs", "fetch"]
    e = pp.PhysicalSortExpr(ColumnExpr.try_create("name", None))
    assert (e.descending, e.nulls_first) == (False, True)  # arrow-rs' SortOptions::default()
    d = pp.PhysicalSortExpr.create(ColumnExpr.try_create("rank", None), descending=True, nulls_first=False)
    assert (d.descending, d.nulls_first) == (True, False)
    plan = pp.PhysicalSortPlan.create(scan, [e, d])
    assert isinstance(plan, pp.PhysicalPlan) and plan.fetch is None and plan.sort_exprs == [e, d]
    assert plan.schema() is scan.schema() and [f.name for f in plan.schema()] == ["id", "name", "department_id", "rank"]
    assert plan.children() == [scan]
    assert pp.PhysicalSortPlan(scan, [e], fetch=3).fetch == 3


def test_rewrite_folds_a_limit_over_a_sort_into_fetch():
    pred = PhysicalBinaryExpr.create(ColumnExpr.try_create("id", None), Operator.Gt, PhysicalLiteralExpr.create(ScalarValue.Int64(0)))
    keys = [pp.PhysicalSortExpr(ColumnExpr.try_create("name", None), descending=True)]
    proj = pp.ProjectionPlan.create(pp.SelectionPlan.create(pp.ScanPlan.create(_Stub(EMP)), pred), EMP, [ColumnExpr.try_create(f.name, None) for f in EMP])
    srt = pp.PhysicalSortPlan.create(proj, keys)
    tree = pp.PhysicalLimitPlan.create(srt, 3)
    assert plan_shape(tree) == ["PhysicalLimitPlan", "PhysicalSortPlan", "ProjectionPlan", "SelectionPlan", "ScanPlan"]
    out = rewrite(tree)
    assert plan_shape(out) == ["PhysicalSortPlan", "FusedSelectionProjectionPlan", "ScanPlan"]
    assert isinstance(out, pp.PhysicalSortPlan) and out.fetch == 3 and out.sort_exprs == keys and out is not srt
    assert srt.fetch is None  # the input tree is left as it was
    assert plan_shape(rewrite(out)) == plan_shape(out) and rewrite(out).fetch == 3
    # a sort that already fetches fewer rows keeps its own count; a bare sort keeps its operator with rewritten children
    assert rewrite(pp.PhysicalLimitPlan.create(pp.PhysicalSortPlan.create(proj, keys, fetch=2), 3)).fetch == 2
    bare = rewrite(srt)
    assert plan_shape(bare) == ["PhysicalSortPlan", "FusedSelectionProjectionPlan", "ScanPlan"] and bare.fetch is None
    # an offset over a sort stays unfused, and so does a limit over that offset
    off = pp.PhysicalLimitPlan.create(pp.PhysicalOffsetPlan.create(srt, 1), 2)
    assert plan_shape(rewrite(off)) == ["PhysicalLimitPlan", "PhysicalOffsetPlan", "PhysicalSortPlan", "FusedSelectionProjectionPlan", "ScanPlan"]
    assert rewrite(off).input.input.fetch is None


# ----------------------------------------------------------------------------- the C ABI
def test_header_declares_the_struct_and_the_entry_point():
    hdr = open(os.path.join(ROOT, "include", "nqe.h")).read()
    assert re.search(r"nqe_status\s+nqe_sort_execute\s*\(\s*nqe_ctx\s*\*\s*ctx\s*,\s*const nqe_table\s*\*\s*in\s*,\s*const nqe_sort_key\s*\*\s*keys\s*,\s*"
                     r"int32_t\s+num_keys\s*,\s*int64_t\s+fetch\s*(/\*.*?\*/)?\s*,\s*nqe_table\s*\*\*\s*out\s*\)\s*;", hdr)
    assert "#define NQE_ABI_VERSION 1" in hdr


def test_sort_key_binding_matches_the_header_struct():
    from naive_query_engine_amd import capi

    hdr = open(os.path.join(ROOT, "include", "nqe.h")).read()
    m = re.search(r"typedef struct nqe_sort_key\s*\{(.*?)\}\s*nqe_sort_key\s*;", hdr, flags=re.S)
    assert m
    fields = re.findall(r"(\w+)\s+(\w+)\s*;", m.group(1))
    assert fields == [("int32_t", "column"), ("int32_t", "descending"), ("int32_t", "nulls_first")]
    assert [(n, t) for n, t in capi.NqeSortKey._fields_] == [(n, C.c_int32) for _, n in fields]
    assert C.sizeof(capi.NqeSortKey) == 12 and [getattr(capi.NqeSortKey, n).offset for _, n in fields] == [0, 4, 8]
    assert "nqe_sort_execute" in capi.SYMBOLS
    fn = capi.lib().nqe_sort_execute
    assert fn.restype is C.c_int32 and len(fn.argtypes) == 6 and fn.argtypes[3] is C.c_int32 and fn.argtypes[4] is C.c_int64
    assert list(inspect.signature(capi.Context.order_by).parameters) == ["self", "table", "keys", "fetch"]
    assert inspect.signature(capi.Context.order_by).parameters["fetch"].default is None


# ----------------------------------------------------------------------------- the other mirrors
def test_cpp_mirror_has_the_sort_plan_and_the_rewrite_arm():
    hpp = open(os.path.join(ROOT, "naive_query_engine_amd", "host", "naive_db.hpp")).read()
    assert "struct PhysicalSortExpr" in hpp and "struct PhysicalSortPlan : PhysicalPlan" in hpp
    assert "nqe_sort_execute(" in hpp
    arm = hpp[hpp.index("std::dynamic_pointer_cast<PhysicalLimitPlan>(plan)"):]
    assert "std::dynamic_pointer_cast<PhysicalSortPlan>(l->input)" in arm[:400]


def test_rust_shim_declares_the_entry_point_and_a_sort_plan():
    path = os.path.join(ROOT, "integration", "rust", "gpu.rs")
    src = crs.strip_rust(open(path).read())
    assert "nqe_sort_execute" in crs.extern_functions(src)
    assert "pub struct NqeSortKey { pub column: i32, pub descending: i32, pub nulls_first: i32 }" in src
    assert "pub struct GpuSortPlan" in src and "impl GpuExec for GpuSortPlan" in src and "impl PhysicalPlan for GpuSortPlan" in src
    assert crs.check(path)[0] == []
