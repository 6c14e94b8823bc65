"""CPU-only: outer hash joins (quirk Q19) in every host layer — the numpy / dict model of tests/outer_join_util.py by hand and against
pyarrow where the two definitions coincide (non-null keys), the golden queries, the header prototypes and their bindings, the Python
mirror and its rewrite arm, the C++ mirror and the Rust shim.  No device is touched: the stub sources below are never executed."""
import ctypes as C
import inspect
import json
import os
import re
import sys
from collections import Counter

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import outer_join_util as oju  # noqa: E402
from naive_query_engine_amd import Column, DType, Field, read_csv  # noqa: E402
from naive_query_engine_amd import physical_plan as pp  # noqa: E402
from naive_query_engine_amd.rewrite import plan_shape, rewrite  # noqa: E402
from tools import check_rust_shim as crs  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
RANK = [Field("id", DType.INT64), Field("rank_name", DType.UTF8)]
DEPT = [Field("id", DType.INT64), Field("department_name", DType.UTF8)]


def i64(a):
    return Column.from_numpy(np.asarray(a, dtype=np.int64))


class _Stub:
    def __init__(self, schema):
        self._schema = schema

    def schema(self):
        return self._schema

    def scan(self, projection):
        raise AssertionError("a stub source is never scanned here")


# ----------------------------------------------------------------------------- the model by hand
def test_model_duplicates_on_both_sides():
    b, p = i64([5, 7, 7, 9]), i64([7, 1, 9, 7])
    assert oju.probe_pairs(b, p, False) == ([1, 2, 3, 1, 2], [0, 0, 2, 3, 3])  # probe-row-major, ascending build row
    assert oju.probe_pairs(b, p, True) == ([1, 2, -1, 3, 1, 2], [0, 0, 1, 2, 3, 3])  # the miss in its place
    assert oju.unmatched_rows(b, [p]) == [0]
    assert oju.unmatched_rows(b, [i64([9]), i64([5])]) == [1, 2]  # matched in none of the batches


def test_model_no_match_all_match_and_empty_sides():
    b, p = i64([1, 2, 3]), i64([4, 5])
    assert oju.probe_pairs(b, p, False) == ([], []) and oju.probe_pairs(b, p, True) == ([-1, -1], [0, 1])
    assert oju.unmatched_rows(b, [p]) == [0, 1, 2]
    assert oju.probe_pairs(b, i64([3, 1, 2]), True) == ([2, 0, 1], [0, 1, 2]) and oju.unmatched_rows(b, [i64([3, 1, 2])]) == []
    e = i64([])
    assert oju.probe_pairs(e, p, True) == ([-1, -1], [0, 1]) and oju.probe_pairs(e, p, False) == ([], [])
    assert oju.probe_pairs(b, e, True) == ([], []) and oju.unmatched_rows(b, [e]) == [0, 1, 2] and oju.unmatched_rows(b, []) == [0, 1, 2]
    assert oju.unmatched_rows(e, [p]) == []


def test_model_a_null_key_slot_that_equals_a_real_key_matches():
    b = Column.from_numpy(np.array([5, 7, 9], dtype=np.int64), np.array([True, False, True]))  # the NULL's slot holds 7
    p = Column.from_numpy(np.array([7, 8, 5], dtype=np.int64), np.array([False, True, True]))
    assert oju.probe_pairs(b, p, True) == ([1, -1, 0], [0, 1, 2])  # validity is ignored on both sides (Q11 / Q19)
    assert oju.unmatched_rows(b, [p]) == [2]


def test_model_take_with_a_null_index():
    cols = [i64([10, 20]), Column.from_numpy(np.array([1.5, -0.0])), Column.from_numpy(np.array([True, True])), oju.utf8_column(["a", None])]
    out = oju.take_null(cols, [1, -1, 0])
    assert out[0].to_list() == [20, None, 10] and out[0].to_numpy().tolist() == [20, 0, 10]  # 0 under the NULL
    assert out[1].to_numpy().view(np.uint64).tolist() == [0x8000000000000000, 0, 0x3ff8000000000000]  # -0.0 survives bit for bit
    assert out[2].to_list() == [True, None, True] and out[2].to_numpy().tolist() == [True, False, True]
    assert out[3].to_list() == [None, None, "a"] and oju.utf8_raw(out[3]) == [b"", b"", b"a"]
    assert all(c.validity is not None for c in out)
    plain = oju.take_null(cols, [1, 0])
    assert [c.validity is not None for c in plain] == [False, False, False, True]  # a bitmap iff the source has NULLs or an index is -1
    nulls = oju.null_columns([DType.INT64, DType.BOOLEAN, DType.UTF8], 2)
    assert [c.to_list() for c in nulls] == [[None, None]] * 3 and all(c.validity is None for c in oju.null_columns([DType.INT64], 0))


# ----------------------------------------------------------------------------- the model against pyarrow
def _model_rows(left, lk, right_batches, rk, how):
    """the rows of a LEFT / RIGHT / FULL join as the operator emits them, all batches together"""
    rows = []
    for right in right_batches:
        rows += oju.rows_of(oju.outer_probe(left, lk, right, rk, how in ("right outer", "full outer")))
    if how in ("left outer", "full outer"):
        rows += oju.rows_of(oju.unmatched_batch(left, lk, [r[rk] for r in right_batches], [c.dtype for c in right_batches[0]]))
    return rows


def _to_arrow(col):
    import pyarrow as pa

    ty = {DType.INT64: pa.int64(), DType.UINT64: pa.uint64(), DType.FLOAT64: pa.uint64(), DType.BOOLEAN: pa.bool_(), DType.UTF8: pa.binary()}[col.dtype]
    return pa.array(oju.column_values(col), type=ty)  # (Float64 travels as its bit pattern: NaN payloads compare)


def _pyarrow_rows(left, lk, right, rk, how):
    import pyarrow as pa

    lt = pa.table({f"l{i}": _to_arrow(c) for i, c in enumerate(left)})
    rt = pa.table({f"r{i}": _to_arrow(c) for i, c in enumerate(right)})
    j = lt.join(rt, keys=f"l{lk}", right_keys=f"r{rk}", join_type=how, coalesce_keys=False)
    j = j.select([f"l{i}" for i in range(len(left))] + [f"r{i}" for i in range(len(right))])
    return [tuple(r) for r in zip(*[j.column(n).to_pylist() for n in j.column_names])]


@pytest.mark.parametrize("how", ["left outer", "right outer", "full outer"])
@pytest.mark.parametrize("kind", ["int", "uint", "utf8"])
def test_model_agrees_with_pyarrow_as_multisets(kind, how):
    pytest.importorskip("pyarrow")
    for seed in range(6):
        rng = np.random.default_rng(seed * 7 + len(kind) + len(how))
        n, m = int(rng.integers(0, 60)), int(rng.integers(0, 90))
        lk, rk = rng.integers(0, 25, n), rng.integers(5, 35, m)  # duplicates on both sides, misses on both sides; keys non-null
        if kind == "utf8":
            lkc, rkc = oju.utf8_column([f"k{v}" for v in lk]), oju.utf8_column([f"k{v}" for v in rk])
        else:
            dt = np.int64 if kind == "int" else np.uint64
            lkc, rkc = Column.from_numpy(lk.astype(dt)), Column.from_numpy(rk.astype(dt))
        left = [lkc, Column.from_numpy(rng.integers(-9, 9, n).astype(np.int64), rng.random(n) > 0.3), oju.utf8_column([None if v % 4 == 0 else "s%d" % v for v in range(n)])]
        right = [Column.from_numpy(rng.normal(0, 1, m)), rkc, Column.from_numpy(rng.random(m) < 0.5, rng.random(m) > 0.2)]
        cut = m // 2
        batches = [oju.take_null(right, np.arange(0, cut)), oju.take_null(right, np.arange(cut, m))]
        got = Counter(_model_rows(left, 0, batches, 1, how))
        assert got == Counter(_pyarrow_rows(left, 0, right, 1, how)), (kind, how, seed)


# ----------------------------------------------------------------------------- golden queries
def _golden():
    with open(os.path.join(GOLDEN, "outer_join_expected.json")) as f:
        return json.load(f)["queries"]


def _plain(rows):
    return [[v.decode() if isinstance(v, bytes) else v for v in r] for r in rows]


def test_golden_queries_match_model_and_pyarrow():
    qs = _golden()
    assert [(q["name"], q["join_type"]) for q in qs] == [("employee_left_join_rank", "Left"), ("rank_left_join_department", "Left"), ("rank_right_join_department", "Right")]
    for q in qs:
        lt, rt = read_csv(os.path.join(GOLDEN, q["left"] + ".csv")), read_csv(os.path.join(GOLDEN, q["right"] + ".csv"))
        assert [f.name for f in lt.fields] + [f.name for f in rt.fields] == q["columns"]
        li, ri = [f.name for f in lt.fields].index(q["left_key"]), [f.name for f in rt.fields].index(q["right_key"])
        batches = [_plain(oju.rows_of(oju.outer_probe(lt.columns, li, rt.columns, ri, q["join_type"] == "Right")))]
        if q["join_type"] == "Left":
            batches.append(_plain(oju.rows_of(oju.unmatched_batch(lt.columns, li, [rt.columns[ri]], [c.dtype for c in rt.columns]))))
        assert batches == q["batches"], q["name"]
        assert len(q["batches"]) == (2 if q["join_type"] == "Left" else 1)
        try:
            import pyarrow  # noqa: F401
        except ImportError:
            continue
        how = {"Left": "left outer", "Right": "right outer"}[q["join_type"]]
        exp = Counter(tuple(r) for b in q["batches"] for r in b)
        assert exp == Counter(tuple(r) for r in _plain(_pyarrow_rows(lt.columns, li, rt.columns, ri, how))), q["name"]
    assert qs[0]["batches"][1] == [] and qs[1]["batches"][1] == [[0, "master", None, None]] and qs[2]["batches"][0][-1] == [None, None, 3, "Human Resource"]


# ----------------------------------------------------------------------------- the C ABI
def test_header_declares_the_prototypes():
    hdr = open(os.path.join(ROOT, "include", "nqe.h")).read()
    ws = lambda s: re.sub(r"\s+", r"\\s*", re.escape(s).replace(r"\ ", " "))  # noqa: E731
    for proto in ["typedef struct nqe_join_marks nqe_join_marks;",
                  "nqe_status nqe_join_marks_create(nqe_ctx *ctx, const nqe_join_table *build, nqe_join_marks **out);",
                  "nqe_status nqe_join_marks_release(nqe_join_marks *marks);",
                  "#define NQE_JOIN_KEEP_PROBE 1u"]:
        assert re.search(ws(proto), hdr), proto
    assert re.search(r"nqe_status\s+nqe_hash_join_probe_outer\s*\(\s*nqe_ctx\s*\*\s*ctx\s*,\s*const nqe_join_table\s*\*\s*build\s*,\s*const nqe_table\s*\*\s*right\s*,\s*int32_t\s+right_key\s*,\s*"
                     r"uint32_t\s+flags\s*,\s*nqe_join_marks\s*\*\s*marks\s*(/\*.*?\*/)?\s*,\s*nqe_table\s*\*\*\s*out\s*\)\s*;", hdr)
    assert re.search(r"nqe_status\s+nqe_hash_join_unmatched_build\s*\(\s*nqe_ctx\s*\*\s*ctx\s*,\s*const nqe_join_table\s*\*\s*build\s*,\s*const nqe_join_marks\s*\*\s*marks\s*,\s*"
                     r"const int32_t\s*\*\s*right_dtypes\s*,\s*int32_t\s+num_right\s*,\s*nqe_table\s*\*\*\s*out\s*\)\s*;", hdr)
    assert "#define NQE_ABI_VERSION 1" in hdr and "Q19" in hdr


def test_bindings_match_the_header():
    from naive_query_engine_amd import capi

    for s in ("nqe_join_marks_create", "nqe_join_marks_release", "nqe_hash_join_probe_outer", "nqe_hash_join_unmatched_build"):
        assert s in capi.SYMBOLS
    L = capi.lib()
    vp, i32 = C.c_void_p, C.c_int32
    assert L.nqe_join_marks_create.argtypes == [vp, vp, C.POINTER(vp)] and L.nqe_join_marks_release.argtypes == [vp]
    assert L.nqe_hash_join_probe_outer.argtypes == [vp, vp, vp, i32, C.c_uint32, vp, C.POINTER(vp)]
    assert L.nqe_hash_join_unmatched_build.argtypes == [vp, vp, vp, C.POINTER(i32), i32, C.POINTER(vp)]
    assert all(f.restype is i32 for f in (L.nqe_join_marks_create, L.nqe_join_marks_release, L.nqe_hash_join_probe_outer, L.nqe_hash_join_unmatched_build))
    assert capi.JOIN_KEEP_PROBE == 1
    assert list(inspect.signature(capi.Context.join_marks).parameters) == ["self", "jt"]
    sig = inspect.signature(capi.Context.hash_join_probe_outer)
    assert list(sig.parameters) == ["self", "jt", "right", "right_key", "keep_probe", "marks"]
    assert sig.parameters["keep_probe"].default is False and sig.parameters["marks"].default is None
    assert list(inspect.signature(capi.Context.hash_join_unmatched_build).parameters) == ["self", "jt", "marks", "right_dtypes"]
    assert inspect.isclass(capi.JoinMarks)


# ----------------------------------------------------------------------------- the mirrors
def test_mirror_construction_schema_children():
    ls, rs = pp.ScanPlan.create(_Stub(RANK)), pp.ScanPlan.create(_Stub(DEPT))
    on = [(pp.ColumnRef(None, "id"), pp.ColumnRef(None, "id"))]
    assert list(inspect.signature(pp.HashOuterJoin.create).parameters) == ["left", "right", "on", "join_type", "schema"]
    plan = pp.HashOuterJoin.create(ls, rs, on, pp.JoinType.Left, RANK + DEPT)
    assert isinstance(plan, pp.PhysicalPlan) and not isinstance(plan, pp.HashJoin)
    assert plan.children() == [ls, rs] and plan.join_type == pp.JoinType.Left and plan.on == on
    assert [f.name for f in plan.schema()] == ["id", "rank_name", "id", "department_name"]
    assert [pp.JoinType.Inner, pp.JoinType.Left, pp.JoinType.Right, pp.JoinType.Cross] == [0, 1, 2, 3] and not hasattr(pp.JoinType, "Full")  # the reference's enum
    assert not hasattr(pp.HashOuterJoin.create(ls, rs, on, pp.JoinType.Right, RANK + DEPT), "_executions")  # no Q11 state
    assert hasattr(pp.HashJoin.create(ls, rs, on, pp.JoinType.Left, RANK + DEPT), "_executions")  # HashJoin itself is untouched


def test_rewrite_keeps_the_operator_with_rewritten_children():
    from naive_query_engine_amd import ColumnExpr, Operator, PhysicalBinaryExpr, PhysicalLiteralExpr, ScalarValue

    pred = PhysicalBinaryExpr.create(ColumnExpr.try_create("id", None), Operator.Gt, PhysicalLiteralExpr.create(ScalarValue.Int64(0)))
    proj = pp.ProjectionPlan.create(pp.SelectionPlan.create(pp.ScanPlan.create(_Stub(RANK)), pred), RANK, [ColumnExpr.try_create(f.name, None) for f in RANK])
    on = [(pp.ColumnRef(None, "id"), pp.ColumnRef(None, "id"))]
    tree = pp.HashOuterJoin.create(proj, pp.ScanPlan.create(_Stub(DEPT)), on, pp.JoinType.Right, RANK + DEPT)
    assert plan_shape(tree) == ["HashOuterJoin", "ProjectionPlan", "SelectionPlan", "ScanPlan", "ScanPlan"]
    out = rewrite(tree)
    assert plan_shape(out) == ["HashOuterJoin", "FusedSelectionProjectionPlan", "ScanPlan", "ScanPlan"]
    assert isinstance(out, pp.HashOuterJoin) and out is not tree and out.join_type == pp.JoinType.Right and out.on == on and out.schema() == tree.schema()
    assert plan_shape(rewrite(out)) == plan_shape(out)


def test_cpp_mirror_has_the_outer_join_and_the_rewrite_arm():
    hpp = open(os.path.join(ROOT, "naive_query_engine_amd", "host", "naive_db.hpp")).read()
    assert "struct HashOuterJoin : PhysicalPlan" in hpp
    for call in ("nqe_join_marks_create(", "nqe_join_marks_release(", "nqe_hash_join_probe_outer(", "nqe_hash_join_unmatched_build(", "NQE_JOIN_KEEP_PROBE"):
        assert call in hpp, call
    assert "std::dynamic_pointer_cast<HashOuterJoin>(plan)) return HashOuterJoin::create(rewrite(" in hpp
    assert os.path.exists(os.path.join(ROOT, "tests", "cpp", "test_outer_join.cpp"))


def test_rust_shim_declares_the_entry_points_and_an_outer_join():
    path = os.path.join(ROOT, "integration", "rust", "gpu.rs")
    src = crs.strip_rust(open(path).read())
    fns = crs.extern_functions(src)
    for s in ("nqe_join_marks_create", "nqe_join_marks_release", "nqe_hash_join_probe_outer", "nqe_hash_join_unmatched_build"):
        assert s in fns, s
    assert "pub struct GpuHashOuterJoin" in src and "impl GpuExec for GpuHashOuterJoin" in src and "impl PhysicalPlan for GpuHashOuterJoin" in src
    assert crs.check(path)[0] == []
