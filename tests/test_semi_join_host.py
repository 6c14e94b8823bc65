"""CPU-only: semi and anti hash joins (quirk Q22) in every host layer — the numpy / dict model of tests/semi_join_util.py by hand and
against pyarrow where the two definitions coincide (non-null keys), the golden queries, the header prototypes and their bindings, the
Python mirror and its rewrite arm, the C++ mirror and the Rust shim.  No device is touched: the stub sources below are never executed."""
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

import outer_join_util as oju  # noqa: E402
import semi_join_util as sju  # noqa: E402
from naive_query_engine_amd import Column, DType, Field, read_csv  # noqa: E402
from naive_query_engine_amd import physical_plan as pp  # noqa: E402
from naive_query_engine_amd.rewrite import plan_shape, rewrite  # noqa: E402
from tools import check_rust_shim as crs  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
RANK = [Field("id", DType.INT64), Field("rank_name", DType.UTF8)]
EMP = [Field("id", DType.INT64), Field("name", DType.UTF8), Field("department_id", DType.INT64), Field("rank", DType.INT64)]
i64 = sju.i64


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
    assert sju.semi_rows(b, p) == [0, 2, 3]  # each probe row once, although 7 has two partners
    assert sju.semi_rows(b, p, anti=True) == [1]
    assert sju.marked_rows(b, [p]) == [1, 2, 3] and sju.marked_rows(b, [p], anti=True) == [0]  # both rows of the key 7
    assert sju.marked_rows(b, [i64([9]), i64([5])]) == [0, 3] and sju.marked_rows(b, [i64([9]), i64([5])], anti=True) == [1, 2]


def test_model_no_match_all_match_and_empty_sides():
    b, p = i64([1, 2, 3]), i64([4, 5])
    assert sju.semi_rows(b, p) == [] and sju.semi_rows(b, p, anti=True) == [0, 1]
    assert sju.marked_rows(b, [p]) == [] and sju.marked_rows(b, [p], anti=True) == [0, 1, 2]
    assert sju.semi_rows(b, i64([3, 1, 2])) == [0, 1, 2] and sju.semi_rows(b, i64([3, 1, 2]), anti=True) == []
    assert sju.marked_rows(b, [i64([3, 1, 2])], anti=True) == []
    e = i64([])
    assert sju.semi_rows(e, p) == [] and sju.semi_rows(e, p, anti=True) == [0, 1]
    assert sju.semi_rows(b, e) == [] and sju.semi_rows(b, e, anti=True) == []
    assert sju.marked_rows(b, [e]) == [] and sju.marked_rows(b, [], anti=True) == [0, 1, 2] and sju.marked_rows(e, [p], anti=True) == []


def test_model_a_null_whose_raw_slot_equals_a_build_key():
    b = i64([5, 7, 9])
    p = Column.from_numpy(np.array([7, 8, 5], dtype=np.int64), np.array([False, True, True]))  # the NULL's slot holds 7
    assert sju.semi_rows(b, p) == [0, 2] and sju.semi_rows(b, p, anti=True) == [1]  # validity is ignored (Q11)
    assert sju.semi_rows(b, p, null_unmatched=True) == [2] and sju.semi_rows(b, p, anti=True, null_unmatched=True) == [0, 1]
    assert sju.marked_rows(b, [p]) == [0, 1] and sju.marked_rows(b, [p], null_unmatched=True) == [0]  # the NULL row sets no mark
    bn = Column.from_numpy(np.array([5, 7], dtype=np.int64), np.array([True, False]))
    assert sju.semi_rows(bn, i64([7])) == [0]  # a NULL on the build side still matches by its slot: only the probe side has the flag


def test_model_tuples_match_at_every_position():
    b = [i64([1, 1, 2]), oju.utf8_column(["a", "b", "a"])]
    p = [i64([1, 2, 2, 1]), oju.utf8_column(["b", "b", "a", "c"])]
    assert sju.semi_rows(b, p) == [0, 2] and sju.semi_rows(b, p, anti=True) == [1, 3]
    assert sju.marked_rows(b, [p]) == [1, 2] and sju.marked_rows(b, [p], anti=True) == [0]
    pn = [Column.from_numpy(np.array([1, 2], dtype=np.int64), np.array([True, False])), oju.utf8_column(["b", "a"])]
    assert sju.semi_rows(b, pn) == [0, 1] and sju.semi_rows(b, pn, null_unmatched=True) == [0]  # a NULL at ANY position


def test_model_output_is_the_compaction_of_the_right_columns():
    right = [i64([10, 20, 30]), Column.from_numpy(np.array([1.5, -0.0, 2.0]), np.array([True, True, False])), oju.utf8_column(["a", None, "c"]),
             Column.from_numpy(np.array([True, False, True]))]
    out = sju.probe_semi(right, i64([7, 8, 7]), i64([7]))
    assert [c.to_list() for c in out] == [[10, 30], [1.5, None], ["a", "c"], [True, True]]
    assert [c.validity is not None for c in out] == [False, True, True, False]
    out = sju.probe_semi(right, i64([7, 8, 7]), i64([7]), anti=True)
    assert out[1].to_numpy().view(np.uint64).tolist() == [0x8000000000000000] and out[2].to_list() == [None]


# ----------------------------------------------------------------------------- the model against pyarrow
def _to_arrow(col):
    import pyarrow as pa

    ty = {DType.INT64: pa.int64(), DType.UINT64: pa.uint64(), DType.FLOAT64: pa.uint64(), DType.BOOLEAN: pa.bool_(), DType.UTF8: pa.binary()}[col.dtype]
    return pa.array(oju.column_values(col), type=ty)  # (Float64 travels as its bit pattern: NaN payloads compare)


def _pyarrow_rows(left, lks, right, rks, how):
    """the rows pyarrow keeps, sorted by the row-number column that each side carries last"""
    import pyarrow as pa

    lt = pa.table({f"l{i}": _to_arrow(c) for i, c in enumerate(left)})
    rt = pa.table({f"r{i}": _to_arrow(c) for i, c in enumerate(right)})
    j = lt.join(rt, keys=[f"l{k}" for k in lks], right_keys=[f"r{k}" for k in rks], join_type=how)
    rows = [tuple(r) for r in zip(*[j.column(n).to_pylist() for n in j.column_names])]
    return sorted(rows, key=lambda r: r[-1])


@pytest.mark.parametrize("how", ["right semi", "right anti", "left semi", "left anti"])
@pytest.mark.parametrize("kind", ["int", "uint", "utf8", "pair"])
def test_model_agrees_with_pyarrow(kind, how):
    pytest.importorskip("pyarrow")
    for seed in range(6):
        rng = np.random.default_rng(seed * 11 + len(kind) + len(how))
        n, m = int(rng.integers(0, 60)), int(rng.integers(0, 90))
        lk, rk = rng.integers(0, 25, n), rng.integers(5, 35, m)  # duplicates on both sides, misses on both sides; keys non-null
        if kind == "utf8":
            lkc, rkc = [oju.utf8_column([f"k{v}" for v in lk])], [oju.utf8_column([f"k{v}" for v in rk])]
        elif kind == "pair":
            lkc = [i64(lk // 5), oju.utf8_column([f"k{v % 5}" for v in lk])]
            rkc = [i64(rk // 5), oju.utf8_column([f"k{v % 5}" for v in rk])]
        else:
            dt = np.int64 if kind == "int" else np.uint64
            lkc, rkc = [Column.from_numpy(lk.astype(dt))], [Column.from_numpy(rk.astype(dt))]
        left = lkc + [Column.from_numpy(rng.integers(-9, 9, n).astype(np.int64), rng.random(n) > 0.3), i64(np.arange(n))]
        right = [Column.from_numpy(rng.random(m) < 0.5, rng.random(m) > 0.2)] + rkc + [i64(np.arange(m))]
        lks, rks = list(range(len(lkc))), list(range(1, 1 + len(rkc)))
        cut = m // 2
        batches = [oju.take_null(right, np.arange(0, cut)), oju.take_null(right, np.arange(cut, m))]
        anti = how.endswith("anti")
        if how.startswith("right"):  # the probe side is kept: one batch per probe batch, probe order
            got = []
            for b in batches:
                got += oju.rows_of(sju.probe_semi(b, [b[k] for k in rks], lkc, anti))
        else:
            got = oju.rows_of(sju.take_rows(left, sju.marked_rows(lkc, [[b[k] for k in rks] for b in batches], anti)))
        assert got == _pyarrow_rows(left, lks, right, rks, how), (kind, how, seed)


# ----------------------------------------------------------------------------- golden queries
def _golden():
    with open(os.path.join(GOLDEN, "semi_join_expected.json")) as f:
        return json.load(f)["queries"]


def _plain(rows):
    return [[v.decode() if isinstance(v, bytes) else v for v in r] for r in rows]


def golden_batches(q):
    """the output batches of one golden query, from the model"""
    lt, rt = read_csv(os.path.join(GOLDEN, q["left"] + ".csv")), read_csv(os.path.join(GOLDEN, q["right"] + ".csv"))
    lnames, rnames = [f.name for f in lt.fields], [f.name for f in rt.fields]
    bk = [lt.columns[lnames.index(k)] for k in q["left_keys"]]
    pk = [rt.columns[rnames.index(k)] for k in q["right_keys"]]
    anti = q["semi_type"].endswith("Anti")
    if q["semi_type"].startswith("Probe"):
        return rnames, [_plain(oju.rows_of(sju.probe_semi(rt.columns, pk, bk, anti)))]
    return lnames, [_plain(oju.rows_of(sju.take_rows(lt.columns, sju.marked_rows(bk, [pk], anti))))]


def test_golden_queries_match_the_model():
    qs = _golden()
    assert [q["name"] for q in qs] == ["employees_whose_department_exists", "employees_whose_department_does_not_exist", "ranks_no_employee_holds",
                                       "ranks_no_employee_holds_build_side", "ranks_some_employee_holds_build_side", "employees_whose_id_is_a_department_id",
                                       "employees_whose_id_is_no_department_id", "ranks_whose_id_is_no_employee_id_build_side", "departments_whose_id_is_no_rank_held_build_side",
                                       "employees_in_employee_on_id_and_name", "ranks_without_employee_on_id_and_name", "ranks_with_employee_on_id_and_name_build_side"]
    for q in qs:
        columns, batches = golden_batches(q)
        assert columns == q["columns"] and batches == q["batches"] and len(batches) == 1, q["name"]
    by = {q["name"]: q["batches"][0] for q in qs}
    assert [r[0] for r in by["employees_whose_department_exists"]] == [1, 2, 3, 4, 5] and by["employees_whose_department_does_not_exist"] == []
    assert by["ranks_no_employee_holds"] == [] == by["ranks_no_employee_holds_build_side"]  # every rank of rank.csv is held
    assert by["ranks_some_employee_holds_build_side"] == [[0, "master"], [1, "diamond"], [2, "grandmaster"]]  # each once: ranks 0 and 1 have two holders
    assert [r[0] for r in by["employees_whose_id_is_a_department_id"]] == [1, 2, 3] and [r[:2] for r in by["employees_whose_id_is_no_department_id"]] == [[4, "jack"], [5, "mike"]]
    assert by["ranks_whose_id_is_no_employee_id_build_side"] == [[0, "master"]] and by["departments_whose_id_is_no_rank_held_build_side"] == [[3, "Human Resource"]]
    assert len(by["employees_in_employee_on_id_and_name"]) == 5 and len(by["ranks_without_employee_on_id_and_name"]) == 3
    assert by["ranks_with_employee_on_id_and_name_build_side"] == []


# ----------------------------------------------------------------------------- the C ABI
def test_header_declares_the_prototypes():
    hdr = open(os.path.join(ROOT, "include", "nqe.h")).read()
    assert re.search(r"#define\s+NQE_SEMI_ANTI\s+1u", hdr) and re.search(r"#define\s+NQE_SEMI_NULL_KEY_UNMATCHED\s+2u", hdr)
    c = r"\s*(/\*.*?\*/)?\s*"
    assert re.search(r"nqe_status\s+nqe_hash_join_probe_semi\s*\(\s*nqe_ctx\s*\*\s*ctx\s*,\s*const nqe_join_table\s*\*\s*build\s*,\s*const nqe_table\s*\*\s*right\s*,\s*"
                     r"const int32_t\s*\*\s*right_keys\s*,\s*int32_t\s+num_keys\s*,\s*uint32_t\s+flags\s*,\s*nqe_join_marks\s*\*\s*marks" + c + r",\s*nqe_table\s*\*\*\s*out" + c + r"\)\s*;", hdr)
    assert re.search(r"nqe_status\s+nqe_hash_join_marked_build\s*\(\s*nqe_ctx\s*\*\s*ctx\s*,\s*const nqe_join_table\s*\*\s*build\s*,\s*const nqe_join_marks\s*\*\s*marks\s*,\s*"
                     r"uint32_t\s+flags" + c + r",\s*nqe_table\s*\*\*\s*out\s*\)\s*;", hdr)
    assert "#define NQE_ABI_VERSION 1" in hdr and "Q22" in hdr and "NOT IN" in hdr  # the three-valued rule is named as out of scope


def test_bindings_match_the_header():
    from naive_query_engine_amd import capi

    assert "nqe_hash_join_probe_semi" in capi.SYMBOLS and "nqe_hash_join_marked_build" in capi.SYMBOLS
    L = capi.lib()
    vp, i32 = C.c_void_p, C.c_int32
    assert L.nqe_hash_join_probe_semi.argtypes == [vp, vp, vp, C.POINTER(i32), i32, C.c_uint32, vp, C.POINTER(vp)]
    assert L.nqe_hash_join_marked_build.argtypes == [vp, vp, vp, C.c_uint32, C.POINTER(vp)]
    assert L.nqe_hash_join_probe_semi.restype is i32 and L.nqe_hash_join_marked_build.restype is i32
    assert (capi.SEMI_ANTI, capi.SEMI_NULL_KEY_UNMATCHED) == (1, 2)
    sig = inspect.signature(capi.Context.hash_join_probe_semi)
    assert list(sig.parameters) == ["self", "jt", "right", "right_keys", "anti", "null_key_unmatched", "marks", "want_out", "flags"]
    assert sig.parameters["anti"].default is False and sig.parameters["null_key_unmatched"].default is False and sig.parameters["marks"].default is None
    assert sig.parameters["want_out"].default is True
    assert list(inspect.signature(capi.Context.hash_join_marked_build).parameters) == ["self", "jt", "marks", "anti", "flags"]


# ----------------------------------------------------------------------------- the mirrors
def test_mirror_construction_schema_children():
    ls, rs = pp.ScanPlan.create(_Stub(RANK)), pp.ScanPlan.create(_Stub(EMP))
    on = [(pp.ColumnRef(None, "id"), pp.ColumnRef(None, "rank")), (pp.ColumnRef(None, "rank_name"), pp.ColumnRef(None, "name"))]
    assert list(inspect.signature(pp.HashSemiJoin.create).parameters) == ["left", "right", "on", "semi_type", "schema", "null_key_unmatched"]
    assert list(inspect.signature(pp.HashSemiJoin.__init__).parameters) == ["self", "left", "right", "on", "semi_type", "schema", "null_key_unmatched"]
    assert inspect.signature(pp.HashSemiJoin.create).parameters["null_key_unmatched"].default is False
    T = pp.SemiJoinType
    assert [T.ProbeSemi, T.ProbeAnti, T.BuildSemi, T.BuildAnti] == [0, 1, 2, 3]
    plan = pp.HashSemiJoin.create(ls, rs, on, T.ProbeAnti, EMP)
    assert isinstance(plan, pp.PhysicalPlan) and not isinstance(plan, (pp.HashJoin, pp.MultiKeyHashJoin))
    assert plan.children() == [ls, rs] and plan.semi_type == T.ProbeAnti and plan.on == on and plan.null_key_unmatched is False
    assert [f.name for f in plan.schema()] == ["id", "name", "department_id", "rank"]  # the kept side's schema: the probe side
    build = pp.HashSemiJoin(ls, rs, on, T.BuildSemi, RANK, null_key_unmatched=True)
    assert [f.name for f in build.schema()] == ["id", "rank_name"] and build.null_key_unmatched is True
    assert not hasattr(plan, "_executions")  # no Q11 state
    assert not hasattr(pp.JoinType, "Semi") and [pp.JoinType.Inner, pp.JoinType.Left, pp.JoinType.Right, pp.JoinType.Cross] == [0, 1, 2, 3]  # the reference's enum stays


def test_rewrite_keeps_the_operator_with_rewritten_children():
    from naive_query_engine_amd import ColumnExpr, Operator, PhysicalBinaryExpr, PhysicalLiteralExpr, ScalarValue

    pred = PhysicalBinaryExpr.create(ColumnExpr.try_create("id", None), Operator.Gt, PhysicalLiteralExpr.create(ScalarValue.Int64(0)))
    proj = pp.ProjectionPlan.create(pp.SelectionPlan.create(pp.ScanPlan.create(_Stub(RANK)), pred), RANK, [ColumnExpr.try_create(f.name, None) for f in RANK])
    on = [(pp.ColumnRef(None, "id"), pp.ColumnRef(None, "rank"))]
    tree = pp.HashSemiJoin.create(proj, pp.ScanPlan.create(_Stub(EMP)), on, pp.SemiJoinType.BuildAnti, RANK, null_key_unmatched=True)
    assert plan_shape(tree) == ["HashSemiJoin", "ProjectionPlan", "SelectionPlan", "ScanPlan", "ScanPlan"]
    out = rewrite(tree)
    assert plan_shape(out) == ["HashSemiJoin", "FusedSelectionProjectionPlan", "ScanPlan", "ScanPlan"]
    assert isinstance(out, pp.HashSemiJoin) and out is not tree and out.semi_type == pp.SemiJoinType.BuildAnti and out.on == on and out.schema() == tree.schema()
    assert out.null_key_unmatched is True
    assert plan_shape(rewrite(out)) == plan_shape(out)


def test_cpp_mirror_has_the_semi_join_and_the_rewrite_arm():
    hpp = open(os.path.join(ROOT, "naive_query_engine_amd", "host", "naive_db.hpp")).read()
    assert "struct HashSemiJoin : PhysicalPlan" in hpp and "enum class SemiJoinType { ProbeSemi, ProbeAnti, BuildSemi, BuildAnti };" in hpp
    for call in ("nqe_hash_join_probe_semi(", "nqe_hash_join_marked_build(", "NQE_SEMI_ANTI", "NQE_SEMI_NULL_KEY_UNMATCHED"):
        assert call in hpp, call
    assert "std::dynamic_pointer_cast<HashSemiJoin>(plan)) return HashSemiJoin::create(rewrite(" in hpp
    assert os.path.exists(os.path.join(ROOT, "tests", "cpp", "test_semi_join.cpp"))


def test_rust_shim_declares_the_entry_points_and_a_semi_join():
    path = os.path.join(ROOT, "integration", "rust", "gpu.rs")
    src = crs.strip_rust(open(path).read())
    fns = crs.extern_functions(src)
    assert "nqe_hash_join_probe_semi" in fns and "nqe_hash_join_marked_build" in fns
    assert "pub struct GpuHashSemiJoin" in src and "impl GpuExec for GpuHashSemiJoin" in src and "impl PhysicalPlan for GpuHashSemiJoin" in src
    assert "pub enum SemiJoinType" in src
    assert crs.check(path)[0] == []
