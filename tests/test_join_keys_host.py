"""CPU-only: the hash join on several keys (quirk Q21) in every host layer — the tuple model of tests/join_keys_util.py by hand, against
pyarrow where the two definitions coincide (non-null keys) and, through dense tuple ids, against the unmodified oracle's single-key
join; the golden queries; the header prototypes and their bindings; the Python mirror and its rewrite arm; the C++ mirror and the Rust
shim.  No device is touched: the stub sources below are never executed."""
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

import join_keys_util as jku  # noqa: E402
import outer_join_util as oju  # noqa: E402
from naive_query_engine_amd import Column, DType, Field, read_csv  # noqa: E402
from naive_query_engine_amd import physical_plan as pp  # noqa: E402
from naive_query_engine_amd.rewrite import plan_shape, rewrite  # noqa: E402
from tools import check_rust_shim as crs  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
RANK = [Field("id", DType.INT64), Field("rank_name", DType.UTF8)]
EMP = [Field("id", DType.INT64), Field("name", DType.UTF8), Field("department_id", DType.INT64), Field("rank", DType.INT64)]
HOW = {"Inner": "inner", "Left": "left", "Right": "right"}


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
def test_model_every_pair_must_hold():
    left = [i64([1, 2, 1, 2, 1]), i64([2, 1, 1, 2, 2])]
    right = [i64([2, 1, 3, 1]), i64([1, 2, 3, 2])]
    # (1, 2) against (2, 1); probe-row-major, the matches of a probe row in ascending build row
    assert jku.join_pairs(left, [0, 1], [right], [0, 1], "inner") == [[(1, 0), (0, 1), (4, 1), (0, 3), (4, 3)]]
    assert jku.join_pairs(left, [0, 1], [right], [0, 1], "right") == [[(1, 0), (0, 1), (4, 1), (None, 2), (0, 3), (4, 3)]]
    assert jku.join_pairs(left, [0, 1], [right], [0, 1], "left") == [[(1, 0), (0, 1), (4, 1), (0, 3), (4, 3)], [(2, None), (3, None)]]
    assert jku.join_pairs(left, [0, 1], [right], [0, 1], "full")[1] == [(2, None), (3, None)]
    # the pairs in the other order are another join; with one pair it is the single-key model
    assert jku.join_pairs(left, [1, 0], [right], [0, 1], "inner") == [[(0, 0), (4, 0), (1, 1), (1, 3)]]
    xs, ys = oju.probe_pairs(left[0], right[0], True)
    assert jku.join_pairs(left, [0], [right], [0], "right") == [[(None if x < 0 else x, y) for x, y in zip(xs, ys)]]
    # the k-key join is a subset of the (k-1)-key join
    assert set(jku.join_pairs(left, [0, 1], [right], [0, 1], "inner")[0]) <= set(jku.join_pairs(left, [0], [right], [0], "inner")[0])


def test_model_marks_over_several_batches_and_empty_sides():
    left = [i64([1, 1, 2]), i64([1, 2, 2])]
    b1, b2, e = [i64([1]), i64([2])], [i64([2, 9]), i64([2, 9])], [i64([]), i64([])]
    assert jku.join_pairs(left, [0, 1], [b1, b2], [0, 1], "full") == [[(1, 0)], [(2, 0), (None, 1)], [(0, None)]]
    assert jku.join_pairs(left, [0, 1], [], [0, 1], "left") == [[(0, None), (1, None), (2, None)]]
    assert jku.join_pairs(e, [0, 1], [b2], [0, 1], "full") == [[(None, 0), (None, 1)], []]
    assert jku.join_pairs(left, [0, 1], [e], [0, 1], "inner") == [[]]


def test_model_null_slots_utf8_and_mixed_words():
    # a NULL key slot whose raw slot equals a real key matches, at every position (Q11)
    left = [Column.from_numpy(np.array([5, 7], dtype=np.int64), np.array([True, False])), oju.utf8_column(["a", "b"])]
    right = [Column.from_numpy(np.array([7, 7], dtype=np.int64), np.array([False, True])), oju.utf8_column(["b", "bb"])]
    assert jku.join_pairs(left, [0, 1], [right], [0, 1], "right") == [[(1, 0), (None, 1)]]
    # ("a", "bc") and ("ab", "c") are different tuples; the empty string is a key like any other
    l2, r2 = [oju.utf8_column(["a", "", "ab"]), oju.utf8_column(["bc", "", "c"])], [oju.utf8_column(["ab", "", "a"]), oju.utf8_column(["c", "", "b"])]
    assert jku.join_pairs(l2, [0, 1], [r2], [0, 1], "right") == [[(2, 0), (1, 1), (None, 2)]]
    # Int64 -1 and UInt64 2^64 - 1 share a raw slot: slots are compared, pair by pair, between columns of one type
    assert jku.tuples_of([i64([-1]), Column.from_numpy(np.array([2**64 - 1], dtype=np.uint64))], [0, 1]) == [(2**64 - 1, 2**64 - 1)]
    exp = jku.expected_batches(left, [0, 1], [right], [0, 1], "full")
    assert [c.to_list() for c in exp[0][0]] == [[None, None], ["b", None], [None, 7], ["b", "bb"]] and jku.null_counts(exp[0][0]) == [2, 1, 1, 0]
    assert [c.to_list() for c in exp[1][0]] == [[5], ["a"], [None], [None]] and exp[1][2].all()


# ----------------------------------------------------------------------------- the model against pyarrow and the oracle
def _tables(rng, kinds, n, m):
    def key(kind, v):
        if kind == "utf8":
            return oju.utf8_column([f"k{x}" for x in v])
        return Column.from_numpy(v.astype(np.int64 if kind == "int" else np.uint64))

    left = [key(kd, rng.integers(0, 5, n)) for kd in kinds] + [Column.from_numpy(rng.integers(-9, 9, n).astype(np.int64), rng.random(n) > 0.3), oju.utf8_column([None if v % 4 == 0 else "s%d" % v for v in range(n)])]
    right = [Column.from_numpy(rng.normal(0, 1, m))] + [key(kd, rng.integers(1, 7, m)) for kd in kinds] + [Column.from_numpy(rng.random(m) < 0.5, rng.random(m) > 0.2)]
    return left, list(range(len(kinds))), right, list(range(1, len(kinds) + 1))


def _to_arrow(col):
    import pyarrow as pa

    ty = {DType.INT64: pa.int64(), DType.UINT64: pa.uint64(), DType.FLOAT64: pa.uint64(), DType.BOOLEAN: pa.bool_(), DType.UTF8: pa.binary()}[col.dtype]
    return pa.array(oju.column_values(col), type=ty)  # (Float64 travels as its bit pattern: NaN payloads compare)


@pytest.mark.parametrize("how", ["inner", "left", "right", "full"])
@pytest.mark.parametrize("kinds", [("int", "int"), ("int", "uint", "utf8"), ("utf8", "utf8"), ("uint", "int", "int", "utf8")])
def test_model_agrees_with_pyarrow_as_multisets(kinds, how):
    pa = pytest.importorskip("pyarrow")
    for seed in range(5):
        rng = np.random.default_rng(seed * 11 + len(kinds) + len(how))
        n, m = int(rng.integers(0, 60)), int(rng.integers(0, 90))
        left, lkeys, right, rkeys = _tables(rng, kinds, n, m)
        cut = m // 2
        batches = [oju.take_null(right, np.arange(0, cut)), oju.take_null(right, np.arange(cut, m))]
        got = Counter(r for cols, _, _ in jku.expected_batches(left, lkeys, batches, rkeys, how) for r in oju.rows_of(cols))
        lt = pa.table({f"l{i}": _to_arrow(c) for i, c in enumerate(left)})
        rt = pa.table({f"r{i}": _to_arrow(c) for i, c in enumerate(right)})
        j = lt.join(rt, keys=[f"l{k}" for k in lkeys], right_keys=[f"r{k}" for k in rkeys], join_type={"inner": "inner", "left": "left outer", "right": "right outer", "full": "full outer"}[how],
                    coalesce_keys=False)
        j = j.select([f"l{i}" for i in range(len(left))] + [f"r{i}" for i in range(len(right))])
        assert got == Counter(tuple(r) for r in zip(*[j.column(nm).to_pylist() for nm in j.column_names])), (kinds, how, seed)


def test_dense_tuple_ids_through_the_single_key_oracle_give_the_inner_rows_in_order():
    from oracle import oracle as orc

    for seed, kinds in enumerate([("int", "int"), ("utf8", "int"), ("uint", "utf8", "int")]):
        rng = np.random.default_rng(40 + seed)
        left, lkeys, right, rkeys = _tables(rng, kinds, 80, 150)
        lid, rids = jku.dense_tuple_ids(left, lkeys, [right], rkeys)
        assert len(set(zip(lid.tolist(), jku.tuples_of(left, lkeys)))) == len(set(lid.tolist()))  # one id per tuple
        ref = orc.hash_join([left + [i64(lid)]], [right + [i64(rids[0])]], len(left), len(right))
        exp = jku.expected_batches(left, lkeys, [right], rkeys, "inner")[0][0]
        assert len(ref) == 1
        cols = ref[0][:len(left)] + ref[0][len(left) + 1:-1]
        oju.assert_same_columns(cols, exp, f"kinds {kinds}", presence=False)


# ----------------------------------------------------------------------------- golden queries
def _plain(rows):
    return [[v.decode() if isinstance(v, bytes) else v for v in r] for r in rows]


def test_golden_queries_match_the_model():
    with open(os.path.join(GOLDEN, "join_keys_expected.json")) as f:
        qs = json.load(f)["queries"]
    assert [(q["name"], q["join_type"]) for q in qs] == [("rank_join_employee_on_rank_and_department", "Inner"), ("rank_left_join_employee_on_rank_and_department", "Left"),
                                                         ("rank_right_join_employee_on_rank_and_department", "Right"), ("employee_join_employee_on_name_and_id", "Inner"),
                                                         ("employee_left_join_employee_on_department_and_rank_swapped", "Left")]
    for q in qs:
        lt, rt = read_csv(os.path.join(GOLDEN, q["left"] + ".csv")), read_csv(os.path.join(GOLDEN, q["right"] + ".csv"))
        assert [f.name for f in lt.fields] + [f.name for f in rt.fields] == q["columns"]
        lkeys = [[f.name for f in lt.fields].index(nm) for nm in q["left_keys"]]
        rkeys = [[f.name for f in rt.fields].index(nm) for nm in q["right_keys"]]
        batches = [_plain(oju.rows_of(cols)) for cols, _, _ in jku.expected_batches(lt.columns, lkeys, [rt.columns], rkeys, HOW[q["join_type"]])]
        assert batches == q["batches"], q["name"]
        assert len(q["batches"]) == (2 if q["join_type"] == "Left" else 1)
    assert qs[0]["batches"] == [[[1, "diamond", 1, "vee", 1, 1]]]  # only employee 1 has rank = department_id
    assert qs[1]["batches"][1] == [[0, "master", None, None, None, None], [2, "grandmaster", None, None, None, None]]
    assert len(qs[3]["batches"][0]) == 5


# ----------------------------------------------------------------------------- the C ABI
def test_header_declares_the_prototypes():
    hdr = open(os.path.join(ROOT, "include", "nqe.h")).read()
    ws = lambda s: re.sub(r"\\?\s+", r"\\s*", re.escape(s))  # noqa: E731
    for proto in ["#define NQE_MAX_JOIN_KEYS 8",
                  "nqe_status nqe_hash_join_build_keys(nqe_ctx *ctx, const nqe_table *left, const int32_t *left_keys, int32_t num_keys, nqe_join_table **out);",
                  "nqe_status nqe_hash_join_execute_keys(nqe_ctx *ctx, const nqe_table *left, const nqe_table *right, const int32_t *left_keys, const int32_t *right_keys, int32_t num_keys, nqe_table **out);"]:
        assert re.search(ws(proto), hdr), proto
    assert re.search(r"nqe_status\s+nqe_hash_join_probe_keys\s*\(\s*nqe_ctx\s*\*\s*ctx\s*,\s*const nqe_join_table\s*\*\s*build\s*,\s*const nqe_table\s*\*\s*right\s*,\s*const int32_t\s*\*\s*right_keys\s*,\s*"
                     r"int32_t\s+num_keys\s*,\s*uint32_t\s+flags\s*,\s*nqe_join_marks\s*\*\s*marks\s*(/\*.*?\*/)?\s*,\s*nqe_table\s*\*\*\s*out\s*\)\s*;", hdr)
    assert "#define NQE_ABI_VERSION 1" in hdr and "Q21" in hdr and "left + right + 2 > 32" in hdr
    assert hdr.index("typedef struct nqe_join_marks nqe_join_marks;") < hdr.index("nqe_hash_join_probe_keys")


def test_bindings_match_the_header():
    from naive_query_engine_amd import capi

    for s in ("nqe_hash_join_build_keys", "nqe_hash_join_probe_keys", "nqe_hash_join_execute_keys"):
        assert s in capi.SYMBOLS
    L = capi.lib()
    vp, i32, pi32, pvp = C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_void_p)
    assert L.nqe_hash_join_build_keys.argtypes == [vp, vp, pi32, i32, pvp]
    assert L.nqe_hash_join_probe_keys.argtypes == [vp, vp, vp, pi32, i32, C.c_uint32, vp, pvp]
    assert L.nqe_hash_join_execute_keys.argtypes == [vp, vp, vp, pi32, pi32, i32, pvp]
    assert all(f.restype is i32 for f in (L.nqe_hash_join_build_keys, L.nqe_hash_join_probe_keys, L.nqe_hash_join_execute_keys))
    assert list(inspect.signature(capi.Context.hash_join_build_keys).parameters) == ["self", "left", "left_keys"]
    sig = inspect.signature(capi.Context.hash_join_probe_keys)
    assert list(sig.parameters) == ["self", "jt", "right", "right_keys", "keep_probe", "marks"]
    assert sig.parameters["keep_probe"].default is False and sig.parameters["marks"].default is None
    assert list(inspect.signature(capi.Context.hash_join_keys).parameters) == ["self", "left", "right", "left_keys", "right_keys"]


# ----------------------------------------------------------------------------- the mirrors
ON2 = [(pp.ColumnRef(None, "id"), pp.ColumnRef(None, "rank")), (pp.ColumnRef(None, "id"), pp.ColumnRef(None, "department_id"))]


def test_mirror_construction_schema_children_and_errors():
    ls, rs = pp.ScanPlan.create(_Stub(RANK)), pp.ScanPlan.create(_Stub(EMP))
    assert list(inspect.signature(pp.MultiKeyHashJoin.create).parameters) == ["left", "right", "on", "join_type", "schema"]
    plan = pp.MultiKeyHashJoin.create(ls, rs, ON2, pp.JoinType.Left, RANK + EMP)
    assert isinstance(plan, pp.PhysicalPlan) and not isinstance(plan, (pp.HashJoin, pp.HashOuterJoin))
    assert plan.children() == [ls, rs] and plan.join_type == pp.JoinType.Left and plan.on == ON2
    assert [f.name for f in plan.schema()] == ["id", "rank_name", "id", "name", "department_id", "rank"]
    assert not hasattr(plan, "_executions")  # no Q11 state
    # Cross is refused before the children run (the stub would raise an AssertionError); an empty `on` after both children ran
    from naive_query_engine_amd import ErrorCode, Status

    with pytest.raises(ErrorCode) as e:
        pp.MultiKeyHashJoin.create(ls, rs, ON2, pp.JoinType.Cross, RANK + EMP).execute()
    assert e.value.status == Status.PlanError
    with pytest.raises(AssertionError, match="never scanned"):
        pp.MultiKeyHashJoin.create(ls, rs, [], pp.JoinType.Inner, RANK + EMP).execute()

    class _Ran(pp.PhysicalPlan):
        ran = 0

        def schema(self):
            return RANK

        def children(self):
            return []

        def execute(self):
            _Ran.ran += 1
            return []

    with pytest.raises(ErrorCode) as e:
        pp.MultiKeyHashJoin.create(_Ran(), _Ran(), [], pp.JoinType.Inner, RANK + RANK).execute()
    assert e.value.status == Status.PlanError and _Ran.ran == 2


def test_rewrite_keeps_the_operator_with_rewritten_children():
    from naive_query_engine_amd import ColumnExpr, Operator, PhysicalBinaryExpr, PhysicalLiteralExpr, ScalarValue

    pred = PhysicalBinaryExpr.create(ColumnExpr.try_create("id", None), Operator.Gt, PhysicalLiteralExpr.create(ScalarValue.Int64(0)))
    proj = pp.ProjectionPlan.create(pp.SelectionPlan.create(pp.ScanPlan.create(_Stub(RANK)), pred), RANK, [ColumnExpr.try_create(f.name, None) for f in RANK])
    tree = pp.MultiKeyHashJoin.create(proj, pp.ScanPlan.create(_Stub(EMP)), ON2, pp.JoinType.Right, RANK + EMP)
    assert plan_shape(tree) == ["MultiKeyHashJoin", "ProjectionPlan", "SelectionPlan", "ScanPlan", "ScanPlan"]
    out = rewrite(tree)
    assert plan_shape(out) == ["MultiKeyHashJoin", "FusedSelectionProjectionPlan", "ScanPlan", "ScanPlan"]
    assert isinstance(out, pp.MultiKeyHashJoin) and out is not tree and out.join_type == pp.JoinType.Right and out.on == ON2 and out.schema() == tree.schema()
    assert plan_shape(rewrite(out)) == plan_shape(out)


def test_cpp_mirror_has_the_join_and_the_rewrite_arm():
    hpp = open(os.path.join(ROOT, "naive_query_engine_amd", "host", "naive_db.hpp")).read()
    assert "struct MultiKeyHashJoin : PhysicalPlan" in hpp
    for call in ("nqe_hash_join_build_keys(", "nqe_hash_join_probe_keys("):
        assert call in hpp, call
    assert "std::dynamic_pointer_cast<MultiKeyHashJoin>(plan)) return MultiKeyHashJoin::create(rewrite(" in hpp
    assert os.path.exists(os.path.join(ROOT, "tests", "cpp", "test_join_keys.cpp"))


def test_rust_shim_declares_the_entry_points_and_the_join():
    path = os.path.join(ROOT, "integration", "rust", "gpu.rs")
    src = crs.strip_rust(open(path).read())
    fns = crs.extern_functions(src)
    for s in ("nqe_hash_join_build_keys", "nqe_hash_join_probe_keys", "nqe_hash_join_execute_keys"):
        assert s in fns, s
    assert "pub struct GpuMultiKeyHashJoin" in src and "impl GpuExec for GpuMultiKeyHashJoin" in src and "impl PhysicalPlan for GpuMultiKeyHashJoin" in src
    assert crs.check(path)[0] == []
