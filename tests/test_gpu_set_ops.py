"""DISTINCT and the set operators on the device (nqe_distinct_execute / nqe_set_op_execute, csrc/set_ops.hip; quirk Q24).

The yardstick is the row-at-a-time model of tests/set_ops_util.py (held to sqlite3 and to the sort's tie in
tests/test_set_ops_model.py).  Rows are copied, so everything is compared bit for bit: values, validity, null_count and order.

The 2^31-row bound is reached with one Boolean column (256 MB of bits).  Not run here: NQE_ERR_OUT_OF_MEMORY (it would take a table
larger than the device's memory) and tables of more than 2^30 rows that are accepted (a 32 GB set table): the arithmetic of the
2^32-slot table is checked on the CPU (tests/cpp/test_set_ops_plan.cpp).  The probe that wraps from the table's end to its start needs
constructed hash collisions: tests/cpp/test_set_ops.cpp."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import order_by_util as obu  # noqa: E402
import set_ops_util as su  # noqa: E402
from naive_query_engine_amd import (Column, ColumnExpr, DType, ErrorCode, Field, Operator, PhysicalBinaryExpr, PhysicalLiteralExpr, RecordBatch, ScalarValue, SetOp,  # noqa: E402
                                    Status, WindowFunc as W)

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(ROOT, "tests", "golden")
EDGES = su.EDGE_ROWS


@pytest.fixture(scope="module")
def pp():
    from naive_query_engine_amd import physical_plan

    return physical_plan


@pytest.fixture(scope="module")
def ctx():
    from naive_query_engine_amd import capi

    return capi.default_context()


class Launches:
    """the kernel launches of the context while the block runs"""

    def __init__(self, ctx):
        self.ctx = ctx

    def __enter__(self):
        self.ctx.timing_enable(True)
        self.ctx.timing_reset()
        return self

    def count(self, name=""):
        return self.ctx.timing_query(name)[1]

    def __exit__(self, *exc):
        self.ctx.timing_enable(False)
        self.ctx.timing_reset()


def same(table, exp, what):
    """the device table against the model's columns: rows bit for bit, and the exact null_count of every column"""
    got = table.to_host()
    obu.assert_same_rows(got, exp, what)
    assert table.num_rows == (exp[0].length if exp else 0), what
    for i, e in enumerate(exp):
        assert int(table.column_info(i).null_count) == e.null_count, f"{what}: null_count of column {i}"
    return got


def check_distinct(ctx, cols, keys, what=""):
    return same(ctx.distinct(ctx.table_from_host(cols), keys), su.distinct(cols, keys), f"{what} distinct on {keys}")


def check_set_ops(ctx, left, right, what=""):
    """all three operators against the model; INTERSECT and EXCEPT interleave back to distinct(left); UNION is distinct(concat)"""
    lt, rt = ctx.table_from_host(left), ctx.table_from_host(right)
    out = {op: same(ctx.set_op(lt, rt, op), su.set_op(left, right, op), f"{what} {op.name} {left[0].length} x {right[0].length}") for op in SetOp}
    irows, erows = su.set_op_rows(left, right, SetOp.Intersect)[1], su.set_op_rows(left, right, SetOp.Except)[1]
    merged = sorted([(r, 0, j) for j, r in enumerate(irows)] + [(r, 1, j) for j, r in enumerate(erows)])
    rebuilt = obu.take(obu.concat_columns([out[SetOp.Intersect], out[SetOp.Except]]), [j + side * len(irows) for _, side, j in merged])
    obu.assert_same_rows(ctx.distinct(lt).to_host(), rebuilt, f"{what} INTERSECT and EXCEPT interleaved in left's order")
    if left[0].length + right[0].length:
        obu.assert_same_rows(out[SetOp.Union], ctx.distinct(ctx.concat([lt, rt])).to_host(), f"{what} UNION is distinct(concat)")
    return out


def i64(a):
    return Column.from_numpy(np.asarray(a, dtype=np.int64))


def f64_bits(bits):
    return Column.from_numpy(np.array(bits, dtype=np.uint64).view(np.float64))


# ----------------------------------------------------------------------------- 1. edges
@pytest.mark.parametrize("n", EDGES)
@pytest.mark.parametrize("shape", su.KEY_SHAPES)
def test_row_count_edges_by_key_shape(ctx, shape, n):
    for distinct_tuples in (1, 7, n):
        rng = np.random.default_rng(1000 * n + distinct_tuples)
        keys = su.key_columns(rng, shape, n, distinct_tuples)
        cols = keys + su.payload_columns(rng, n)  # two payload columns outside `cols`, one Utf8 with NULLs
        with Launches(ctx) as L:
            got = check_distinct(ctx, cols, list(range(len(keys))), what=f"{shape} n={n} tuples={distinct_tuples}")
            assert len(got) == len(cols)  # zero rows: a 0-row table with every column
            if n:
                assert [L.count(s) for s in ("set_table_init", "set_insert", "set_keep", "set_find")] == [1, 1, 1, 0]
        if shape != "five_dtypes" and distinct_tuples == n:
            assert got[0].length == n  # every row its own tuple: nothing is dropped


def test_key_order_does_not_matter_and_payload_comes_from_the_first_row(ctx):
    rng = np.random.default_rng(3)
    n = 5000
    cols = su.key_columns(rng, "five_dtypes", n, 40) + su.payload_columns(rng, n)
    a = check_distinct(ctx, cols, [0, 1, 2, 3, 4])
    b = check_distinct(ctx, cols, [4, 2, 0, 3, 1])
    obu.assert_same_rows(a, b, "permuted key list")
    check_distinct(ctx, cols, [3])  # a Boolean key alone: at most true, false and NULL
    check_distinct(ctx, cols, [4, 3])
    check_distinct(ctx, cols, None)  # every column, the row number among them: every row stays
    assert ctx.distinct(ctx.table_from_host(cols)).num_rows == n


# ----------------------------------------------------------------------------- 2. semantics, one small table each
def test_nulls_over_different_bytes_collapse(ctx):
    k = Column.from_numpy(np.array([5, 9, 5, -1, 9], dtype=np.int64), np.array([False, False, True, False, True]))
    s = obu.utf8_column([None, None, b"a", None, b"a"], null_bytes=b"")
    s2 = Column(DType.UTF8, 5, np.array([0, 2, 5, 6, 7, 8], dtype=np.int32), s.validity.copy(), np.frombuffer(b"xxyyyaza", dtype=np.uint8).copy())  # other bytes under each NULL
    got = check_distinct(ctx, [k, s2, i64(range(5))], [0, 1])
    assert got[2].to_list() == [0, 2, 4]
    assert check_distinct(ctx, [k, i64(range(5))], [0])[1].to_list() == [0, 2, 4]


def test_signed_zeros_collapse_and_the_first_rows_bits_survive(ctx):
    for bits, first in (([0x8000000000000000, 0, 0x8000000000000000, 0], 0x8000000000000000), ([0, 0x8000000000000000, 0], 0)):
        got = check_distinct(ctx, [f64_bits(bits), i64(range(len(bits)))], [0])
        assert got[0].to_numpy().view(np.uint64).tolist() == [first] and got[1].to_list() == [0]


def test_nan_payloads_collapse(ctx):
    bits = [0x7ff8000000000000, 0xfff0000000000001, 0x7ff8000000001234, 0x7ff0000000000000, 0xfff0000000000000, 0xffffffffffffffff]
    got = check_distinct(ctx, [f64_bits(bits), i64(range(6))], [0])
    assert got[1].to_list() == [0, 3, 4] and got[0].to_numpy().view(np.uint64)[0] == bits[0]  # one NaN (its own payload kept), +inf, -inf
    got = check_distinct(ctx, [Column.from_numpy(np.array(bits, dtype=np.uint64).view(np.float64), np.array([True, True, False, True, True, False])), i64(range(6))], [0])
    assert got[1].to_list() == [0, 2, 3, 4]  # a NULL over a NaN is a NULL


def test_empty_string_is_not_null(ctx):
    got = check_distinct(ctx, [obu.utf8_column([b"", None, b"", None, b"a"], null_bytes=b""), i64(range(5))], [0])
    assert got[1].to_list() == [0, 1, 4] and got[0].to_list() == ["", None, "a"]


def test_tuples_compare_position_by_position(ctx):
    assert check_distinct(ctx, [obu.utf8_column([b"a", b"ab", b"a"]), obu.utf8_column([b"b", b"", b"b"])], None)[0].to_list() == ["a", "ab"]
    assert check_distinct(ctx, [i64([1, 2, 1]), i64([2, 1, 2])], None)[0].to_list() == [1, 2]
    u = Column.from_numpy(np.array([1, 2, 1], dtype=np.uint64))
    assert check_distinct(ctx, [i64([1, 2, 1]), u, i64([2, 1, 2]), u, i64([0, 0, 0])], None)[0].to_list() == [1, 2]  # five word keys: the general form


def test_boolean_keys(ctx):
    b = Column.from_numpy(np.array([True, False, True, False, True, False]), np.array([True, True, True, True, False, False]))
    assert check_distinct(ctx, [b, i64(range(6))], [0])[1].to_list() == [0, 1, 4]
    b2 = Column.from_numpy(np.array([True, False, True, True]))
    assert check_distinct(ctx, [b2, Column.from_numpy(np.array([False, False, False, True])), i64(range(4))], [0, 1])[2].to_list() == [0, 1, 3]


def test_a_null_in_one_key_only(ctx):
    a = Column.from_numpy(np.array([1, 1, 1, 1, 2], dtype=np.int64), np.array([True, False, True, False, True]))
    b = i64([7, 7, 7, 7, 7])
    assert check_distinct(ctx, [a, b, i64(range(5))], [0, 1])[2].to_list() == [0, 1, 4]  # (1,7), (NULL,7), (2,7)
    assert check_distinct(ctx, [b, a, i64(range(5))], [0, 1])[2].to_list() == [0, 1, 4]
    # a validity buffer of all ones is not a NULL: the word form and the general form agree
    ones = Column.from_numpy(np.array([3, 3, 4], dtype=np.int64), np.ones(3, dtype=bool))
    assert check_distinct(ctx, [ones, i64(range(3))], [0])[1].to_list() == [0, 2]


# ----------------------------------------------------------------------------- 3. determinism and contention
def test_one_tuple_keeps_row_zero(ctx):
    n = 12289
    for keys in ([i64(np.full(n, 42))], [i64(np.full(n, 42)), Column.from_numpy(np.full(n, 7, dtype=np.uint64))],
                 [obu.utf8_column([b"same"] * n), Column.from_numpy(np.full(n, np.nan))], [Column.from_numpy(np.zeros(n, dtype=np.int64), np.zeros(n, dtype=bool))]):
        got = check_distinct(ctx, keys + [i64(range(n))], list(range(len(keys))))
        assert got[-1].to_list() == [0]


def test_three_runs_give_identical_bytes(ctx):
    rng = np.random.default_rng(11)
    n = 12289
    cols = su.key_columns(rng, "five_dtypes", n, 300) + su.payload_columns(rng, n)
    t = ctx.table_from_host(cols)
    right = ctx.table_from_host(obu.take(cols, rng.integers(0, n, 500)))
    runs = [[ctx.distinct(t, [0, 1, 2, 3, 4]).to_host()] + [ctx.set_op(t, right, op).to_host() for op in SetOp] for _ in range(3)]
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            obu.assert_same_rows(a, b, "run to run")
            for x, y in zip(a, b):
                assert x.values.tobytes() == y.values.tobytes() and (x.data is None or x.data.tobytes() == y.data.tobytes())


# ----------------------------------------------------------------------------- 4. the second device path: row_number() over the tuple, then a selection
def test_equals_window_row_number_then_selection(ctx):
    n = 1 << 17
    rng = np.random.default_rng(17)
    keys = su.key_columns(rng, "five_dtypes", n, 3000)
    cols = keys + su.payload_columns(rng, n)
    t = ctx.table_from_host(cols)
    part = [0, 1, 2, 3, 4]
    rn = ctx.window(t, part, [], [(W.RowNumber,)])
    beside = ctx.append_columns(t, [rn])
    fields = [Field(f"c{i}", c.dtype, True) for i, c in enumerate(cols)] + [Field("rn", DType.UINT64, False)]
    pred = PhysicalBinaryExpr.create(ColumnExpr.try_create(None, len(cols)), Operator.Eq, PhysicalLiteralExpr.create(ScalarValue.UInt64(1)))
    first = ctx.project(ctx.selection(beside, pred.flatten(fields)), list(range(len(cols))))
    got = ctx.distinct(t, part)
    assert 0 < got.num_rows < n
    obu.assert_same_rows(got.to_host(), first.to_host(), "distinct against row_number() = 1")


# ----------------------------------------------------------------------------- 5. set operators
def _overlapping(rng, shape, nl, nr, overlap):
    """left and right tables of the key shape (every column is a key of a set operation), drawn from a pool of tuple ids a third of
    left's rows, so both sides hold duplicates; `overlap`: none / about half / all of right's tuples occur in left"""
    pool = max(1, nl // 3)
    lids = rng.integers(0, pool, nl)
    first = {"none": pool, "half": pool // 2, "all": 0}[overlap]
    rids = rng.integers(first, first + pool, nr)

    def table(ids):
        if shape == "words2":
            return [i64(ids % 11 - 5), Column.from_numpy((ids // 11).astype(np.uint64))]
        f = np.array([0.0, -0.0, np.nan, 1.5], dtype=np.float64)
        nulls = lambda salt: ((ids * 2654435761 + salt) >> 2) % 3 != 0
        return [Column.from_numpy((ids * 5).astype(np.int64), nulls(1)), Column.from_numpy(f[ids % 4] + ids // 4, nulls(2)), Column.from_numpy(ids % 2 == 0, nulls(3)),
                obu.utf8_column([obu.WORDS[int(t) % len(obu.WORDS)] + str(int(t)).encode() if ok else None for t, ok in zip(ids, nulls(4))], null_bytes=b"??")]

    return table(lids), table(rids)


SET_SIZES = [(0, 0), (0, 65), (65, 0), (1, 1), (64, 4097), (2049, 63), (4096, 4096), (4097, 12289), (1229, 12289)]  # the last: right ten times left


@pytest.mark.parametrize("overlap", ["none", "half", "all"])
@pytest.mark.parametrize("shape", ["words2", "general"])
def test_set_operators_against_the_model(ctx, shape, overlap):
    for nl, nr in SET_SIZES:
        rng = np.random.default_rng(nl * 31 + nr)
        left, right = _overlapping(rng, shape, nl, nr, overlap)
        what = f"{shape} {overlap} {nl} x {nr}"
        res = check_set_ops(ctx, left, right, what)
        if nl and nr and overlap == "none" and shape == "words2":  # (the general shape's tuples may be all NULL on both sides whatever the ids)
            assert res[SetOp.Intersect][0].length == 0 and res[SetOp.Except][0].length == su.distinct(left)[0].length, what
        if nl > 100 and nr > 100 and overlap == "half":
            assert res[SetOp.Intersect][0].length and res[SetOp.Except][0].length, what


def test_launches_of_the_three_operators(ctx):
    left, right = _overlapping(np.random.default_rng(2), "words2", 4097, 2049, "half")
    lt, rt = ctx.table_from_host(left), ctx.table_from_host(right)
    for op, finds in ((SetOp.Union, 0), (SetOp.Intersect, 1), (SetOp.Except, 1)):
        with Launches(ctx) as L:
            ctx.set_op(lt, rt, op)
            assert [L.count(s) for s in ("set_table_init", "set_insert", "set_find", "set_keep")] == [1, 1, finds, 1]


def test_a_nullable_right_side_against_a_plain_left_side(ctx):
    # left takes the word form, right holds NULLs and cannot: both are read through the general form, the same hash
    left = [i64([1, 2, 3, 2, 0]), Column.from_numpy(np.array([5, 6, 7, 6, 0], dtype=np.uint64))]
    right = [Column.from_numpy(np.array([2, 0, 3], dtype=np.int64), np.array([True, False, True])), Column.from_numpy(np.array([6, 0, 8], dtype=np.uint64))]
    res = check_set_ops(ctx, left, right)
    assert res[SetOp.Intersect][0].to_list() == [2] and res[SetOp.Except][0].to_list() == [1, 3, 0]
    res = check_set_ops(ctx, right, left)
    assert res[SetOp.Intersect][0].to_list() == [2] and res[SetOp.Except][0].to_list() == [None, 3]


# ----------------------------------------------------------------------------- 6. errors
def test_errors_launch_nothing(pp, ctx):
    from naive_query_engine_amd import capi

    cols = [i64(np.arange(10)), obu.utf8_column([b"x"] * 10), Column.from_numpy(np.arange(10) % 2 == 0), Column.from_numpy(np.arange(10.0))]
    t = ctx.table_from_host(cols)
    t2 = ctx.table_from_host(cols[:3])
    t3 = ctx.table_from_host([cols[0], cols[1], cols[3], cols[2]])
    wide = ctx.table_from_host([cols[0]] * 33)

    def refused(status, text, fn, *args):
        with pytest.raises(ErrorCode) as e:
            fn(*args)
        assert e.value.status == status and text in str(e.value), (args, str(e.value))

    with Launches(ctx) as L:
        d, s = capi.lib().nqe_distinct_execute, capi.lib().nqe_set_op_execute
        h = C.c_void_p()
        ints = (C.c_int32 * 2)(0, 1)
        for args in ((None, t.handle, ints, 2, C.byref(h)), (ctx.handle, None, ints, 2, C.byref(h)), (ctx.handle, t.handle, ints, 2, None), (ctx.handle, t.handle, None, 2, C.byref(h)),
                     (ctx.handle, t.handle, None, 99, C.byref(h))):  # a NULL array with a positive count comes before the limit
            assert d(*args) == Status.InvalidArgument and not h.value
        for args in ((None, t.handle, t.handle, 0, C.byref(h)), (ctx.handle, None, t.handle, 0, C.byref(h)), (ctx.handle, t.handle, None, 0, C.byref(h)), (ctx.handle, t.handle, t.handle, 0, None),
                     (ctx.handle, t.handle, t.handle, 3, C.byref(h)), (ctx.handle, t.handle, t.handle, -1, C.byref(h)),
                     (ctx.handle, t.handle, t2.handle, 3, C.byref(h))):  # the operator's enum comes before the column counts
            assert s(*args) == Status.InvalidArgument and not h.value
        assert d(ctx.handle, t.handle, ints, -1, C.byref(h)) == Status.NotSupported and not h.value
        refused(Status.PlanError, "4 and 3 columns", ctx.set_op, t, t2, SetOp.Union)
        refused(Status.PlanError, "column 2 differs in type", ctx.set_op, t, t3, SetOp.Intersect)  # the FIRST differing column
        refused(Status.PlanError, "33 and 4 columns", ctx.set_op, wide, t, SetOp.Except)            # the column counts come before the limit
        refused(Status.NotSupported, "at most 32 columns", ctx.set_op, wide, wide, SetOp.Except)
        refused(Status.NotSupported, "at most 32 key columns", ctx.distinct, wide, None)
        refused(Status.NotSupported, "at most 32 key columns", ctx.distinct, wide, list(range(33)))
        refused(Status.NotSupported, "at most 32 key columns", ctx.distinct, t, [0] * 33)           # the limit comes before the duplicate
        for bad in ([4], [-1], [0, 4]):
            refused(Status.NotSupported, "key column index out of range", ctx.distinct, t, bad)
        refused(Status.NotSupported, "given twice", ctx.distinct, t, [1, 0, 1])
        refused(Status.NotSupported, "key column index out of range", ctx.distinct, t, [0, 0, 7][::-1])  # the first offending key in list order
        refused(Status.PlanError, "no key columns", ctx.distinct, t, [])
        assert L.count("") == 0  # nothing was launched
    assert ctx.distinct(wide, list(range(32))).num_rows == 10  # the limit itself is fine
    fields = [Field("a", DType.INT64, False), Field("s", DType.UTF8, False), Field("b", DType.BOOLEAN, False), Field("f", DType.FLOAT64, False)]
    empty = pp.ScanPlan.create(pp.MemTable(fields, []), None)
    full = pp.ScanPlan.create(pp.MemTable.try_create(fields, [RecordBatch(fields, cols)], ctx), None)
    for plan in (pp.PhysicalDistinctPlan.create(empty), pp.PhysicalSetOpPlan.create(empty, full, SetOp.Union), pp.PhysicalSetOpPlan.create(full, empty, SetOp.Except)):
        with pytest.raises(ErrorCode) as e:
            plan.execute()
        assert e.value.status == Status.NotSupported


def test_two_to_the_31_rows_are_refused_and_the_probed_side_has_no_limit(ctx):
    n = 1 << 31
    bits = np.zeros(n // 8, dtype=np.uint8)
    bits[0] = 0b101  # rows 0 and 2 true, everything else false
    big = ctx.table_from_host([Column(DType.BOOLEAN, n, bits)])
    half = ctx.table_from_host([Column(DType.BOOLEAN, n // 2, bits[: n // 16])])
    small = ctx.table_from_host([Column.from_numpy(np.array([True, True, False]))])
    only_true = ctx.table_from_host([Column.from_numpy(np.array([True, True]))])
    with Launches(ctx) as L:
        for fn, args in ((ctx.distinct, (big,)), (ctx.distinct, (big, [0])), (ctx.set_op, (big, small, SetOp.Intersect)), (ctx.set_op, (big, small, SetOp.Except)),
                         (ctx.set_op, (big, small, SetOp.Union)), (ctx.set_op, (small, big, SetOp.Union)), (ctx.set_op, (half, half, SetOp.Union))):  # UNION inserts both sides
            with pytest.raises(ErrorCode) as e:
                fn(*args)
            assert e.value.status == Status.NotSupported and "fewer than 2^31" in str(e.value), str(e.value)
        assert L.count("") == 0  # nothing was launched
    # the probed right side of INTERSECT / EXCEPT has no such limit: 2^31 rows are looked up
    assert ctx.set_op(small, big, SetOp.Intersect).to_host()[0].to_list() == [True, False]
    assert ctx.set_op(small, big, SetOp.Except).num_rows == 0
    assert ctx.set_op(only_true, big, SetOp.Intersect).to_host()[0].to_list() == [True]


# ----------------------------------------------------------------------------- 7. the differential fuzzer
FUZZ_SEEDS = list(range(20 + int(os.environ.get("NQE_SET_FUZZ_EXTRA_SEEDS", "0"))))


@pytest.mark.parametrize("seed", FUZZ_SEEDS)
def test_fuzz_both_entry_points(ctx, seed):
    rng = np.random.default_rng(7000 + seed)
    ncols = int(rng.integers(1, 7))
    dtypes = [obu.ALL_DTYPES[int(rng.integers(0, 5))] for _ in range(ncols)]
    null_fraction = float(rng.choice([0.0, 0.1, 1.0]))
    distinct = int(rng.choice([2, 5, 17]))
    n, m = int(rng.choice(EDGES)), int(rng.choice(EDGES))
    left, right = su.random_table(rng, n, dtypes, null_fraction, distinct), su.random_table(rng, m, dtypes, float(rng.choice([0.0, 0.1, 1.0])), distinct)
    what = f"seed {seed}: {[d.name for d in dtypes]} nulls {null_fraction} {n} x {m}"
    keys = sorted(rng.choice(ncols, int(rng.integers(1, ncols + 1)), replace=False).tolist())
    rng.shuffle(keys)
    check_distinct(ctx, left + [i64(range(n))], [int(k) for k in keys], what)
    check_distinct(ctx, left, None, what)
    check_set_ops(ctx, left, right, what)


# ----------------------------------------------------------------------------- 8. the Python mirrors
def _mem(pp, ctx, fields, cols, cuts):
    """a scan over a MemTable whose batches are the rows of `cols` cut at `cuts`"""
    n = cols[0].length
    edges = [0] + [c for c in cuts if c < n] + [n]
    batches = [obu.take(cols, np.arange(a, b)) for a, b in zip(edges[:-1], edges[1:])]
    return pp.ScanPlan.create(pp.MemTable.try_create(fields, [RecordBatch(fields, b) for b in batches], ctx), None)


def test_golden_queries_through_the_python_mirrors_over_several_batches(pp, ctx):
    from naive_query_engine_amd.rewrite import NaiveDB, plan_shape, rewrite

    doc, tables = su.golden_load(GOLDEN)
    db = NaiveDB()
    col = lambda name: ColumnExpr.try_create(name, None)
    for q in doc["queries"]:
        def scan(spec):
            fields, cols = su.golden_input(tables, spec)
            return _mem(pp, ctx, fields, cols, [2, 2, 3])  # three or four batches, one of them empty
        if q["kind"] == "distinct":
            plan = pp.PhysicalDistinctPlan.create(scan(q["input"]), None if q["on"] is None else [col(c) for c in q["on"]])
            assert plan_shape(rewrite(plan)) == ["PhysicalDistinctPlan", "ScanPlan"]
        else:
            plan = pp.PhysicalSetOpPlan.create(scan(q["left"]), scan(q["right"]), SetOp[q["op"]])
            assert plan_shape(rewrite(plan)) == ["PhysicalSetOpPlan", "ScanPlan", "ScanPlan"]
        for out in (plan.execute(), db.run_plan(plan)):
            assert len(out) == 1 and [f.name for f in out[0].fields] == q["columns"], q["name"]
            rows = [list(r) for r in zip(*[c.to_list() for c in out[0].table.to_host()])]
            assert rows == q["rows"], q["name"]


def test_distinct_on_an_expression_through_the_mirror(pp, ctx):
    n = 4097
    rng = np.random.default_rng(41)
    fields = [Field("id", DType.INT64, False), Field("v", DType.FLOAT64, True)]
    cols = [i64(rng.integers(0, 1000, n)), obu.random_column(rng, DType.FLOAT64, n, True, 5)]
    expr = PhysicalBinaryExpr.create(ColumnExpr.try_create("id", None), Operator.Modulos, PhysicalLiteralExpr.create(ScalarValue.Int64(7)))
    plan = pp.PhysicalDistinctPlan.create(_mem(pp, ctx, fields, cols, [100, 4096]), [expr, ColumnExpr.try_create("v", None)])
    out = plan.execute()
    assert len(out) == 1 and [f.name for f in out[0].fields] == ["id", "v"] and out[0].num_columns == 2  # the temporary never reaches the output
    with_temp = cols + [i64(cols[0].to_numpy() % 7)]
    obu.assert_same_rows(out[0].table.to_host(), su.distinct(with_temp, [2, 1])[:2], "distinct on (id % 7, v)")
