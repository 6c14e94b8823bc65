"""GROUP BY on several keys on the device (nqe_group_aggregate_execute, csrc/group_keys.hip; quirk Q20).

The yardstick is the dict-over-tuples model of tests/group_keys_util.py.  As a second, independent check the model's dense tuple ids are
handed to the unmodified oracle's single-key aggregate with the same predicate: its rows, ordered by min(id), are the expected aggregate
rows.  Values are integer-valued Float64 (or Int64) unless a test says otherwise, so sums are exact and every column compares bit for
bit.  Which path ran — packed or dictionary — is asserted through nqe_ctx_timing_query on the kernels' names."""
import ctypes as C
import gc
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import group_keys_util as gku  # noqa: E402
from helpers import assert_column_equal  # noqa: E402
from naive_query_engine_amd import AggregateFunc, Column, DType, ErrorCode, Field, Operator, RecordBatch, Status  # noqa: E402
from naive_query_engine_amd.arrow_host import node_column  # noqa: E402
from naive_query_engine_amd.expression import binop, col, lit_f64, lit_i64, lit_utf8  # noqa: E402

pytestmark = pytest.mark.gpu
I64 = np.iinfo(np.int64)
ALL = [(AggregateFunc.Count, None), (AggregateFunc.Sum, None), (AggregateFunc.Avg, None), (AggregateFunc.Min, None), (AggregateFunc.Max, None)]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def ctx():
    from naive_query_engine_amd import capi

    c = capi.default_context()
    c.timing_enable(True)
    yield c
    c.timing_enable(False)


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle

    return oracle


def fields_of(cols):
    return [Field(f"c{i}", c.dtype, True) for i, c in enumerate(cols)]


def aggs_over(c):
    return [(f, c) for f, _ in ALL]


class Key:
    """one group key: a bare column, or `column % m` (an expression key)"""

    def __init__(self, column, mod=None):
        self.column, self.mod = column, mod

    def nodes(self, cols):
        e = col(self.column) if self.mod is None else binop(col(self.column), Operator.Modulos, lit_i64(self.mod))
        return e.flatten(fields_of(cols))

    def values(self, cols):
        vals = gku.key_values(cols[self.column])
        if self.mod is None:
            return vals
        return [None if v is None else (abs(v) % self.mod) * (-1 if v < 0 else 1) for v in vals]  # truncated remainder


def keys_of(*specs):
    return [s if isinstance(s, Key) else Key(s) for s in specs]


def path_taken(ctx):
    pack, dct = ctx.timing_query("group_keys_pack")[1], ctx.timing_query("group_keys_dict")[1]
    ranges, decode = ctx.timing_query("group_keys_ranges")[1], ctx.timing_query("group_keys_decode")[1]
    if pack:
        assert ranges == 1 and pack == 1 and dct == 0
        return "pack"
    if dct:
        assert decode == 0
        return "dict"
    assert ranges == 0 and decode == 0
    return "none"


def check(ctx, orc, cols, keys, aggs, pred=None, keep=None, path=None, rtol=None, what=""):
    """runs the call and compares with the model and, through dense ids, with the oracle; returns the downloaded columns"""
    keys = keys_of(*keys)
    t = ctx.table_from_host(cols)
    ctx.timing_reset()
    out = ctx.group_aggregate(t, [k.nodes(cols) for k in keys], aggs, pred_nodes=pred)
    taken = path_taken(ctx)
    got = out.to_host()
    tuples, exp, dense = gku.model([k.values(cols) for k in keys], cols, aggs, keep)
    if path is not None and cols[0].length > 0:
        assert taken == path, f"{what}: path {taken}, expected {path}"
    assert len(got) == len(keys) + len(aggs), what
    assert out.num_rows == len(tuples), f"{what}: {out.num_rows} groups, model {len(tuples)}"
    for i, k in enumerate(keys):
        kc = got[i]
        src = cols[k.column]
        assert kc.dtype == src.dtype and kc.validity is None, f"{what}: key column {i}"
        assert gku.key_values(kc) == [tp[i] for tp in tuples], f"{what}: key column {i} differs"
    for j, (func, _) in enumerate(aggs):
        e = Column.from_numpy(exp[j])
        assert_column_equal(got[len(keys) + j], e, rtol=rtol if func in (AggregateFunc.Sum, AggregateFunc.Avg) else None, what=f"{what} aggregate {j} vs model")
    # the oracle's single-key aggregate over the dense ids
    idc = Column.from_numpy(np.where(dense < 0, 0, dense).astype(np.int64), mask=(dense >= 0) if (dense < 0).any() else None)
    ocols = list(cols) + [idc]
    oaggs = list(aggs) + [(AggregateFunc.Min, len(cols))]
    ref = orc.aggregate([ocols], oaggs, group_nodes=[node_column(len(cols))], pred_nodes=pred)[0]
    assert ref[0].length == len(tuples), f"{what}: oracle has {ref[0].length} groups, model {len(tuples)}"
    order = np.argsort(ref[-1].to_numpy(), kind="stable")
    for j, (func, _) in enumerate(aggs):
        e = Column.from_numpy(np.ascontiguousarray(ref[j].to_numpy()[order]))
        assert_column_equal(got[len(keys) + j], e, rtol=rtol if func in (AggregateFunc.Sum, AggregateFunc.Avg) else None, what=f"{what} aggregate {j} vs oracle")
    return got


def int_table(rng, n, cards, nullable=(), utf8=()):
    """key columns of the given cardinalities (a negative one: values below zero too), then an integer-valued Float64 value column"""
    cols = []
    for i, c in enumerate(cards):
        a = rng.integers(0, abs(c), n).astype(np.int64)
        if c < 0:
            a = a - abs(c) // 2
        mask = rng.random(n) > 0.2 if i in nullable else None
        if i in utf8:
            cols.append(gku.utf8_column([b"k%d" % v for v in a], mask))
        else:
            cols.append(Column.from_numpy(a, mask))
    cols.append(Column.from_numpy(rng.integers(-50, 50, n).astype(np.float64)))
    return cols


# ----------------------------------------------------------------------------- row counts, both paths
GRID_ROWS_PACK = 256 * 8 * 256 * 2 * 4  # the ranges kernel's full grid: 2048 blocks x 256 lanes x 2 rows x 4 loads (the pack kernel's is half of it)
GRID_ROWS_DICT = 256 * 8 * 256


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097])
def test_row_counts_on_both_paths(ctx, orc, n):
    rng = np.random.default_rng(100 + n)
    cols = int_table(rng, n, [7, -5], nullable=(1,))
    check(ctx, orc, cols, [0, 1], aggs_over(2), path="pack", what=f"packed n={n}")
    wide = int_table(rng, n, [7, 3])
    if n:
        wide[1].values[0] = I64.min
        wide[1].values[n - 1] = I64.max if n > 1 else I64.min
    check(ctx, orc, wide, [0, 1], aggs_over(2), path="dict" if n > 1 else None, what=f"dictionary n={n}")
    s = int_table(rng, n, [7, 5], nullable=(0,), utf8=(1,))
    check(ctx, orc, s, [0, 1], aggs_over(2), path="dict", what=f"utf8 n={n}")


def sorted_groups_np(key_arrays, v):
    """vectorised model for the large cases: keys without NULLs, exact integer-valued values → (key columns, count, sum)"""
    order = np.lexsort(key_arrays[::-1])
    ks = [a[order] for a in key_arrays]
    new = np.ones(len(order), dtype=bool)
    new[1:] = np.logical_or.reduce([k[1:] != k[:-1] for k in ks])
    starts = np.nonzero(new)[0]
    return [k[starts] for k in ks], np.diff(np.append(starts, len(order))).astype(np.uint64), np.add.reduceat(v[order], starts)


@pytest.mark.parametrize("path", ["pack", "dict"])
def test_a_second_trip_of_the_grid_stride_loops(ctx, path):
    n = (GRID_ROWS_PACK if path == "pack" else GRID_ROWS_DICT) + 4097
    rng = np.random.default_rng(7)
    a = rng.integers(-3, 4, n).astype(np.int64)
    b = rng.integers(0, 5, n).astype(np.uint64)
    if path == "dict":
        b[rng.integers(0, n, 3)] = np.uint64(2**64 - 1)
        a[5], a[n - 6] = I64.min, I64.max
    v = rng.integers(0, 100, n).astype(np.float64)
    t = ctx.table_from_host([Column.from_numpy(a), Column.from_numpy(b), Column.from_numpy(v)])
    ctx.timing_reset()
    out = ctx.group_aggregate(t, [[node_column(0)], [node_column(1)]], [(AggregateFunc.Count, 2), (AggregateFunc.Sum, 2)])
    assert path_taken(ctx) == path
    got = out.to_host()
    ek, ecount, esum = sorted_groups_np([a, b], v)
    assert got[0].dtype == DType.INT64 and got[1].dtype == DType.UINT64
    assert (got[0].to_numpy() == ek[0]).all() and (got[1].to_numpy() == ek[1]).all()
    assert (got[2].to_numpy() == ecount).all() and (got[3].to_numpy() == esum).all()


# ----------------------------------------------------------------------------- key counts and tuple shapes
@pytest.mark.parametrize("k", [1, 2, 3, 8])
def test_key_counts(ctx, orc, k):
    rng = np.random.default_rng(200 + k)
    cols = int_table(rng, 3000, [3] * k)
    check(ctx, orc, cols, list(range(k)), aggs_over(k), path="pack" if k > 1 else "none", what=f"{k} keys")
    # eight keys of 2^8 values each span 2^64: the dictionary
    if k == 8:
        wide = int_table(rng, 3000, [256] * k)
        for c in range(k):
            wide[c].values[c], wide[c].values[100 + c] = 0, 255
        check(ctx, orc, wide, list(range(k)), aggs_over(k), path="dict", what="8 wide keys")


def test_tuple_shapes(ctx, orc):
    f = lambda *a: Column.from_numpy(np.array(a, dtype=np.float64))  # noqa: E731
    i = lambda *a: Column.from_numpy(np.array(a, dtype=np.int64))  # noqa: E731
    u = lambda *a: Column.from_numpy(np.array(a, dtype=np.uint64))  # noqa: E731
    # (1, 2) against (2, 1); tuples that differ only in the first key, or only in the last
    got = check(ctx, orc, [i(1, 2, 1, 2, 1, 3), i(2, 1, 2, 1, 1, 1), f(1, 2, 3, 4, 5, 6)], [0, 1], aggs_over(2), path="pack", what="(1,2) vs (2,1)")
    assert gku.key_values(got[0]) == [1, 1, 2, 3] and gku.key_values(got[1]) == [1, 2, 1, 1]
    for keys in ([0, 1], [1, 0]):
        check(ctx, orc, [i(1, 2, 1, 2, 1, 3), i(2, 1, 2, 1, 1, 1), f(1, 2, 3, 4, 5, 6)], keys, aggs_over(2), path="pack", what=f"keys {keys}")
    # every row a distinct tuple; two tuples in all
    n = 1000
    check(ctx, orc, [Column.from_numpy(np.arange(n, dtype=np.int64) // 10), Column.from_numpy(np.arange(n, dtype=np.int64) % 10), Column.from_numpy(np.arange(n, dtype=np.float64))],
          [0, 1], aggs_over(2), path="pack", what="all distinct")
    check(ctx, orc, [i(*([5] * 500)), Column.from_numpy((np.arange(500) % 2).astype(np.int64)), Column.from_numpy(np.arange(500, dtype=np.float64))], [0, 1], aggs_over(2), path="pack",
          what="two tuples")
    # negative minima; INT64_MIN and INT64_MAX in one key (the dictionary); a UInt64 above 2^63; mixed Int64 + UInt64
    check(ctx, orc, [i(-7, -7, -9, 3, -9), i(-1, -1, 4, 4, 4), f(1, 2, 3, 4, 5)], [0, 1], aggs_over(2), path="pack", what="negative minima")
    got = check(ctx, orc, [i(I64.min, I64.max, I64.min, 0, I64.max), i(1, 2, 1, 2, 2), f(1, 2, 3, 4, 5)], [0, 1], aggs_over(2), path="dict", what="int64 extremes")
    assert gku.key_values(got[0]) == [I64.min, 0, I64.max]
    big = 2**63 + 5
    got = check(ctx, orc, [u(big, 3, big, big + 1, 3), i(-2, -2, -2, 7, 7), f(1, 2, 3, 4, 5)], [0, 1], aggs_over(2), path="dict", what="uint64 above 2^63 beside small values")
    assert gku.key_values(got[0]) == [3, 3, big, big + 1]  # unsigned order
    check(ctx, orc, [u(big, big + 2, big, big + 1, big + 2), i(-2, -2, -2, 7, 7), f(1, 2, 3, 4, 5)], [0, 1], aggs_over(2), path="pack", what="uint64 minimum above 2^63, packed")
    # an expression key (`id % 4`, negative ids included) beside a column key
    ids = Column.from_numpy(np.arange(-20, 20, dtype=np.int64))
    check(ctx, orc, [ids, Column.from_numpy((np.arange(40) % 3).astype(np.int64)), Column.from_numpy(np.arange(40, dtype=np.float64))], [Key(0, mod=4), 1], aggs_over(2), path="pack",
          what="id % 4 beside a column")


def test_utf8_keys(ctx, orc):
    # lengths 0, 7, 8, 9 and a shared 8-byte prefix
    strs = [b"", b"abcdefg", b"abcdefgh", b"abcdefghi", b"abcdefghj", b"abcdefgh", b"", b"abcdefg", b"abcdefgi"]
    s = gku.utf8_column(strs)
    n = len(strs)
    a = Column.from_numpy((np.arange(n) % 2).astype(np.int64))
    v = Column.from_numpy(np.arange(n, dtype=np.float64))
    got = check(ctx, orc, [s, a, v], [0, 1], aggs_over(2), path="dict", what="utf8 first")
    assert gku.key_values(got[0]) == sorted(gku.key_values(got[0]))  # byte order, the shorter string first on a common prefix
    check(ctx, orc, [s, a, v], [1, 0], aggs_over(2), path="dict", what="utf8 last")
    check(ctx, orc, [s, a, v], [0, 1, 0], aggs_over(2), path="dict", what="utf8 first and last")
    # the empty string against NULL; a NULL slot whose bytes equal a real key
    mask = np.array([True, True, False, True, True, False, True, False, True])
    sn = gku.utf8_column(strs, mask)
    got = check(ctx, orc, [sn, a, v], [0, 1], aggs_over(2), path="dict", what="utf8 with NULLs")
    assert b"" in gku.key_values(got[0])
    got = check(ctx, orc, [sn, v], [0, 0], aggs_over(1), path="dict", what="the same utf8 column twice")
    assert gku.key_values(got[0]) == gku.key_values(got[1])


def test_null_keys(ctx, orc):
    rng = np.random.default_rng(5)
    n = 777
    for pos in range(3):  # a NULL in each key position
        cols = int_table(rng, n, [4, 3, 5], nullable=(pos,))
        cols[pos].values[~cols[pos].valid_mask()] = 2  # the NULL slots hold a real key
        check(ctx, orc, cols, [0, 1, 2], aggs_over(3), path="pack", what=f"NULLs in key {pos}")
        cols[0].values[0], cols[0].values[1] = I64.min, I64.max  # … and on the dictionary path
        m = cols[0].validity
        if m is not None:
            m[0] |= 3
        check(ctx, orc, cols, [0, 1, 2], aggs_over(3), path="dict", what=f"NULLs in key {pos}, dictionary")
    # a NULL slot outside the range of the valid keys must not widen the codes or reach a table
    a = Column.from_numpy(np.array([1, 2, I64.max, 1, I64.min, 2], dtype=np.int64), mask=np.array([1, 1, 0, 1, 0, 1], dtype=bool))
    b = Column.from_numpy(np.array([5, 5, 5, 6, 6, 6], dtype=np.int64))
    check(ctx, orc, [a, b, Column.from_numpy(np.arange(6, dtype=np.float64))], [0, 1], aggs_over(2), path="pack", what="wild NULL slots")
    # an all-NULL key column: 0 groups, every column present
    z = Column.from_numpy(np.zeros(100, dtype=np.int64), mask=np.zeros(100, dtype=bool))
    cols = [z, Column.from_numpy(np.arange(100, dtype=np.int64) % 3), Column.from_numpy(np.ones(100))]
    got = check(ctx, orc, cols, [0, 1], aggs_over(2), path="pack", what="all-NULL key")
    assert len(got) == 7 and all(c.length == 0 for c in got) and got[2].dtype == DType.UINT64
    zs = gku.utf8_column([b"x"] * 100, np.zeros(100, dtype=bool))
    got = check(ctx, orc, [zs, cols[1], cols[2]], [1, 0], aggs_over(2), path="dict", what="all-NULL utf8 key")
    assert all(c.length == 0 for c in got) and got[1].dtype == DType.UTF8
    # a validity buffer with null_count 0
    full = Column.from_numpy(np.arange(130, dtype=np.int64) % 4, mask=np.ones(130, dtype=bool))
    check(ctx, orc, [full, Column.from_numpy(np.arange(130, dtype=np.int64) % 3), Column.from_numpy(np.ones(130))], [0, 1], aggs_over(2), path="pack", what="full validity")


def test_null_values_follow_q10(ctx, orc):
    # group (1, 1) has only NULL values: count 0, sum 0.0, avg NaN, min f64::MAX, max f64::MIN
    a = Column.from_numpy(np.array([1, 1, 2, 2], dtype=np.int64))
    b = Column.from_numpy(np.array([1, 1, 1, 1], dtype=np.int64))
    v = Column.from_numpy(np.array([9.0, 9.0, 3.0, 4.0]), mask=np.array([0, 0, 1, 1], dtype=bool))
    got = check(ctx, orc, [a, b, v], [0, 1], aggs_over(2), path="pack", what="all-NULL values")
    row = [got[2 + j].to_numpy()[0] for j in range(5)]
    assert row[0] == 0 and row[1] == 0.0 and np.isnan(row[2]) and row[3] == gku.F64_MAX and row[4] == -gku.F64_MAX
    vi = Column.from_numpy(np.array([9, 9, 3, -4], dtype=np.int64), mask=np.array([0, 0, 1, 1], dtype=bool))
    check(ctx, orc, [a, b, vi], [0, 1], aggs_over(2), path="pack", what="Int64 values (Q10: as f64)")


def test_predicates(ctx, orc):
    rng = np.random.default_rng(11)
    n = 2000
    cols = int_table(rng, n, [5, 4])
    cols.append(Column.from_numpy(rng.integers(0, 10, n).astype(np.int64), mask=rng.random(n) > 0.3))  # the predicate's column, with NULLs (Q4)
    fl = fields_of(cols)
    pv, pm = cols[3].to_numpy(), cols[3].valid_mask()
    pred = binop(col(3), Operator.Lt, lit_i64(5)).flatten(fl)
    keep = pm & (pv < 5)
    for path, keys in (("pack", [0, 1]), ("dict", None)):
        c2 = list(cols)
        if keys is None:
            c2[1] = gku.utf8_column([b"s%d" % x for x in cols[1].to_numpy()])
            keys = [0, 1]
        got = check(ctx, orc, c2, keys, aggs_over(2), pred=pred, keep=keep, path=path, what=f"predicate with NULLs ({path})")
        assert got[0].length == 20
        # a predicate that rejects everything
        none = binop(col(3), Operator.Lt, lit_i64(-1)).flatten(fl)
        got = check(ctx, orc, c2, keys, aggs_over(2), pred=none, keep=np.zeros(n, dtype=bool), path=path, what="rejects everything")
        assert all(c.length == 0 for c in got) and len(got) == 7
    # a tuple whose rows are all rejected must not appear
    k0 = cols[0].to_numpy()
    only = binop(col(0), Operator.NotEq, lit_i64(4)).flatten(fl)
    got = check(ctx, orc, cols, [0, 1], aggs_over(2), pred=only, keep=k0 != 4, path="pack", what="a rejected tuple")
    assert 4 not in gku.key_values(got[0]) and got[0].length == 16
    # a predicate over the value column beside an expression key
    vp = binop(col(2), Operator.GtEq, lit_f64(0.0)).flatten(fl)
    check(ctx, orc, cols, [Key(0, mod=3), 1], aggs_over(2), pred=vp, keep=cols[2].to_numpy() >= 0.0, path="pack", what="predicate on the values")


def test_fractional_values_within_the_project_tolerance(ctx, orc):
    rng = np.random.default_rng(3)
    n = 20000
    cols = int_table(rng, n, [6, 7])
    cols[2] = Column.from_numpy(rng.random(n) * 100.0)
    check(ctx, orc, cols, [0, 1], aggs_over(2), path="pack", rtol=1e-9, what="fractional values")


# ----------------------------------------------------------------------------- against the existing call
@pytest.mark.parametrize("dtype", ["int64", "uint64", "utf8"])
def test_one_key_against_the_existing_call(ctx, dtype):
    rng = np.random.default_rng(21)
    n = 5000
    raw = rng.integers(0, 50, n)
    if dtype == "utf8":
        # (NULL slots hold bytes no valid row has: the existing call's keys_out takes each string from its representative row, which
        # may be a NULL slot with the same bytes — it then reports a NULL; the grouped call never makes a NULL row a representative)
        mask = rng.random(n) > 0.1
        key = gku.utf8_column([b"key-%02d" % x if ok else b"null slot" for x, ok in zip(raw, mask)], mask)
    else:
        key = Column.from_numpy((raw.astype(np.int64) - 25) if dtype == "int64" else raw.astype(np.uint64) + np.uint64(2**63), mask=rng.random(n) > 0.1)
    cols = [key, Column.from_numpy(rng.integers(-9, 9, n).astype(np.float64), mask=rng.random(n) > 0.1)]
    t = ctx.table_from_host(cols)
    aggs = aggs_over(1)
    ctx.timing_reset()
    out = ctx.group_aggregate(t, [[node_column(0)]], aggs).to_host()
    assert path_taken(ctx) == ("dict" if dtype == "utf8" else "none")  # integer keys forward; a Utf8 key takes the tuple dictionary
    ref, ref_keys = ctx.aggregate(t, aggs, group_nodes=[node_column(0)], with_keys=True)
    ref, ref_keys = ref.to_host(), ref_keys.to_host()[0]
    ref_vals = gku.key_values(ref_keys)
    order = np.arange(ref_keys.length)
    if dtype == "utf8":  # the existing call leaves the strings in the order of their codes: sort them
        order = np.array(sorted(range(ref_keys.length), key=lambda i: ref_vals[i]), dtype=np.int64)
    assert out[0].dtype == ref_keys.dtype and out[0].validity is None
    assert gku.key_values(out[0]) == [ref_vals[i] for i in order]
    for j, (func, _) in enumerate(aggs):
        e = Column.from_numpy(np.ascontiguousarray(ref[j].to_numpy()[order]))
        assert_column_equal(out[1 + j], e, rtol=1e-9 if func in (AggregateFunc.Sum, AggregateFunc.Avg) else None, what=f"aggregate {j}")
    # an expression key keeps its tier: the same kernels as the existing call
    ids = Column.from_numpy(np.arange(n, dtype=np.int64))
    t2 = ctx.table_from_host([ids, cols[1]])
    knodes = binop(col(0), Operator.Modulos, lit_i64(1024)).flatten(fields_of([ids, cols[1]]))
    ctx.group_aggregate(t2, [knodes], aggs)  # (both once, so that what the context remembers of the query has settled)
    ctx.aggregate(t2, aggs, group_nodes=knodes, with_keys=True)
    ctx.timing_reset()
    a = ctx.group_aggregate(t2, [knodes], aggs).to_host()
    mine = {k for k in ctx.timing_report() if k.startswith("agg")}
    ctx.timing_reset()
    b, bk = ctx.aggregate(t2, aggs, group_nodes=knodes, with_keys=True)
    theirs = {k for k in ctx.timing_report() if k.startswith("agg")}
    assert mine == theirs and mine
    assert (a[0].to_numpy() == bk.to_host()[0].to_numpy()).all()
    for j in range(len(aggs)):
        assert_column_equal(a[1 + j], b.to_host()[j], what=f"id % 1024 aggregate {j}")


def test_output_is_sorted_and_two_calls_give_identical_bytes(ctx):
    rng = np.random.default_rng(31)
    n = 10000
    for cols, keys in ((int_table(rng, n, [-40, 30, 20]), [0, 1, 2]), (int_table(rng, n, [40, 30], utf8=(0,)), [0, 1]), (int_table(rng, n, [40, 30], utf8=(1,)), [1, 0])):
        t = ctx.table_from_host(cols)
        nodes = [[node_column(c)] for c in keys]
        a = ctx.group_aggregate(t, nodes, aggs_over(len(cols) - 1)).to_host()
        b = ctx.group_aggregate(t, nodes, aggs_over(len(cols) - 1)).to_host()
        tuples = list(zip(*[gku.key_values(a[i]) for i in range(len(keys))]))
        assert tuples == sorted(tuples) and len(set(tuples)) == len(tuples)
        for x, y in zip(a, b):
            assert x.values.tobytes() == y.values.tobytes() and (x.data is None or x.data.tobytes() == y.data.tobytes())


# ----------------------------------------------------------------------------- the mirrors
def test_grouped_plan_over_a_multi_batch_child_fused_and_unfused(ctx):
    from naive_query_engine_amd import ColumnExpr, physical_plan as pp
    from naive_query_engine_amd.rewrite import FusedSelectionGroupedAggregatePlan, NaiveDB, plan_shape, rewrite

    rng = np.random.default_rng(41)
    schema = [Field("a", DType.INT64, False), Field("s", DType.UTF8, False), Field("v", DType.FLOAT64, False)]

    def batch(n):
        return RecordBatch(schema, [Column.from_numpy(rng.integers(0, 4, n).astype(np.int64)), gku.utf8_column([b"s%d" % x for x in rng.integers(0, 3, n)]),
                                    Column.from_numpy(rng.integers(0, 9, n).astype(np.float64))])

    def rows(batches):
        assert len(batches) == 1
        return [c.to_list() for c in batches[0].to_host().columns], [f.name for f in batches[0].fields]

    keys = [pp.ColumnExpr.try_create("s", None), binop(col("a"), Operator.Modulos, lit_i64(3))]
    ops = [pp.Count.create(ColumnExpr.try_create("v", None)), pp.Sum.create(ColumnExpr.try_create("v", None))]
    pred = binop(col("v"), Operator.Gt, lit_f64(2.0))
    for batches in ([batch(500)], [batch(300), batch(200), batch(7)]):
        scan = pp.ScanPlan.create(pp.MemTable.try_create(schema, batches, ctx), None)
        plain = pp.GroupedAggregatePlan.create(keys, ops, scan)
        assert [f.name for f in plain.schema()] == ["s", "group_1", "count(v)", "sum(v)"]
        got, names = rows(plain.execute())
        assert names == ["s", "group_1", "count(v)", "sum(v)"]
        # the model over the concatenated batches
        s = [x for b in batches for x in gku.key_values(b.columns[1])]
        a = np.concatenate([b.columns[0].to_numpy() for b in batches])
        v = np.concatenate([b.columns[2].to_numpy() for b in batches])
        tuples, exp, _ = gku.model([s, [int(x) % 3 for x in a]], [None, None, Column.from_numpy(v)], [(AggregateFunc.Count, 2), (AggregateFunc.Sum, 2)])
        assert [x.encode() for x in got[0]] == [t[0] for t in tuples] and got[1] == [t[1] for t in tuples]
        assert got[2] == exp[0].tolist() and got[3] == exp[1].tolist()
        tree = pp.GroupedAggregatePlan.create(keys, ops, pp.SelectionPlan.create(scan, pred))
        fused = rewrite(tree)
        assert isinstance(fused, FusedSelectionGroupedAggregatePlan) and plan_shape(fused) == ["FusedSelectionGroupedAggregatePlan", "ScanPlan"]
        assert rows(fused.execute()) == rows(tree.execute())
        db = NaiveDB()
        assert rows(db.run_plan(tree)) == rows(tree.execute())
        if len(batches) == 1:  # (several batches: the selection's predicate comes from batch 0, quirk Q3 — not the model's business)
            tuples, exp, _ = gku.model([s, [int(x) % 3 for x in a]], [None, None, Column.from_numpy(v)], [(AggregateFunc.Count, 2), (AggregateFunc.Sum, 2)], keep=v > 2.0)
            got, _ = rows(fused.execute())
            assert [x.encode() for x in got[0]] == [t[0] for t in tuples] and got[3] == exp[1].tolist()


def test_golden_group_by_through_the_python_mirror(ctx):
    from naive_query_engine_amd import ColumnExpr, physical_plan as pp

    with open(os.path.join(GOLDEN, "group_keys_expected.json")) as f:
        doc = json.load(f)
    data = pp.CsvTable.try_create(os.path.join(GOLDEN, "test_data.csv"), None, ctx)
    keys = [binop(col("id"), Operator.Modulos, lit_i64(3)), ColumnExpr.try_create("age", None)]
    ops = [pp.Count.create(col("score")), pp.Sum.create(col("score")), pp.Min.create(col("id")), pp.Max.create(col("score"))]
    for q in doc["queries"]:
        child = pp.ScanPlan.create(data, None)
        if "where" in q["sql"]:
            child = pp.SelectionPlan.create(child, binop(col("age"), Operator.Gt, lit_i64(19)))
        out = pp.GroupedAggregatePlan.create(keys, ops, child).execute()
        assert [f.name for f in out[0].fields] == q["columns"]
        got = [c.to_list() for c in out[0].to_host().columns]
        assert [list(r) for r in zip(*got)] == q["rows"], q["name"]


# ----------------------------------------------------------------------------- errors, memory
def raw_call(ctx, table, keys, aggs, pred=None, num_keys=None, offsets=None, out=True):
    from naive_query_engine_amd import capi

    parr, pn = ctx._nodes(pred)
    garr, offs, nk = ctx._flat(keys)
    if offsets is not None:
        offs = (C.c_int32 * len(offsets))(*offsets)
    h = C.c_void_p()
    return capi.lib().nqe_group_aggregate_execute(ctx.handle, table.handle, parr, pn, garr, offs, nk if num_keys is None else num_keys, ctx._aggs(aggs), len(aggs),
                                                  C.byref(h) if out else None), h


def test_errors_are_raised_before_anything_is_allocated_or_launched(ctx):
    n = 100
    cols = [Column.from_numpy(np.arange(n, dtype=np.int64)), Column.from_numpy(np.arange(n, dtype=np.uint64)), Column.from_numpy(np.arange(n, dtype=np.float64)),
            gku.utf8_column([b"x"] * n), Column.from_numpy(np.arange(n) % 2 == 0)]
    fl = fields_of(cols)
    t = ctx.table_from_host(cols)
    empty = ctx.table_from_host([gku.utf8_column([]) if c.dtype == DType.UTF8 else Column.from_numpy(c.to_numpy()[:0]) for c in cols])
    k0, k1, kf, ks, kb = ([node_column(i)] for i in range(5))
    good = [(AggregateFunc.Sum, 2)]
    div0 = binop(col(0), Operator.Divide, binop(col(0), Operator.Minus, col(0))).flatten(fl)
    cases = [
        ("no keys", dict(keys=[], aggs=good), Status.PlanError),
        ("negative key count", dict(keys=[k0], aggs=good, num_keys=-1), Status.PlanError),
        ("nine keys", dict(keys=[k0] * 9, aggs=good), Status.NotSupported),
        ("offsets that do not ascend", dict(keys=[k0, k1], aggs=good, offsets=[0, 2, 1]), Status.InvalidArgument),
        ("an empty key", dict(keys=[k0, k1], aggs=good, offsets=[0, 0, 2]), Status.InvalidArgument),
        ("a NULL out", dict(keys=[k0, k1], aggs=good, out=False), Status.InvalidArgument),
        ("a Float64 key", dict(keys=[k0, kf], aggs=good), Status.NotSupported),
        ("a Boolean key", dict(keys=[kb, k0], aggs=good), Status.NotSupported),
        ("a Utf8 key that is not a bare column", dict(keys=[k0, lit_utf8("x").flatten(fl)], aggs=good), Status.NotSupported),
        ("an unknown aggregate function", dict(keys=[k0, k1], aggs=[(7, 2)]), Status.NoMatchFunction),
        ("an aggregate column out of range", dict(keys=[k0, k1], aggs=[(AggregateFunc.Sum, 9)]), Status.NotSupported),
        ("sum over a Utf8 column", dict(keys=[k0, k1], aggs=[(AggregateFunc.Sum, 3)]), Status.NotSupported),
        ("a predicate that is no Boolean", dict(keys=[k0, k1], aggs=good, pred=k0), Status.NotSupported),
        ("a predicate with mismatched operands", dict(keys=[k0, k1], aggs=good, pred=binop(col(0), Operator.Lt, col(2)).flatten(fl)), Status.IntervalError),
    ]
    for tab, where in ((t, "rows"), (empty, "0 rows")):
        for name, kw, status in cases:
            live = ctx.memory_stats()[0]
            ctx.timing_reset()
            st, h = raw_call(ctx, tab, **kw)
            assert st == int(status), f"{name} ({where}): status {st}, expected {int(status)}"
            assert not h.value and ctx.timing_query("")[1] == 0 and ctx.memory_stats()[0] == live, f"{name} ({where}): something ran"
    # the same arguments give nqe_aggregate_execute's status where the existing call has one
    for name, kw, status in cases[9:]:
        with pytest.raises(ErrorCode) as e:
            ctx.aggregate(t, kw["aggs"], group_nodes=k0, pred_nodes=kw.get("pred"))
        assert e.value.status == status, name
    # a key expression that faults reports what nqe_expr_evaluate reports
    with pytest.raises(ErrorCode) as e1:
        ctx.expr_evaluate(t, div0)
    with pytest.raises(ErrorCode) as e2:
        ctx.group_aggregate(t, [k1, div0], good)
    assert e1.value.status == e2.value.status == Status.ArrowError and str(e1.value) == str(e2.value)
    # … and sees only the rows a predicate keeps: a divisor the filter excludes does not fault
    safe = binop(col(0), Operator.Divide, col(0)).flatten(fl)
    out = ctx.group_aggregate(t, [k1, safe], good, pred_nodes=binop(col(0), Operator.Gt, lit_i64(0)).flatten(fl)).to_host()
    assert out[0].length == n - 1 and set(out[1].to_numpy().tolist()) == {1}


def test_live_bytes_return_to_their_start(ctx):
    rng = np.random.default_rng(51)
    gc.collect()
    ctx.synchronize()
    live0 = ctx.memory_stats()[0]
    cols = int_table(rng, 5000, [9, 8, 7], nullable=(1,))
    t = ctx.table_from_host(cols)
    s = ctx.table_from_host(int_table(rng, 5000, [9, 8], utf8=(0,)))
    outs = [ctx.group_aggregate(t, [[node_column(0)], [node_column(1)], [node_column(2)]], aggs_over(3)),
            ctx.group_aggregate(s, [[node_column(0)], [node_column(1)]], aggs_over(2)),
            ctx.group_aggregate(t, [[node_column(0)]], aggs_over(3))]
    assert ctx.memory_stats()[0] > live0
    for o in outs:
        o.release()
    t.release()
    s.release()
    gc.collect()
    assert ctx.memory_stats()[0] == live0


# ----------------------------------------------------------------------------- a seeded sweep
def _random_case(seed):
    rng = np.random.default_rng(9000 + seed)
    n = int(rng.choice([0, 1, 2, 63, 65, 500, 4097, 20000]))
    k = int(rng.integers(1, 9))
    cols, keys = [], []
    for i in range(k):
        kind = rng.choice(["i64", "u64", "utf8", "wide"], p=[0.4, 0.25, 0.2, 0.15])
        card = int(rng.choice([1, 2, 5, 40]))
        raw = rng.integers(0, card, n)
        mask = (rng.random(n) > rng.choice([0.02, 0.3])) if rng.random() < 0.25 else None
        if kind == "utf8":
            cols.append(gku.utf8_column([b"v" * int(x % 3) + b"%d" % x for x in raw], mask))
        elif kind == "u64":
            cols.append(Column.from_numpy(raw.astype(np.uint64) + np.uint64([0, 2**63 - 2, 2**64 - 50][int(rng.integers(0, 3))]), mask))
        elif kind == "wide":
            cols.append(Column.from_numpy(np.where(raw % 2 == 0, I64.min + raw, I64.max - raw).astype(np.int64), mask))
        else:
            cols.append(Column.from_numpy(raw.astype(np.int64) - int(rng.choice([0, 3, 10**12])), mask))
        keys.append(Key(i, mod=int(rng.choice([2, 3, 7]))) if kind == "i64" and rng.random() < 0.25 else Key(i))
    vmask = (rng.random(n) > 0.2) if rng.random() < 0.5 else None
    cols.append(Column.from_numpy(rng.integers(-1000, 1000, n).astype(np.float64), vmask))
    cols.append(Column.from_numpy(rng.integers(0, 100, n).astype(np.int64), (rng.random(n) > 0.1) if rng.random() < 0.5 else None))
    aggs = [(f, k + int(rng.integers(0, 2))) for f, _ in ALL]
    pred = keep = None
    if rng.random() < 0.6:
        cut = int(rng.choice([-1, 30, 70, 200], p=[0.1, 0.3, 0.3, 0.3]))
        pred = binop(col(k + 1), Operator.Lt, lit_i64(cut)).flatten(fields_of(cols))
        keep = cols[k + 1].valid_mask() & (cols[k + 1].to_numpy() < cut)
    return cols, keys, aggs, pred, keep


@pytest.mark.parametrize("chunk", range(8))
def test_seeded_sweep(ctx, orc, chunk):
    for seed in range(chunk * 4, chunk * 4 + 4):
        cols, keys, aggs, pred, keep = _random_case(seed)
        check(ctx, orc, cols, keys, aggs, pred=pred, keep=keep, what=f"seed {seed}")
