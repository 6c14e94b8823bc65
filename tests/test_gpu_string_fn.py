"""GPU: the string functions of an NQE_EXPR_STRING node (quirk Q25: trim / ltrim / rtrim, lower / upper, character_length, reverse)
through nqe_expr_evaluate, every operator that takes expression trees, and the Python plan mirror — against the plain-Python model of
tests/string_fn_util.py.  Every comparison is bit for bit: the offsets relative to offsets[0], the bytes between them, the Int64 words,
the validity bits and null_count.  The kernels never read validity, so the bytes under a NULL are compared like any other."""
import ctypes as C
from collections import Counter

import numpy as np
import pytest

from tests.helpers import fields
from tests.string_fn_util import (CONTENTS, INVALID, LENGTH, LENGTH_PRESERVING, LENGTHS, LOWER, LTRIM, REVERSE, ROW_COUNTS, RTRIM, STRING_FUNCTIONS, TRIM, TRIMS, UPPER,
                                  byte_strings, model, relative_offsets, sized, utf8_column)

pytestmark = pytest.mark.gpu

F = fields("s")
# what each function may launch: the labels of DESIGN §3.19 (the scan's own kernels are sort.hip's: scan_single / scan_chunk / scan_add)
LABELS = {LOWER: {"str_case"}, UPPER: {"str_case"}, REVERSE: {"str_reverse"}, LENGTH: {"str_length"},
          TRIM: {"str_trim_bounds", "str_trim_copy"}, LTRIM: {"str_trim_bounds", "str_trim_copy"}, RTRIM: {"str_trim_bounds", "str_trim_copy"}}


@pytest.fixture(scope="module")
def ctx():
    from naive_query_engine_amd import capi

    c = capi.Context(0)
    yield c
    c.close()


def strfn(func, e):
    from naive_query_engine_amd.expression import strop

    return strop(func, e)


def col(i):
    from naive_query_engine_amd.expression import col as c

    return c(i)


def evaluate(ctx, t, func, column=0, names=F):
    return ctx.expr_evaluate(t, strfn(func, col(column)).flatten(names))


def assert_result(got, items, func, mask=None, what=""):
    """`got`: the downloaded result column; items: the operand's byte strings (NULL slots included); mask: the operand's validity"""
    from naive_query_engine_amd import DType

    n = len(items)
    assert got.length == n, (what, got.length, n)
    exp = [model(func, s) for s in items]
    if func == LENGTH:
        assert got.dtype == DType.INT64, what
        g = got.to_numpy()
        assert g.dtype == np.int64 and (g == np.array(exp, dtype=np.int64)).all(), (what, func.name, np.nonzero(g != np.array(exp, dtype=np.int64))[0][:8])
    else:
        assert got.dtype == DType.UTF8, what
        lens = np.array([len(s) for s in exp], dtype=np.int64)
        rel = relative_offsets(got)
        assert len(rel) == n + 1 and (rel == np.concatenate([[0], np.cumsum(lens)])).all(), (what, func.name, "offsets")
        blob = b"".join(exp)
        raw = bytes(got.data.tobytes()) if got.data is not None else b""
        first = int(got.values[0])
        if raw[first: first + len(blob)] != blob or len(raw) < first + len(blob):
            gs = byte_strings(got)
            bad = [i for i in range(n) if gs[i] != exp[i]]
            raise AssertionError((what, func.name, bad[:8], [(items[i], gs[i], exp[i]) for i in bad[:3]]))
    valid = got.valid_mask()
    assert (valid == (np.ones(n, dtype=bool) if mask is None else np.asarray(mask, dtype=bool))).all(), (what, func.name, "validity")


def check_all(ctx, items, mask=None, what="", funcs=STRING_FUNCTIONS):
    t = ctx.table_from_host([utf8_column(items, mask)])
    for func in funcs:
        out = evaluate(ctx, t, func)
        assert_result(out.to_host()[0], items, func, mask, what)
        assert out.column_info(0).null_count == (0 if mask is None else int((~np.asarray(mask)).sum())), (what, func.name)
    return t


# ----------------------------------------------------------------------------- shapes
@pytest.mark.parametrize("length", LENGTHS)
def test_every_string_length(ctx, length):
    """65 rows of exactly `length` bytes: the mean picks the lanes per string (<= 32: 4, <= 96: 8, <= 256: 16, <= 1024: 32, else 64), the
    length the split between 8-byte words and the byte tail, the total the head / body / tail of str_case"""
    check_all(ctx, [sized(length, seed) for seed in range(65)], what=f"length {length}")


@pytest.mark.parametrize("n", ROW_COUNTS)
def test_every_row_count(ctx, n):
    pool = CONTENTS + [sized(L, 3) for L in (1, 9, 17, 33)]
    items = [pool[(i * 7) % len(pool)] for i in range(n)]
    t = check_all(ctx, items, what=f"{n} rows")
    if n == 0:  # a well-formed 0-row column of the right type
        from naive_query_engine_amd import DType

        for func in STRING_FUNCTIONS:
            c = evaluate(ctx, t, func).to_host()[0]
            assert c.length == 0 and c.dtype == (DType.INT64 if func == LENGTH else DType.UTF8)


def test_contents(ctx):
    """spaces everywhere they matter, the whitespace that is kept, code points across byte 8 and 16 of a string and (the strings lie back to
    back) of the data buffer, the neighbours of the letter ranges, bytes >= 0x80"""
    check_all(ctx, CONTENTS, what="contents")
    check_all(ctx, list(reversed(CONTENTS)), what="contents reversed")     # the same strings at other positions of the buffer
    check_all(ctx, [b"abc"] + CONTENTS, what="contents shifted by 3")


def test_all_empty_and_all_spaces_columns(ctx):
    check_all(ctx, [b""] * 130, what="all empty")
    check_all(ctx, [b" " * (i % 40) for i in range(130)], what="all spaces")
    check_all(ctx, [b" " * 300 + b"x"] * 5 + [b"y" + b" " * 2000] * 3, what="long runs")


def test_invalid_utf8_between_valid_neighbours(ctx):
    items = []
    for bad in INVALID:
        items += ["né日".encode(), bad, b" ok "]
    check_all(ctx, items, what="invalid utf-8")
    # the two cases of the specification, spelled out
    t = ctx.table_from_host([utf8_column([b"ab", b"\xa9" * 6, b"cd", b"\xc3" + b"\xa9" * 5, b"ef"])])
    assert byte_strings(evaluate(ctx, t, REVERSE).to_host()[0]) == [b"ba", b"\xa9" * 6, b"dc", b"\xa9\xa9\xc3\xa9\xa9\xa9", b"fe"]
    assert evaluate(ctx, t, LENGTH).to_host()[0].to_numpy().tolist() == [2, 0, 2, 1, 2]


@pytest.mark.parametrize("func", [LOWER, REVERSE, LENGTH, TRIM], ids=lambda f: f.name)
def test_second_step_of_every_grid_stride_loop(ctx, func):
    """600 001 rows of short strings: at 4 lanes per string a workgroup takes 64 strings per step and the grid is capped at 4 workgroups
    per compute unit, str_case's grid covers 4 MiB per step — every loop goes round again (str_trim_copy under TRIM)"""
    n = 600_001
    rng = np.random.default_rng(11)
    pool = [sized(int(L), k) for k, L in enumerate(rng.integers(4, 20, 997))]
    pick = rng.integers(0, len(pool), n)
    items = [pool[i] for i in pick]
    col0 = utf8_column(items)
    assert col0.data.size > 5_000_000
    t = ctx.table_from_host([col0])
    got = evaluate(ctx, t, func).to_host()[0]
    exp_pool = [model(func, s) for s in pool]
    if func == LENGTH:
        assert (got.to_numpy() == np.array(exp_pool, dtype=np.int64)[pick]).all()
    else:
        exp = [exp_pool[i] for i in pick]
        assert (relative_offsets(got) == np.concatenate([[0], np.cumsum([len(s) for s in exp])])).all()
        assert bytes(got.data.tobytes())[: int(got.values[n])] == b"".join(exp)


# ----------------------------------------------------------------------------- layout
def borrowed_table(ctx, specs, keep):
    """a table over the caller's device memory (NQE_DEVICE): specs = [(length, values_ptr, validity_ptr or None, data_ptr, data_length)]"""
    from naive_query_engine_amd import DType, capi
    from naive_query_engine_amd.arrow_host import DEVICE, NqeColumn

    arr = (NqeColumn * len(specs))()
    for i, (n, values, validity, data, data_length) in enumerate(specs):
        arr[i].dtype = int(DType.UTF8)
        arr[i].location = DEVICE
        arr[i].length = n
        arr[i].null_count = -1 if validity else 0
        arr[i].values = values
        arr[i].validity = validity
        arr[i].data = data
        arr[i].data_length = data_length
    h = C.c_void_p()
    ctx.check(capi.lib().nqe_table_create_flags(ctx.handle, arr, len(specs), 0, C.byref(h)))
    t = capi.Table(ctx, h)
    t._keep = [keep]
    return t


def test_sub_range_of_a_column_and_an_odd_data_base(ctx):
    """offsets[0] != 0 with bytes before offsets[0] and past offsets[n]; and a data base address that is odd: the head of str_case's
    16-byte body, unaligned words everywhere else"""
    items = [CONTENTS[(i * 5) % len(CONTENTS)] for i in range(90)] + [sized(L, 1) for L in (7, 9, 33, 257)]
    n = len(items)
    whole = utf8_column(items)
    pad = 1
    shifted = utf8_column(items)
    shifted.values = (shifted.values + pad).astype(np.int32)                              # offsets into a buffer with one byte in front
    shifted.data = np.concatenate([np.frombuffer(b"Q", dtype=np.uint8), shifted.data])
    src = ctx.table_from_host([shifted, whole])
    a, b = src.column_info(0), src.column_info(1)
    skip, drop = 11, 7
    m = n - skip - drop
    sub = borrowed_table(ctx, [(m, a.values + 4 * skip, None, a.data, a.data_length)], src)
    odd = borrowed_table(ctx, [(n, b.values, None, a.data + pad, a.data_length - pad)], src)
    assert (a.data + pad) % 2 == 1, "the library's allocations are at least 2-byte aligned"
    for func in STRING_FUNCTIONS:
        out = evaluate(ctx, sub, func)
        assert_result(out.to_host()[0], items[skip: skip + m], func, what="sub-range")
        info = out.column_info(0)
        assert info.values != a.values + 4 * skip and info.data != a.data  # borrowed memory is never aliased by an output
        out = evaluate(ctx, odd, func)
        assert_result(out.to_host()[0], items, func, what="odd base")
    # the source is untouched
    assert byte_strings(src.to_host()[1]) == items


def test_nullable_operand_shares_validity_and_offsets(ctx):
    rng = np.random.default_rng(4)
    items = [CONTENTS[(i * 3) % len(CONTENTS)] for i in range(300)]  # non-empty strings under the NULLs, transformed like any other
    mask = rng.random(300) > 0.4
    assert any(len(s) and not ok for s, ok in zip(items, mask))
    t = check_all(ctx, items, mask, what="nullable")
    tin = t.column_info(0)
    for func in STRING_FUNCTIONS:
        out = evaluate(ctx, t, func)
        info = out.column_info(0)
        assert info.validity == tin.validity, func.name        # reference-counted alias, no copy
        assert info.null_count == int((~mask).sum())
        if func in LENGTH_PRESERVING:
            assert info.values == tin.values and info.data != tin.data, func.name   # the operand's offsets buffer, new bytes
        else:
            assert info.values != tin.values, func.name


def test_nullable_borrowed_operand_copies_validity_and_offsets(ctx):
    rng = np.random.default_rng(5)
    n = 1000
    items = [sized(int(L), k) for k, L in enumerate(rng.integers(0, 40, n))]
    mask = rng.random(n) > 0.3
    src = ctx.table_from_host([utf8_column(items, mask)])
    a = src.column_info(0)
    t = borrowed_table(ctx, [(n, a.values, a.validity, a.data, a.data_length)], src)
    for func in STRING_FUNCTIONS:
        out = evaluate(ctx, t, func)
        info = out.column_info(0)
        assert info.validity and info.validity != a.validity and info.values != a.values and info.data != a.data, func.name
        assert info.null_count == int((~mask).sum())
        assert_result(out.to_host()[0], items, func, mask, what="borrowed nullable")


# ----------------------------------------------------------------------------- launches
def launches(ctx, run):
    ctx.timing_enable(True)
    ctx.timing_reset()
    try:
        out = run()
        return out, set(ctx.timing_report())
    finally:
        ctx.timing_enable(False)


def test_launch_labels_per_function(ctx):
    items = [sized(int(L), k) for k, L in enumerate(np.random.default_rng(6).integers(0, 30, 500))]
    t = ctx.table_from_host([utf8_column(items)])
    empty_rows = ctx.table_from_host([utf8_column([])])
    empty_bytes = ctx.table_from_host([utf8_column([b""] * 77)])
    for func in STRING_FUNCTIONS:
        out, ran = launches(ctx, lambda: evaluate(ctx, t, func))
        scans = {name for name in ran if name.startswith("scan") or "exclusive_scan" in name}
        assert ran - scans == LABELS[func], (func.name, ran)
        assert bool(scans) == (func in TRIMS), (func.name, ran)  # the length-preserving functions and str_length: no scan, no copy
        assert_result(out.to_host()[0], items, func, what="labels")
        for what, tab, its in (("0 rows", empty_rows, []), ("0 bytes", empty_bytes, [b""] * 77)):
            out, ran = launches(ctx, lambda: evaluate(ctx, tab, func))
            assert ran == set(), (func.name, what, ran)
            assert_result(out.to_host()[0], its, func, what=what)
    # all spaces under a trim: the copy has nothing to move and is not launched
    spaces = ctx.table_from_host([utf8_column([b"  ", b" "])])
    out, ran = launches(ctx, lambda: evaluate(ctx, spaces, TRIM))
    assert "str_trim_bounds" in ran and "str_trim_copy" not in ran
    assert byte_strings(out.to_host()[0]) == [b"", b""]


# ----------------------------------------------------------------------------- every consumer, 257 rows
N_CONS = 257
NAMES = [b"bob", b"Bob", b" BOB ", b"alice", b"bOb", b"bobby", b"  carol", b"dave  ", "zoé".encode(), b"", b"BOB", b" bob"]


def consumer_table(ctx, nullable=False):
    from naive_query_engine_amd import Column

    rng = np.random.default_rng(8)
    items = [NAMES[int(i)] for i in rng.integers(0, len(NAMES), N_CONS)]
    ids = np.arange(N_CONS, dtype=np.int64)
    v = rng.integers(-50, 50, N_CONS).astype(np.float64)
    mask = (rng.random(N_CONS) > 0.25) if nullable else None
    t = ctx.table_from_host([Column.from_numpy(ids), utf8_column(items, mask), Column.from_numpy(v)])
    return t, ids, items, v, mask


FC = fields("id", "s", "v")


def lower_is_bob():
    from naive_query_engine_amd import Operator
    from naive_query_engine_amd.expression import binop, lit_utf8

    return binop(strfn(LOWER, col(1)), Operator.Eq, lit_utf8("bob"))


def test_selection_by_a_string_predicate(ctx):
    t, ids, items, v, _ = consumer_table(ctx)
    keep = np.array([model(LOWER, s) == b"bob" for s in items])
    assert 0 < keep.sum() < N_CONS
    got = ctx.selection(t, lower_is_bob().flatten(FC)).to_host()
    assert (got[0].to_numpy() == ids[keep]).all() and byte_strings(got[1]) == [s for s, k in zip(items, keep) if k] and (got[2].to_numpy() == v[keep]).all()
    # a NULL predicate emits a NULL row (quirk Q4): the rows whose string is NULL come out as well, as NULLs
    t, ids, items, v, mask = consumer_table(ctx, nullable=True)
    got = ctx.selection(t, lower_is_bob().flatten(FC)).to_host()
    assert got[0].length == int((keep & mask).sum() + (~mask).sum())
    assert (got[0].to_numpy()[got[0].valid_mask()] == ids[keep & mask]).all()


def test_selection_projection_with_string_nodes_in_the_predicate_the_list_or_both(ctx):
    from naive_query_engine_amd import Operator
    from naive_query_engine_amd.expression import binop, lit_i64

    t, ids, items, v, _ = consumer_table(ctx)
    bob = np.array([model(LOWER, s) == b"bob" for s in items])
    small = ids < 100
    length2 = binop(strfn(LENGTH, col(1)), Operator.Multiply, lit_i64(2))
    string_list = [strfn(TRIM, col(1)), length2, col(0), strfn(LOWER, strfn(TRIM, col(1)))]
    plain_list = [col(0), binop(col(0), Operator.Plus, lit_i64(1))]
    plain_pred = binop(col(0), Operator.Lt, lit_i64(100))
    # in the predicate only
    got = ctx.selection_projection(t, lower_is_bob().flatten(FC), [e.flatten(FC) for e in plain_list]).to_host()
    assert (got[0].to_numpy() == ids[bob]).all() and (got[1].to_numpy() == ids[bob] + 1).all()
    # in the projected expressions only, and in both
    for pred, keep in ((plain_pred, small), (lower_is_bob(), bob)):
        got = ctx.selection_projection(t, pred.flatten(FC), [e.flatten(FC) for e in string_list]).to_host()
        kept = [s for s, k in zip(items, keep) if k]
        assert byte_strings(got[0]) == [model(TRIM, s) for s in kept]
        assert (got[1].to_numpy() == np.array([2 * model(LENGTH, s) for s in kept], dtype=np.int64)).all()
        assert (got[2].to_numpy() == ids[keep]).all()
        assert byte_strings(got[3]) == [model(LOWER, model(TRIM, s)) for s in kept]


def test_projection_of_string_expressions(ctx):
    from naive_query_engine_amd import DType, Operator, ScalarValue
    from naive_query_engine_amd.expression import PhysicalLiteralExpr, binop, lit_i64, lit_utf8

    t, ids, items, v, mask = consumer_table(ctx, nullable=True)
    exprs = [strfn(TRIM, col(1)),                                                        # a bare STRING root as an output column
             binop(strfn(LENGTH, col(1)), Operator.Multiply, lit_i64(2)),               # character_length(s) * 2
             strfn(LOWER, strfn(TRIM, col(1))),                                          # lower(trim(s))
             strfn(REVERSE, lit_utf8("abc")),                                            # over a literal: num_rows copies
             strfn(REVERSE, PhysicalLiteralExpr.create(ScalarValue.Utf8(None))),          # over a NULL literal: all NULL
             strfn(LENGTH, lit_utf8("né日")),
             binop(binop(strfn(LENGTH, col(1)), Operator.Plus, lit_i64(1)), Operator.Gt, lit_i64(3)),  # a step under word operators
             strfn(UPPER, strfn(REVERSE, strfn(RTRIM, strfn(LTRIM, col(1)))))]
    out = ctx.projection(t, [e.flatten(FC) for e in exprs])
    got = out.to_host()
    assert_result(got[0], items, TRIM, mask, "trim(s)")
    assert (got[1].valid_mask() == mask).all() and (got[1].to_numpy()[mask] == np.array([2 * model(LENGTH, s) for s in items], dtype=np.int64)[mask]).all()
    assert byte_strings(got[2]) == [model(LOWER, model(TRIM, s)) for s in items] and (got[2].valid_mask() == mask).all()
    assert byte_strings(got[3]) == [b"cba"] * N_CONS and got[3].valid_mask().all()
    assert got[4].dtype == DType.UTF8 and got[4].length == N_CONS and not got[4].valid_mask().any() and out.column_info(4).null_count == N_CONS
    assert (got[5].to_numpy() == 3).all() and got[5].dtype == DType.INT64
    assert (got[6].valid_mask() == mask).all() and (got[6].to_numpy()[mask] == np.array([model(LENGTH, s) + 1 > 3 for s in items])[mask]).all()
    assert byte_strings(got[7]) == [model(UPPER, model(REVERSE, model(TRIM, s))) for s in items]
    # the same through nqe_expr_evaluate, one at a time
    for k in (0, 2, 3):
        c = ctx.expr_evaluate(t, exprs[k].flatten(FC)).to_host()[0]
        assert byte_strings(c) == byte_strings(got[k]) and (c.valid_mask() == got[k].valid_mask()).all()


def test_aggregate_under_a_string_predicate_and_by_a_character_length_key(ctx):
    from naive_query_engine_amd import AggregateFunc, ErrorCode, Operator, Status
    from naive_query_engine_amd.expression import binop, lit_i64

    t, ids, items, v, _ = consumer_table(ctx)
    bob = np.array([model(LOWER, s) == b"bob" for s in items])
    aggs = [(AggregateFunc.Count, 2), (AggregateFunc.Sum, 2), (AggregateFunc.Min, 2), (AggregateFunc.Max, 2)]
    pred = lower_is_bob().flatten(FC)
    # ungrouped, under the predicate (v holds small integers: the Float64 sum is exact in any order)
    got = [c.to_numpy()[0] for c in ctx.aggregate(t, aggs, pred_nodes=pred).to_host()]
    assert got == [bob.sum(), v[bob].sum(), v[bob].min(), v[bob].max()]
    # grouped by id % 4, under the predicate
    key = binop(col(0), Operator.Modulos, lit_i64(4)).flatten(FC)
    out, keys = ctx.aggregate(t, aggs, group_nodes=key, pred_nodes=pred, with_keys=True)
    rows = {int(k): tuple(float(c.to_numpy()[i]) for c in out.to_host()) for i, k in enumerate(keys.to_host()[0].to_numpy())}
    exp = {}
    for g in range(4):
        sel = bob & (ids % 4 == g)
        if sel.any():
            exp[g] = (float(sel.sum()), float(v[sel].sum()), float(v[sel].min()), float(v[sel].max()))
    assert rows == exp
    # group by character_length(s): an Int64 key expression, through both entries, with and without the predicate
    lens = np.array([model(LENGTH, s) for s in items])
    klen = strfn(LENGTH, col(1)).flatten(FC)
    for p, sel in ((None, np.ones(N_CONS, dtype=bool)), (pred, bob)):
        exp = Counter(lens[sel].tolist())
        out, keys = ctx.aggregate(t, [(AggregateFunc.Count, 0)], group_nodes=klen, pred_nodes=p, with_keys=True)
        assert dict(zip(keys.to_host()[0].to_numpy().tolist(), out.to_host()[0].to_numpy().tolist())) == dict(exp)
        got = ctx.group_aggregate(t, [klen], [(AggregateFunc.Count, 0)], pred_nodes=p).to_host()
        assert got[0].to_numpy().tolist() == sorted(exp) and got[1].to_numpy().tolist() == [exp[k] for k in sorted(exp)]
    # two keys, one of them the length
    got = ctx.group_aggregate(t, [klen, key], [(AggregateFunc.Count, 0)]).to_host()
    exp = Counter(zip(lens.tolist(), (ids % 4).tolist()))
    assert list(zip(got[0].to_numpy().tolist(), got[1].to_numpy().tolist())) == sorted(exp) and got[2].to_numpy().tolist() == [exp[k] for k in sorted(exp)]
    # a Utf8-valued key that is not a bare column stays NotSupported
    ktrim = strfn(TRIM, col(1)).flatten(FC)
    with pytest.raises(ErrorCode) as e:
        ctx.group_aggregate(t, [ktrim], [(AggregateFunc.Count, 0)])
    assert e.value.status == Status.NotSupported
    with pytest.raises(ErrorCode) as e:
        ctx.aggregate(t, [(AggregateFunc.Count, 0)], group_nodes=ktrim)
    assert e.value.status == Status.NotSupported


def test_sort_plan_ordered_by_trim_through_the_python_mirror(ctx):
    from naive_query_engine_amd import DType, Field, RecordBatch
    from naive_query_engine_amd import physical_plan as pp

    t, ids, items, v, _ = consumer_table(ctx)
    flds = [Field("id", DType.INT64, False), Field("s", DType.UTF8, False), Field("v", DType.FLOAT64, False)]
    cols = t.to_host()
    scan = pp.ScanPlan.create(pp.MemTable.try_create(flds, [RecordBatch(flds, cols)], ctx), None)
    out = pp.PhysicalSortPlan.create(scan, [pp.PhysicalSortExpr(strfn(TRIM, col("s")))]).execute()
    assert len(out) == 1 and out[0].num_columns == 3  # the temporary key column is dropped again
    got = out[0].table.to_host()
    order = sorted(range(N_CONS), key=lambda i: model(TRIM, items[i]))  # stable: ties in row order; Utf8 keys compare as bytes
    assert got[0].to_numpy().tolist() == [int(ids[i]) for i in order]
    assert byte_strings(got[1]) == [items[i] for i in order]


# ----------------------------------------------------------------------------- errors, decided before any launch
def test_error_cases(ctx):
    from naive_query_engine_amd import Column, DType, ErrorCode, ScalarValue, Status, UnaryOperator
    from naive_query_engine_amd.arrow_host import node_column, node_string
    from naive_query_engine_amd.expression import PhysicalLiteralExpr, unop

    n = 100
    t = ctx.table_from_host([Column.from_numpy(np.arange(n, dtype=np.int64)), Column.from_numpy(np.arange(n, dtype=np.uint64)),
                             Column.from_numpy(np.arange(n) % 2 == 0), Column.from_numpy(np.ones(n)), Column.from_list(["a"] * n, DType.UTF8)])
    f = fields("i", "u", "b", "v", "s")

    def status_of(nodes):
        ctx.timing_enable(True)
        ctx.timing_reset()
        try:
            with pytest.raises(ErrorCode) as e:
                ctx.expr_evaluate(t, nodes)
            assert ctx.timing_report() == {}, "a kernel was launched before the error was raised"
            return e.value.status
        finally:
            ctx.timing_enable(False)

    for func in UnaryOperator:
        assert status_of([node_string(func)]) == Status.InvalidArgument                            # nothing on the stack
    bad = node_string(UnaryOperator.Trim)
    for op in (14, -1, 1000):
        bad.op = op
        for c in (4, 0):
            assert status_of([node_column(c), bad]) == Status.InvalidArgument                      # outside nqe_unary_operator
    for func in (UnaryOperator.Abs, UnaryOperator.Sin, UnaryOperator.Cos, UnaryOperator.Tan):       # not a string function
        for c in (4, 3, 0):
            assert status_of(strfn(func, col(c)).flatten(f)) == Status.InvalidArgument, (func, c)
    for func in (UnaryOperator.Repeat, UnaryOperator.Replace, UnaryOperator.Substr):                # need arguments the node cannot carry
        for c in (4, 0):
            assert status_of(strfn(func, col(c)).flatten(f)) == Status.NotSupported, (func, c)
    for func in STRING_FUNCTIONS:                                                                   # an operand that is not Utf8
        for c in range(4):
            assert status_of(strfn(func, col(c)).flatten(f)) == Status.NotSupported, (func, c)
        assert status_of(strfn(func, PhysicalLiteralExpr.create(ScalarValue.Int64(3))).flatten(f)) == Status.NotSupported
        assert status_of(strfn(func, PhysicalLiteralExpr.create(ScalarValue.Null())).flatten(f)) == Status.NotSupported
        assert status_of(unop(func, col(4)).flatten(f)) == Status.NotSupported                      # the UNARY node stays the reference's todo!()
    assert status_of(strfn(TRIM, strfn(LENGTH, col(4))).flatten(f)) == Status.NotSupported          # trim(an Int64)
    kind7 = node_string(UnaryOperator.Trim)
    kind7.kind = 7
    assert status_of([node_column(4), kind7]) == Status.InvalidArgument
    # the same errors through the other entries, before any launch
    for run in (lambda nodes: ctx.selection(t, nodes), lambda nodes: ctx.projection(t, [nodes]),
                lambda nodes: ctx.selection_projection(t, col(2).flatten(f), [nodes])):
        with pytest.raises(ErrorCode) as e:
            run(strfn(UnaryOperator.Substr, col(4)).flatten(f))
        assert e.value.status == Status.NotSupported
    # and a well-formed call still works on this context
    assert byte_strings(ctx.expr_evaluate(t, strfn(UPPER, col(4)).flatten(f)).to_host()[0]) == [b"A"] * n
