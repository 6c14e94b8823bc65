"""GPU: an NQE_EXPR_CAST node (quirk Q29) through nqe_expr_evaluate, the operators that take expression trees and the Python plan mirror
— every from -> to pair against the model of tests/cast_util.py (itself checked against pyarrow in tests/test_cast_model.py).  Every
comparison is bit for bit: the values where valid, the ZERO under a NULL (word 0, bit 0, empty string), the packed value and validity
bytes including the zero tail of the last byte, whether a validity buffer is present at all, and null_count.

Row counts.  cast_kernels.hpp: a 256-thread workgroup of cast_fixed covers CAST_BLOCK_ROWS = 256 x CAST_ROWS = 1024 rows per trip, one of
the lane-per-row kernels (cast_parse, cast_text_lengths, cast_text_write) CAST_LANE_ROWS = 256.  stream_grid caps a grid at 8
workgroups per CU (2048 on the 256 CUs of an MI355X; the test reads the device's count): a wave of cast_fixed takes a second chunk
from cap x 1024 + 1 rows on, a lane of the others a second row from cap x 256 + 1.  The parse kernel gives one lane to a row — there is no lanes-per-row split whose groups a
row's bytes could straddle — so the long rows (40, 400 bytes) sit between short ones in every column."""
import numpy as np
import pytest

from tests import cast_util as cu
from tests.cast_util import PAIRS, Val
from tests.helpers import fields
from tests.string_fn_util import byte_strings, utf8_column

pytestmark = pytest.mark.gpu

CAST_BLOCK_ROWS, CAST_LANE_ROWS, BLOCKS_PER_CU = 1024, 256, 8
ROW_COUNTS = (0, 1, 63, 64, 65, CAST_LANE_ROWS - 1, CAST_LANE_ROWS, CAST_LANE_ROWS + 1, CAST_BLOCK_ROWS - 1, CAST_BLOCK_ROWS, CAST_BLOCK_ROWS + 1)
FORMS = ("col", "nullable", "lit", "litnull", "sub", "nullable sub")


@pytest.fixture(scope="module")
def ctx():
    from naive_query_engine_amd import capi

    c = capi.Context(0)
    yield c
    c.close()


def E():
    from naive_query_engine_amd import expression

    return expression


def dtype_of(kind):
    from naive_query_engine_amd import DType

    return {"i64": DType.INT64, "u64": DType.UINT64, "f64": DType.FLOAT64, "bool": DType.BOOLEAN, "utf8": DType.UTF8}[kind]


def to_column(val):
    from naive_query_engine_amd import Column

    mask = val.valid if val.nullable else None
    return utf8_column(val.values, mask) if val.kind == "utf8" else Column.from_numpy(np.asarray(val.values), mask)


def lit_expr(kind, value):
    e = E()
    if value is None:
        return e.lit_null(dtype_of(kind))
    return {"i64": e.lit_i64, "u64": e.lit_u64, "f64": e.lit_f64, "bool": e.lit_bool, "utf8": e.lit_utf8}[kind](value)


def passthrough(kind, x):
    """an operator node that leaves the operand's values and validity as they are: the operand as a SUBTREE"""
    from naive_query_engine_amd import Operator

    e = E()
    if kind == "utf8":
        return e.repeat(x, 1)
    if kind == "bool":
        return e.binop(x, Operator.And, e.lit_bool(True))
    return e.binop(x, Operator.Multiply, lit_expr(kind, 1.0 if kind == "f64" else 1))


def assert_val(out, expected, null_count, what=""):
    """`out`: the 1-column result table; `expected`: the model's Val"""
    from naive_query_engine_amd.arrow_host import pack_bits

    got, info, n = out.to_host()[0], out.column_info(0), len(expected)
    assert got.dtype == dtype_of(expected.kind) and got.length == n, (what, got.dtype, got.length)
    assert (got.valid_mask() == expected.valid).all(), (what, "validity", np.flatnonzero(got.valid_mask() != expected.valid)[:8].tolist())
    if got.validity is not None and n:
        assert (np.asarray(got.validity, dtype=np.uint8)[: (n + 7) // 8] == pack_bits(expected.valid)).all(), (what, "validity tail bits")
    if n:  # (a column of no rows may carry a validity buffer of no bytes or none)
        assert bool(info.validity) == expected.nullable, (what, "validity buffer present", expected.nullable)
        assert info.null_count == null_count, (what, "null_count", info.null_count, null_count)
    if expected.kind == "utf8":
        rows = byte_strings(got)
        assert rows == list(expected.values), (what, [(i, rows[i], expected.values[i]) for i in range(n) if rows[i] != expected.values[i]][:8])
        assert (got.data.size if got.data is not None else 0) == sum(len(s) for s in expected.values), (what, "data length")
    elif expected.kind == "bool":
        bits = np.asarray(got.values, dtype=np.uint8)[: (n + 7) // 8]
        assert (bits == pack_bits(np.asarray(expected.values, dtype=bool))[: (n + 7) // 8]).all(), (what, "value bits", np.flatnonzero(got.to_numpy() != expected.values)[:8].tolist())
    else:
        g, x = np.ascontiguousarray(got.to_numpy()).view(np.uint64), np.ascontiguousarray(expected.values).view(np.uint64)
        assert (g == x).all(), (what, np.flatnonzero(g != x)[:8].tolist(), got.to_numpy()[g != x][:8].tolist(), expected.values[g != x][:8].tolist())


NO_VALUE = object()


def run_case(ctx, frm, to, operand, form="col", expected=None, lit=NO_VALUE):
    """cast(<operand in `form`> as `to`) over one table; operand: a Val — for a literal form its row count alone counts, `lit` is the value"""
    from naive_query_engine_amd import Column

    e, n = E(), len(operand)
    if form in ("lit", "litnull"):
        value = None if form == "litnull" else lit
        assert form == "litnull" or lit is not NO_VALUE
        x, cols = lit_expr(frm, value), [Column.from_numpy(np.zeros(n, dtype=np.int64))]
        operand = Val(frm, [cu.zero_of(frm) if value is None else value] * n, np.full(n, value is not None), nullable=value is None)
    else:
        x, cols = e.col(0), [to_column(operand)]
        if form.endswith("sub"):
            x = passthrough(frm, x)
    expected = cu.cast(operand, to) if expected is None else expected
    if form in ("col", "nullable"):
        cu.guard(frm, to, expected)
    out = ctx.expr_evaluate(ctx.table_from_host(cols), e.cast(x, dtype_of(to)).flatten(fields("c0")))
    assert_val(out, expected, cu.null_count_of(form, operand, frm, to), f"{frm} -> {to} {form} rows {n}")
    return out


# ----------------------------------------------------------------------------- every pair, row count and operand form
@pytest.mark.parametrize("frm,to", PAIRS)
def test_every_pair_at_every_row_count(ctx, frm, to):
    """0, 1, the edges of a bitmap word and a wave, and one below / at / one above the rows a workgroup of each kernel covers, over a plain
    and a nullable column"""
    for n in ROW_COUNTS:
        run_case(ctx, frm, to, cu.pair_column(frm, to, n), "col")
        run_case(ctx, frm, to, cu.pair_column(frm, to, n, nullable=True), "nullable")


@pytest.mark.parametrize("frm,to", PAIRS)
def test_every_pair_over_every_operand_form(ctx, frm, to):
    """a literal and a NULL literal (expanded, then cast like a column: no folding path), a literal the cast refuses, a subtree with and
    without validity; a plain column through an input that begins at an odd offset"""
    n = 257
    rows = cu.pair_rows(frm, to)
    for form in ("sub", "nullable sub"):
        run_case(ctx, frm, to, cu.pair_column(frm, to, n, nullable=form.startswith("nullable")), form)
    for value in [rows[0][0], rows[1][0]] + [v for v, x, _ in rows if x is None][:2]:
        run_case(ctx, frm, to, Val(frm, [value] * n), "lit", lit=value)
    run_case(ctx, frm, to, Val(frm, [cu.zero_of(frm)] * n), "litnull")
    for m in (0, 1):
        run_case(ctx, frm, to, Val(frm, [rows[0][0]] * m), "lit", lit=rows[0][0])
        run_case(ctx, frm, to, Val(frm, [cu.zero_of(frm)] * m), "litnull")
    # the operand is a slice that begins 3 and 13 rows into the uploaded buffers (24 bytes: no 16-byte alignment; bit 3, bit 5 of a byte)
    e = E()
    for lead in (3, 13):
        full = cu.pair_column(frm, to, n + lead, nullable=True, seed=lead)
        t = ctx.slice(ctx.table_from_host([to_column(full)]), lead, n)
        part = Val(frm, full.values[lead:], full.valid[lead:], nullable=True)
        out = ctx.expr_evaluate(t, e.cast(e.col(0), dtype_of(to)).flatten(fields("c0")))
        assert_val(out, cu.cast(part, to), -1, f"{frm} -> {to} lead {lead}")


@pytest.mark.parametrize("kind", cu.KINDS)
def test_the_same_dtype_cast_is_the_operand(ctx, kind):
    src = [p for p in PAIRS if p[0] == kind][0]
    for n in (0, 1, 65, 257):
        for nullable in (False, True):
            col = cu.pair_column(kind, src[1], n, nullable)
            out = ctx.expr_evaluate(ctx.table_from_host([to_column(col)]), E().cast(E().col(0), dtype_of(kind)).flatten(fields("c0")))
            got = out.to_host()[0]
            assert got.dtype == dtype_of(kind) and got.length == n and (got.valid_mask() == col.valid).all()
            if n:
                assert bool(out.column_info(0).validity) == nullable
            if kind == "utf8":
                assert byte_strings(got) == col.values  # as a bare column evaluates: the bytes under a NULL stay
            elif kind == "bool":
                assert (got.to_numpy()[col.valid] == col.values[col.valid]).all()
            else:
                assert (np.ascontiguousarray(got.to_numpy()).view(np.uint64) == np.ascontiguousarray(col.values).view(np.uint64)).all()
        value = cu.pair_rows(*src)[0][0]
        t = ctx.table_from_host([to_column(Val("i64", np.zeros(n, dtype=np.int64)))])  # a literal is expanded to the table's rows, as a bare literal is
        got = ctx.expr_evaluate(t, E().cast(lit_expr(kind, value), dtype_of(kind)).flatten(fields("c0"))).to_host()[0]
        assert got.dtype == dtype_of(kind) and got.length == n and got.validity is None
        assert (byte_strings(got) if kind == "utf8" else got.to_numpy().tolist()) == [value] * n


def tiled(frm, to, n, nullable):
    """n rows by repeating a block of 4096 (the model runs over the block alone)"""
    block = cu.pair_column(frm, to, 4096, nullable)
    want = cu.cast(block, to)
    reps = n // 4096 + 1
    tile = (lambda v, kind: (list(v) * reps)[:n] if kind == "utf8" else np.tile(v, reps)[:n])
    operand = Val(frm, tile(block.values, frm), np.tile(block.valid, reps)[:n], nullable=block.nullable)
    return operand, Val(to, tile(want.values, to), np.tile(want.valid, reps)[:n], nullable=want.nullable)


def grid_cap():
    """the workgroups stream_grid gives a kernel at most: 8 per compute unit of device 0, the context's (nqe_ctx_create reads the same
    count from hipGetDeviceProperties).  Asked of the HIP runtime the library has loaded into this process."""
    import ctypes

    hip = ctypes.CDLL("libamdhip64.so")
    cus = ctypes.c_int(0)
    HIP_DEVICE_ATTRIBUTE_MULTIPROCESSOR_COUNT = 63  # hipDeviceAttributeMultiprocessorCount (hip_runtime_api.h)
    assert hip.hipDeviceGetAttribute(ctypes.byref(cus), HIP_DEVICE_ATTRIBUTE_MULTIPROCESSOR_COUNT, 0) == 0
    assert 16 <= cus.value <= 1024, cus.value
    return BLOCKS_PER_CU * cus.value


@pytest.mark.parametrize("frm,to,block_rows", [("i64", "f64", CAST_BLOCK_ROWS), ("f64", "i64", CAST_BLOCK_ROWS), ("f64", "bool", CAST_BLOCK_ROWS), ("bool", "u64", CAST_BLOCK_ROWS),
                                               ("utf8", "i64", CAST_LANE_ROWS), ("utf8", "bool", CAST_LANE_ROWS), ("i64", "utf8", CAST_LANE_ROWS), ("bool", "utf8", CAST_LANE_ROWS)])
def test_the_second_trip_of_every_kernels_grid_stride_loop(ctx, frm, to, block_rows):
    """the smallest row count at which some wave of cast_fixed takes a second chunk / some lane of cast_parse, cast_text_lengths and
    cast_text_write a second row (the last row is that trip's only one): the grid's cap x the rows a workgroup covers, + 1"""
    n = grid_cap() * block_rows + 1
    operand, expected = tiled(frm, to, n, nullable=True)
    run_case(ctx, frm, to, operand, "nullable", expected=expected)


def test_utf8_lengths(ctx):
    """0, 1, 19 / 20 digits, 40 and 400 bytes — valid and refused — between short rows, for every parser; the texts of every digit count"""
    digits19, digits20 = b"1234567890123456789", b"12345678901234567890"
    rows = [b"", b"7", digits19, digits20, b"-" + digits19, b"+" + digits19, b"18446744073709551615", b"0" * 21 + b"42", b"0" * 398 + b"42", b"4" * 40, b"4" * 400, b"0." + b"3" * 398, b"1e5", b"true", b"false", b"False", b"TRUE" + b" " * 396]
    col = Val("utf8", [rows[i % len(rows)] for i in range(300)], cu.mask_of(300, "lengths"))
    for to in ("i64", "u64", "f64", "bool"):
        run_case(ctx, "utf8", to, col, "nullable")
    ints = [0] + [10 ** k for k in range(19)] + [10 ** k - 1 for k in range(1, 19)] + [-(10 ** k) for k in range(19)] + [cu.I64_MIN, cu.I64_MAX]
    run_case(ctx, "i64", "utf8", Val("i64", ints))
    out = run_case(ctx, "u64", "utf8", Val("u64", [0, cu.U64_MAX] + [10 ** k for k in range(20)] + [10 ** k - 1 for k in range(1, 20)]))
    assert sorted({len(s) for s in byte_strings(out.to_host()[0])}) == list(range(1, 21))  # every digit count from 1 to 20
    assert byte_strings(run_case(ctx, "i64", "utf8", Val("i64", [cu.I64_MIN] * 3)).to_host()[0]) == [b"-9223372036854775808"] * 3  # 20 bytes


# ----------------------------------------------------------------------------- through the operators
def test_id_times_one_and_a_half_written_with_a_cast_equals_numpy(ctx):
    from naive_query_engine_amd import Column, DType, Operator

    e, n = E(), 100_003
    ids = cu.rng_for("ids").integers(-(1 << 62), 1 << 62, n).astype(np.int64)
    ids[:4] = [0, -1, (1 << 53) + 1, cu.I64_MAX]
    t = ctx.table_from_host([Column.from_numpy(ids)])
    out = ctx.expr_evaluate(t, e.binop(e.cast(e.col(0), DType.FLOAT64), Operator.Multiply, e.lit_f64(1.5)).flatten(fields("id"))).to_host()[0]
    assert out.validity is None and (out.to_numpy().view(np.uint64) == (ids.astype(np.float64) * 1.5).view(np.uint64)).all()
    # without the cast it cannot be written (Q6: no coercion)
    from naive_query_engine_amd import ErrorCode, Status

    with pytest.raises(ErrorCode) as err:
        ctx.expr_evaluate(t, e.binop(e.col(0), Operator.Multiply, e.lit_f64(1.5)).flatten(fields("id")))
    assert err.value.status == Status.IntervalError
    # v > 0 with an Int64 literal; coalesce(v, 0) over a Float64 v
    v, vmask = (ids % 7 - 3).astype(np.float64), cu.mask_of(n, "v")
    t = ctx.table_from_host([Column.from_numpy(v, vmask)])
    got = ctx.expr_evaluate(t, e.binop(e.col(0), Operator.Gt, e.cast(e.lit_i64(0), DType.FLOAT64)).flatten(fields("v"))).to_host()[0]
    assert (got.valid_mask() == vmask).all() and (got.to_numpy()[vmask] == (v > 0)[vmask]).all()
    got = ctx.expr_evaluate(t, e.coalesce(e.col(0), e.cast(e.lit_i64(0), DType.FLOAT64)).flatten(fields("v"))).to_host()[0]
    assert got.validity is None and (got.to_numpy() == np.where(vmask, v, 0.0)).all()


def test_as_filter_projection_group_key_sort_key_and_aggregate_predicate(ctx):
    from naive_query_engine_amd import AggregateFunc, Column, DType, Field, Operator, RecordBatch
    from naive_query_engine_amd import physical_plan as pp

    e, n = E(), 5000
    r = cu.rng_for("operators")
    ids = np.arange(n, dtype=np.int64)
    num = r.integers(-50, 51, n)
    texts = [(b"%d" % x if i % 11 else b"n/a") for i, x in enumerate(num)]  # a numeric column the CSV reader inferred as Utf8
    smask = cu.mask_of(n, "s")
    good = smask & (np.arange(n) % 11 != 0)
    v = (r.integers(-100, 101, n) / 4.0).astype(np.float64)
    cols = [Column.from_numpy(ids), utf8_column(texts, smask), Column.from_numpy(v)]
    f = fields("id", "s", "v")
    t = ctx.table_from_host(cols)
    ID, S, V = (e.col(i) for i in range(3))
    as_int = e.cast(S, DType.INT64)
    # filter: where cast(s as bigint) > 0 — a NULL predicate row is emitted as a NULL row (quirk Q4)
    out = ctx.selection(t, e.binop(as_int, Operator.Gt, e.lit_i64(0)).flatten(f)).to_host()
    keep = ~good | (num > 0)
    assert out[0].length == int(keep.sum()) and (out[0].valid_mask() == good[keep]).all() and (out[0].to_numpy()[good[keep]] == ids[good & (num > 0)]).all()
    # where cast(v as boolean): a Boolean cast as the whole predicate
    out = ctx.selection(t, e.cast(V, DType.BOOLEAN).flatten(f)).to_host()
    assert (out[0].to_numpy() == ids[v != 0]).all() and 0 < out[0].length < n
    # projection, alone and behind a selection: the text summed
    proj = ctx.projection(t, [as_int.flatten(f), e.cast(ID, DType.UTF8).flatten(f)])
    got = proj.to_host()
    assert (got[0].valid_mask() == good).all() and (got[0].to_numpy()[good] == num[good]).all() and byte_strings(got[1]) == [b"%d" % i for i in ids]
    total = ctx.aggregate(proj, [(AggregateFunc.Sum, 0)]).to_host()
    assert total[0].to_numpy().tolist() == [float(num[good].sum())] and good.sum() > n // 2
    out = ctx.selection_projection(t, e.cast(V, DType.BOOLEAN).flatten(f), [e.cast(V, DType.INT64).flatten(f), ID.flatten(f)]).to_host()
    assert (out[1].to_numpy() == ids[v != 0]).all() and (out[0].to_numpy() == np.trunc(v).astype(np.int64)[v != 0]).all() and out[0].valid_mask().all()
    # group key and aggregate predicate: group by cast(v as bigint) where cast(s as bigint) is not NULL
    key = e.cast(V, DType.INT64)
    kk = np.trunc(v).astype(np.int64)
    out, keys = ctx.aggregate(t, [(AggregateFunc.Count, 0), (AggregateFunc.Sum, 0)], group_nodes=key.flatten(f), pred_nodes=e.is_not_null(as_int).flatten(f), with_keys=True)
    got = {int(g): (int(c), float(s)) for g, c, s in zip(keys.to_host()[0].to_numpy(), out.to_host()[0].to_numpy(), out.to_host()[1].to_numpy())}
    want = {int(g): (int((good & (kk == g)).sum()), float(ids[good & (kk == g)].sum())) for g in np.unique(kk[good])}
    assert got == want and len(want) > 10
    out = ctx.group_aggregate(t, [key.flatten(f)], [(AggregateFunc.Count, 0)], pred_nodes=e.not_(e.is_null(as_int)).flatten(f)).to_host()
    assert out[0].to_numpy().tolist() == sorted(want) and out[1].to_numpy().astype(np.int64).tolist() == [want[g][0] for g in sorted(want)]
    # sort key through the mirror: order by cast(s as bigint) — numerically, not as text; the sort is stable
    schema = [Field("id", DType.INT64, True), Field("s", DType.UTF8, True), Field("v", DType.FLOAT64, True)]
    all_good = [b"%d" % x for x in num]
    scan = pp.ScanPlan.create(pp.MemTable.try_create(schema, [RecordBatch(schema, [cols[0], utf8_column(all_good), cols[2]])], ctx))
    out = pp.PhysicalSortPlan.create(scan, [pp.PhysicalSortExpr.create(e.cast(e.col("s"), DType.INT64))]).execute()[0].table.to_host()
    assert out[0].to_numpy().tolist() == sorted(range(n), key=lambda i: int(num[i])) and len(out) == 3
    assert out[0].to_numpy().tolist() != sorted(range(n), key=lambda i: all_good[i])


# ----------------------------------------------------------------------------- the errors, at the C ABI, in their order
def test_the_four_errors_at_the_c_abi_in_their_order(ctx):
    from naive_query_engine_amd import Column, DType, ErrorCode, PhysicalLiteralExpr, ScalarValue, Status
    from naive_query_engine_amd.arrow_host import node_cast, node_column

    e, n = E(), 100
    cols = [Column.from_numpy(np.arange(n, dtype=np.int64)), Column.from_numpy(np.arange(n) % 2 == 0), Column.from_numpy(np.arange(n, dtype=np.float64)), utf8_column([b"12"] * n)]
    f = fields("i", "b", "v", "s")
    t = ctx.table_from_host(cols)
    I, B, V, S = (e.col(k) for k in range(4))
    entries = [("expr_evaluate", lambda nodes: ctx.expr_evaluate(t, nodes)), ("selection", lambda nodes: ctx.selection(t, nodes)),
               ("projection", lambda nodes: ctx.projection(t, [nodes])), ("selection_projection", lambda nodes: ctx.selection_projection(t, B.flatten(f), [nodes])),
               ("selection_projection predicate", lambda nodes: ctx.selection_projection(t, nodes, [I.flatten(f)]))]

    def status_of(nodes):
        seen = set()
        for name, run in entries:
            ctx.timing_enable(True)
            ctx.timing_reset()
            try:
                with pytest.raises(ErrorCode) as err:
                    run(nodes)
                assert ctx.timing_report() == {}, (name, "a kernel was launched before the error was raised")
                seen.add(err.value.status)
            finally:
                ctx.timing_enable(False)
        assert len(seen) == 1, seen
        return seen.pop()

    def raw(target, operands):
        nodes = []
        for x in operands:
            nodes += x.flatten(f)
        return nodes + [node_cast(target)]

    null_typed = PhysicalLiteralExpr.create(ScalarValue.Null())
    # 1. `dtype` outside Boolean .. Utf8 — before the empty stack, the Null-typed operand and Float64 -> Utf8
    for target in (0, -1, 6, 100):
        assert status_of(raw(target, [])) == Status.InvalidArgument
        assert status_of(raw(target, [null_typed])) == Status.InvalidArgument
        assert status_of(raw(target, [V])) == Status.InvalidArgument
    # 2. no operand
    for target in range(1, 6):
        assert status_of(raw(target, [])) == Status.InvalidArgument
    # 3. a Null-typed operand, to every target (Utf8 too: not 4.)
    for target in range(1, 6):
        assert status_of(raw(target, [null_typed])) == Status.NotSupported
    # 4. Float64 -> Utf8, of every operand form
    for x in (V, e.lit_f64(1.5), e.lit_null(DType.FLOAT64), e.cast(I, DType.FLOAT64)):
        assert status_of(raw(int(DType.UTF8), [x])) == Status.NotSupported
    # kind 9 is unknown; kind 8 with dtype 0 is rule 1
    nine = node_cast(DType.INT64)
    nine.kind = 9
    assert status_of([node_column(0), nine]) == Status.InvalidArgument
    assert status_of([node_column(0), node_cast(0)]) == Status.InvalidArgument
    # and well-formed calls still work on this context
    assert ctx.expr_evaluate(t, e.cast(S, DType.INT64).flatten(f)).to_host()[0].to_numpy().tolist() == [12] * n
    assert ctx.selection(t, e.cast(B, DType.BOOLEAN).flatten(f)).to_host()[0].length == n // 2


def test_a_result_of_more_than_2_31_bytes_is_an_arrow_error_before_the_data_exists(ctx):
    """2^31 / 20 + 1 rows of INT64_MIN, 20 bytes each: more than 2^31-1 bytes.  The literal is expanded over a Boolean table (13 MB to upload);
    the lengths kernel and the read-back of the total run, and nothing of the data is allocated"""
    from naive_query_engine_amd import Column, DType, ErrorCode, Status

    n = (1 << 31) // 20 + 1
    t = ctx.table_from_host([Column.from_numpy(np.zeros(n, dtype=bool))])
    with pytest.raises(ErrorCode) as err:
        ctx.expr_evaluate(t, E().cast(E().lit_i64(cu.I64_MIN), DType.UTF8).flatten(fields("b")))
    assert err.value.status == Status.ArrowError and "offset overflow" in str(err.value)
    del t
    small = ctx.table_from_host([Column.from_numpy(np.arange(5, dtype=np.int64))])
    assert byte_strings(ctx.expr_evaluate(small, E().cast(E().col(0), DType.UTF8).flatten(fields("id"))).to_host()[0]) == [b"0", b"1", b"2", b"3", b"4"]
