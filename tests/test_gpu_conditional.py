"""GPU: an NQE_EXPR_CONDITIONAL node (quirk Q28: not, is_null, is_not_null, coalesce, nullif, if) through nqe_expr_evaluate, every
operator that takes expression trees, and the Python plan mirror — against the numpy model of tests/conditional_util.py (itself checked
against pyarrow in tests/test_conditional_model.py).  Every comparison is bit for bit: the values where valid, the ZERO under a NULL
(word 0, bit 0, empty string), the packed value and validity bytes including the zero tail of the last byte, whether a validity buffer
is present at all, and null_count (-1 with a buffer, 0 without).  The case lists are conditional_util's; tests/test_conditional_cases.py
shows on the CPU that none of them can be passed with a constant answer, and every case asserts its guard again here."""
import numpy as np
import pytest

from tests import conditional_util as cu
from tests.conditional_util import COALESCE, IF, IS_NOT_NULL, IS_NULL, KINDS, NOT, NULLIF, ROW_COUNTS
from tests.helpers import fields
from tests.string_fn_util import byte_strings, utf8_column

pytestmark = pytest.mark.gpu


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
    if val.kind == "utf8":
        return utf8_column(val.values, mask)
    return Column.from_numpy(np.asarray(val.values), mask)


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
    return e.binop(x, Operator.Multiply, lit_expr(kind, 1 if kind != "f64" else 1.0))


class Inputs:
    """the columns of one input table, and the expression of every operand over it"""

    def __init__(self, n, lead=0):
        self.n, self.lead, self.cols = n, lead, []

    def operand(self, arg):
        if arg.form in ("lit", "litnull"):
            return lit_expr(arg.kind, arg.lit)
        val = arg.val
        if self.lead:  # `lead` extra rows in front, cut off again by a slice: the column's buffers then begin at an odd offset
            pad = cu.make(val.kind, cu.values_of(val.kind, self.lead, 99), np.zeros(self.lead, dtype=bool) if val.nullable else None)
            values = (list(pad.values) + list(val.values)) if val.kind == "utf8" else np.concatenate([pad.values, val.values])
            val = cu.Val(val.kind, values, np.concatenate([pad.valid, val.valid]), val.nullable)
        self.cols.append(to_column(val))
        x = E().col(len(self.cols) - 1)
        return passthrough(arg.kind, x) if arg.form == "sub" else x

    def table(self, ctx):
        from naive_query_engine_amd import Column

        if not self.cols:  # an all-literal node: expanded to the table's rows
            self.cols.append(Column.from_numpy(np.zeros(self.n + self.lead, dtype=np.int64)))
        t = ctx.table_from_host(self.cols)
        return ctx.slice(t, self.lead, self.n) if self.lead else t

    def fields(self):
        return fields(*[f"c{i}" for i in range(max(1, len(self.cols)))])


def node(op, operands):
    from naive_query_engine_amd import CondOperator, PhysicalConditionalExpr

    return PhysicalConditionalExpr.create(CondOperator(op), operands)


def assert_val(out, expected, what=""):
    """`out`: the 1-column result table; `expected`: the model's Val"""
    from naive_query_engine_amd.arrow_host import pack_bits

    got, info, n = out.to_host()[0], out.column_info(0), len(expected)
    assert got.dtype == dtype_of(expected.kind) and got.length == n, (what, got.dtype, got.length)
    assert (got.valid_mask() == expected.valid).all(), (what, "validity", np.flatnonzero(got.valid_mask() != expected.valid)[:8].tolist())
    if got.validity is not None and n:
        assert (np.asarray(got.validity, dtype=np.uint8)[: (n + 7) // 8] == pack_bits(expected.valid)).all(), (what, "validity tail bits")
    if n:  # (a column of no rows may carry a validity buffer of no bytes or none)
        assert bool(info.validity) == expected.nullable, (what, "validity buffer present", expected.nullable)
    assert info.null_count == cu.null_count_of(expected), (what, "null_count", info.null_count)
    if expected.kind == "utf8":
        rows = byte_strings(got)
        assert rows == list(expected.values), (what, [i for i in range(n) if rows[i] != expected.values[i]][:8])
        assert (got.data.size if got.data is not None else 0) == sum(len(s) for s in expected.values), (what, "data length")
    elif expected.kind == "bool":
        bits = np.asarray(got.values, dtype=np.uint8)[: (n + 7) // 8]
        assert (bits == pack_bits(np.asarray(expected.values, dtype=bool))[: (n + 7) // 8]).all(), (what, "value bits", np.flatnonzero(got.to_numpy() != expected.values)[:8].tolist())
    else:
        g, x = np.ascontiguousarray(got.to_numpy()).view(np.uint64), np.ascontiguousarray(expected.values).view(np.uint64)
        assert (g == x).all(), (what, np.flatnonzero(g != x)[:8].tolist(), got.to_numpy()[g != x][:8].tolist(), expected.values[g != x][:8].tolist())


def run_case(ctx, case, lead=0, what=""):
    op, args, expected = case
    cu.guard(op, args, expected)
    inputs = Inputs(len(expected), lead)
    expr = node(op, [inputs.operand(a) for a in args])
    t = inputs.table(ctx)
    out = ctx.expr_evaluate(t, expr.flatten(inputs.fields()))
    assert_val(out, expected, f"{what} op {op} forms {[a.form for a in args]} kind {expected.kind if op > IS_NOT_NULL else args[0].kind} rows {len(expected)} lead {lead}")
    return out


# ----------------------------------------------------------------------------- every function, dtype family, row count and operand form
@pytest.mark.parametrize("n", ROW_COUNTS)
@pytest.mark.parametrize("kind", KINDS)
def test_every_row_count(ctx, kind, n):
    """0, 1 and the edges of a bitmap word, a wave, a workgroup and the grid's stride, over the diagonal of the operand forms: cond_words
    for the word types, cond_bits for Boolean and for NOT / IS_NULL / IS_NOT_NULL of every type, the Utf8 kernels"""
    for case in cu.row_count_cases(kind, n):
        run_case(ctx, case)


@pytest.mark.parametrize("op", [COALESCE, NULLIF, IF])
@pytest.mark.parametrize("kind", KINDS)
def test_every_combination_of_operand_forms_at_257_rows(ctx, kind, op):
    """column without validity, with ~30 % NULLs, all NULL, literal, NULL literal, subtree — in every position at once (IF: 6^3); the
    COALESCE whose first operand is a column without validity launches nothing and returns that column"""
    for case in cu.grid_cases(kind, op):
        run_case(ctx, case)


@pytest.mark.parametrize("kind", KINDS)
def test_columns_that_begin_at_an_odd_offset(ctx, kind):
    """the input is a slice that begins 3 rows (word columns: 24 bytes, no 16-byte alignment) and 13 rows into the uploaded buffers"""
    for lead in (3, 13):
        for n in (1, 64, 257, 1025):
            for case in cu.row_count_cases(kind, n)[:12]:
                run_case(ctx, case, lead=lead)


def test_nullif_at_the_edge_values_of_every_word_type(ctx):
    nan, inf, n = float("nan"), float("inf"), 257
    lo, hi = np.iinfo(np.int64).min, np.iinfo(np.int64).max
    sets = {"f64": ([nan, nan, -0.0, 0.0, 0.0, inf, inf, -inf, 1.5, 1.5, 2.0, -0.0], [nan, 1.0, 0.0, -0.0, 0.0, inf, -inf, -inf, 1.5, 2.5, nan, -0.0]),
            "i64": ([lo, lo, hi, hi, 0, -1, lo], [lo, hi, hi, lo, 0, 1, lo + 1]),
            "u64": ([(1 << 63), (1 << 63) + 5, (1 << 64) - 1, (1 << 64) - 1, 0, 1 << 63], [(1 << 63), (1 << 63) - 5, (1 << 64) - 1, (1 << 63) - 1, 0, 0])}
    for kind, (a, b) in sets.items():
        reps = n // len(a) + 1
        av, bv = cu.make(kind, (a * reps)[:n]), cu.make(kind, (b * reps)[:n])
        am = cu.make(kind, (a * reps)[:n], cu.mask_of(n, 5))
        for x, y in ((av, bv), (am, bv), (bv, am)):
            args = [cu.Arg(kind, "nullable" if x.nullable else "plain", x), cu.Arg(kind, "nullable" if y.nullable else "plain", y)]
            run_case(ctx, (NULLIF, args, cu.nullif(x, y)), what="edge values")
            run_case(ctx, (COALESCE, args, cu.coalesce(x, y)) if x.nullable else (IF, [cu.make_arg("bool", "nullable", n, 3)] + args, cu.if_else(cu.make_arg("bool", "nullable", n, 3).val, x, y)),
                     what="edge values")
        for value in a[:4]:  # the literal on either side
            lit = cu.Arg(kind, "lit", cu.literal(kind, value, n), value)
            run_case(ctx, (NULLIF, [cu.Arg(kind, "plain", av), lit], cu.nullif(av, lit.val)), what="edge literal")
            run_case(ctx, (NULLIF, [lit, cu.Arg(kind, "nullable", am)], cu.nullif(lit.val, am)), what="edge literal first")
    # by hand, from NQE_OP_EQ: NaN equals nothing, -0.0 equals +0.0
    r = cu.nullif(cu.make("f64", sets["f64"][0]), cu.make("f64", sets["f64"][1]))
    assert r.valid.tolist() == [True, True, False, False, False, False, True, False, False, True, True, False]


# ----------------------------------------------------------------------------- Utf8
BANDS = {2: (0, 32), 3: (33, 96), 4: (97, 256), 5: (257, 1024), 6: (1025, 1 << 30)}  # lanes_log2 by the RESULT's mean length


def band_case(op, lg, target, n=130):
    """operands whose rows are about `target` bytes long, the word-edge lengths among them"""
    r = cu.rng_for("band", lg, op)
    lens = [0, 1, 7, 8, 9, 31, 32, 33] + [int(x) for x in r.integers(max(0, target - 9), target + 10, n - 8)]
    a_items = [bytes([65 + i % 26]) * L for i, L in enumerate(lens)]
    b_items = [bytes([97 + i % 26]) * lens[(i * 7 + 3) % n] for i in range(n)]
    a, b = cu.make("utf8", a_items, cu.mask_of(n, 11)), cu.make("utf8", b_items, cu.mask_of(n, 12))
    if op == NULLIF:
        vals = [a, cu.make("utf8", [a_items[i] if i % 3 == 0 else b_items[i] for i in range(n)])]
    else:
        vals = ([cu.make_arg("bool", "nullable", n, 13).val] if op == IF else []) + [a, b]
    expected = cu.apply(op, *vals)
    return [cu.Arg(v.kind, "nullable" if v.nullable else "plain", v) for v in vals], expected, sum(len(s) for s in expected.values) // n


@pytest.mark.parametrize("lg", sorted(BANDS))
def test_every_copy_instance_by_the_results_mean_length(ctx, lg):
    """one case per band of lanes_log2 — taken on the RESULT's mean length, NULL and empty rows included: the operands' lengths are
    scaled (on the host, from the model alone) until the expected mean lies in the band, so the copy kernel of that lane group runs"""
    lo, hi = BANDS[lg]
    middle = (lo + min(hi, 3 * lo + 40)) // 2
    for op in (COALESCE, IF, NULLIF):
        target = middle
        for _ in range(6):
            args, expected, mean = band_case(op, lg, target)
            if lo + 2 <= mean <= hi - 2 or (lg == 2 and mean <= hi - 2):
                break
            target = max(1, target * middle // max(mean, 1))
        assert lo <= mean <= hi, (lg, op, mean)
        run_case(ctx, (op, args, expected), what=f"2^{lg} lanes")


def test_utf8_empty_buffers_literals_and_the_classic(ctx):
    n = 300
    names = [b"n%d" % i if i % 4 else b"" for i in range(n)]
    s = cu.make("utf8", names, cu.mask_of(n, 21))
    unknown = cu.Arg("utf8", "lit", cu.literal("utf8", b"unknown", n), b"unknown")
    out = run_case(ctx, (COALESCE, [cu.Arg("utf8", "nullable", s), unknown], cu.coalesce(s, unknown.val)), what="coalesce(s, 'unknown')")
    assert out.column_info(0).null_count == 0 and b"unknown" in byte_strings(out.to_host()[0])
    run_case(ctx, (COALESCE, [unknown, cu.Arg("utf8", "nullable", s)], cu.coalesce(unknown.val, s)), what="literal first")
    run_case(ctx, (NULLIF, [cu.Arg("utf8", "nullable", s), cu.Arg("utf8", "lit", cu.literal("utf8", b"", n), b"")], cu.nullif(s, cu.literal("utf8", b"", n))), what="nullif(s, '')")
    # columns without a byte: every string empty, and every row NULL
    empty, allnull = cu.make("utf8", [b""] * n, cu.mask_of(n, 22)), cu.make("utf8", [b""] * n, np.zeros(n, dtype=bool))
    c = cu.make_arg("bool", "nullable", n, 23)
    form = lambda v: "nullable" if v.valid.any() else "allnull"
    for x, y in ((empty, allnull), (allnull, empty), (allnull, allnull), (empty, s)):
        args = [cu.Arg("utf8", form(x), x), cu.Arg("utf8", form(y), y)]
        for op in (COALESCE, NULLIF):
            run_case(ctx, (op, args, cu.apply(op, x, y)), what="empty data")
        run_case(ctx, (IF, [c] + args, cu.if_else(c.val, x, y)), what="empty data")
    # an all-literal node: n rows
    for op, args in ((COALESCE, [cu.make_arg("utf8", "litnull", n, 0), unknown]), (IF, [cu.make_arg("bool", "litnull", n, 0), unknown, cu.make_arg("utf8", "litnull", n, 0)]),
                     (IS_NULL, [cu.make_arg("utf8", "litnull", n, 0)]), (IS_NOT_NULL, [unknown])):
        run_case(ctx, (op, args, cu.apply(op, *[a.val for a in args])), what="all literals")


def test_utf8_result_past_int32_offsets_is_an_arrow_error_and_the_context_lives(ctx):
    """two operands of ~1.1 GiB each (repeat of a 1-byte string, the counts alternating 2^21 / 0 and 0 / 2^21 over 1100 rows): the IF
    that takes the long row of each holds ~2.2 GiB — NQE_ERR_ARROW before the data buffer is allocated; then the same context works"""
    from naive_query_engine_amd import Column, ErrorCode, Status

    e, n, big = E(), 1100, 1 << 21
    ka = np.where(np.arange(n) % 2 == 0, big, 0).astype(np.int64)
    cols = [utf8_column([b"x"] * n), Column.from_numpy(ka), Column.from_numpy(big - ka), Column.from_numpy(np.arange(n) % 2 == 0)]
    f = fields("s", "ka", "kb", "even")
    t = ctx.table_from_host(cols)
    a, b = e.repeat(e.col(0), e.col(1)), e.repeat(e.col(0), e.col(2))
    with pytest.raises(ErrorCode) as err:
        ctx.expr_evaluate(t, e.if_else(e.col(3), a, b).flatten(f))
    assert err.value.status == Status.ArrowError and "offset overflow" in str(err.value)
    # the other branch of every row is empty: the same operands, a result of no bytes — on the same context
    out = ctx.expr_evaluate(t, e.if_else(e.col(3), b, a).flatten(f))
    got = out.to_host()[0]
    assert got.length == n and (np.asarray(got.values) == 0).all() and out.column_info(0).null_count == 0
    small = ctx.expr_evaluate(t, e.coalesce(e.lit_null(dtype_of("utf8")), e.col(0)).flatten(f))
    assert byte_strings(small.to_host()[0]) == [b"x"] * n


# ----------------------------------------------------------------------------- identities, evaluated on the device itself
@pytest.mark.parametrize("kind", KINDS)
def test_differential_identities(ctx, kind):
    from naive_query_engine_amd import Operator

    e, n = E(), 1025
    a, b, c = cu.make_arg(kind, "nullable", n, 31), cu.make_arg(kind, "nullable", n, 32), cu.make_arg("bool", "nullable", n, 33)
    b = cu.make_arg(kind, "nullable", n, 32, like=a)
    inputs = Inputs(n)
    A, B, C = inputs.operand(a), inputs.operand(b), inputs.operand(c)
    t, f = inputs.table(ctx), inputs.fields()

    def same(x, y, where_valid_only=False):
        gx, gy = ctx.expr_evaluate(t, x.flatten(f)).to_host()[0], ctx.expr_evaluate(t, y.flatten(f)).to_host()[0]
        assert (gx.valid_mask() == gy.valid_mask()).all()
        rx = byte_strings(gx) if kind == "utf8" and gx.dtype == dtype_of("utf8") else gx.to_numpy()
        ry = byte_strings(gy) if kind == "utf8" and gy.dtype == dtype_of("utf8") else gy.to_numpy()
        if where_valid_only:
            m = gx.valid_mask()
            assert (np.asarray(rx)[m] == np.asarray(ry)[m]).all()
        elif isinstance(rx, list):
            assert rx == ry
        else:
            assert (np.ascontiguousarray(rx).view(np.uint8) == np.ascontiguousarray(ry).view(np.uint8)).all()
        return gx

    null = e.lit_null(dtype_of(kind))
    r = same(e.nullif(A, B), e.if_else(e.binop(A, Operator.Eq, B), null, A))  # nullif(a, b) = if(a = b, NULL, a)
    assert 0 < (~r.valid_mask() & a.val.valid).sum() and r.valid_mask().any()
    same(e.coalesce(A, B), e.if_else(e.is_not_null(A), A, B))  # coalesce(a, b) = if(is_not_null(a), a, b)
    r = same(e.is_null(A), e.not_(e.is_not_null(A)))  # is_null(x) = not(is_not_null(x))
    assert r.to_numpy().any() and not r.to_numpy().all()
    same(e.not_(e.not_(C)), C, where_valid_only=True)  # not(not(b)) = b where valid
    same(e.coalesce(A, B, A), e.coalesce(A, B))  # coalesce(a, b, a): the nested form
    same(e.case_when([(C, A), (e.not_(C), B)], null), e.if_else(C, A, e.if_else(e.not_(C), B, null)))


# ----------------------------------------------------------------------------- through the operators
def test_through_selection_aggregate_group_by_order_by_and_an_outer_join(ctx):
    from naive_query_engine_amd import AggregateFunc, Column, DType, Field, Operator, RecordBatch
    from naive_query_engine_amd import physical_plan as pp

    e, n = E(), 5000
    r = cu.rng_for("operators")
    ids = np.arange(n, dtype=np.int64)
    d = r.integers(-5, 6, n).astype(np.int64)
    dmask = cu.mask_of(n, 41)
    v = (r.integers(-100, 101, n) / 2.0).astype(np.float64)
    vmask = cu.mask_of(n, 42)
    k = r.integers(0, 7, n).astype(np.int64)
    kmask = cu.mask_of(n, 43)
    names = [b"s%03d" % int(x) for x in r.integers(0, 40, n)]
    smask = cu.mask_of(n, 44)
    cols = [Column.from_numpy(ids), Column.from_numpy(d, dmask), Column.from_numpy(v, vmask), Column.from_numpy(k, kmask), utf8_column(names, smask)]
    f = fields("id", "d", "v", "k", "s")
    t = ctx.table_from_host(cols)
    ID, D, V, K, S = (e.col(i) for i in range(5))

    # where d is null (the anti-join idiom): is_null is never NULL, so exactly the NULL rows stay
    out = ctx.selection(t, e.is_null(D).flatten(f)).to_host()
    assert (out[0].to_numpy() == ids[~dmask]).all() and 0 < out[0].length < n and not out[1].valid_mask().any()
    # where not (d > 0 and v > 0): NULL where the conjunction is NULL (those rows are emitted as NULL rows, quirk Q4)
    conj = e.binop(e.binop(D, Operator.Gt, e.lit_i64(0)), Operator.And, e.binop(V, Operator.Gt, e.lit_f64(0.0)))
    dg, vg = (d > 0), (v > 0)
    c_false = (dmask & ~dg) | (vmask & ~vg)
    c_true = dmask & dg & vmask & vg
    c_null = ~c_false & ~c_true
    keep = c_false | c_null  # not(false) = true: kept; not(NULL) = NULL: a NULL row
    out = ctx.selection(t, e.not_(conj).flatten(f)).to_host()
    assert out[0].length == int(keep.sum()) and c_true.any() and c_null.any() and c_false.any()
    assert (out[0].valid_mask() == c_false[keep]).all() and (out[0].to_numpy()[c_false[keep]] == ids[c_false]).all()
    # the same predicate in selection + projection, the node in the projection list too
    out = ctx.selection_projection(t, e.is_not_null(D).flatten(f), [e.coalesce(V, e.lit_f64(-1.0)).flatten(f), ID.flatten(f)]).to_host()
    assert (out[1].to_numpy() == ids[dmask]).all() and (out[0].to_numpy() == np.where(vmask, v, -1.0)[dmask]).all() and out[0].validity is None
    # sum(case when v > 0 then 1 else 0 end): a projection under the aggregate (a NULL v takes the else branch)
    case = e.if_else(e.binop(V, Operator.Gt, e.lit_f64(0.0)), e.lit_i64(1), e.lit_i64(0))
    proj = ctx.projection(t, [case.flatten(f), K.flatten(f)])
    ones = (vmask & (v > 0)).astype(np.int64)
    assert (proj.to_host()[0].to_numpy() == ones).all() and 0 < ones.sum() < n
    total = ctx.aggregate(proj, [(AggregateFunc.Sum, 0)]).to_host()[0].to_numpy()
    assert total.tolist() == [float(ones.sum())]
    # the node as the aggregate's predicate and as its group key: group by coalesce(k, -1)
    key = e.coalesce(K, e.lit_i64(-1))
    kk = np.where(kmask, k, -1)
    out, keys = ctx.aggregate(t, [(AggregateFunc.Count, 0), (AggregateFunc.Sum, 0)], group_nodes=key.flatten(f), pred_nodes=e.is_not_null(V).flatten(f), with_keys=True)
    got = {int(g): (int(c), float(s)) for g, c, s in zip(keys.to_host()[0].to_numpy(), out.to_host()[0].to_numpy(), out.to_host()[1].to_numpy())}
    want = {int(g): (int((vmask & (kk == g)).sum()), float(ids[vmask & (kk == g)].sum())) for g in np.unique(kk[vmask])}
    assert got == want and -1 in want and len(want) == 8
    out = ctx.group_aggregate(t, [key.flatten(f)], [(AggregateFunc.Count, 0)], pred_nodes=e.not_(e.is_null(V)).flatten(f)).to_host()
    assert out[0].to_numpy().tolist() == sorted(want) and out[1].to_numpy().astype(np.int64).tolist() == [want[g][0] for g in sorted(want)]
    # order by coalesce(s, '') through the mirror: the NULL names sort as the empty string, the sort is stable
    schema = [Field("id", DType.INT64, True), Field("d", DType.INT64, True), Field("v", DType.FLOAT64, True), Field("k", DType.INT64, True), Field("s", DType.UTF8, True)]
    scan = pp.ScanPlan.create(pp.MemTable.try_create(schema, [RecordBatch(schema, cols)], ctx))
    plan = pp.PhysicalSortPlan.create(scan, [pp.PhysicalSortExpr.create(e.coalesce(e.col("s"), e.lit_utf8("")))])
    out = plan.execute()[0].table.to_host()
    filled = [names[i] if smask[i] else b"" for i in range(n)]
    assert out[0].to_numpy().tolist() == sorted(range(n), key=lambda i: filled[i]) and len(out) == 5
    # a LEFT join's NULL-extended column, then coalesce over it
    dim = [Column.from_numpy(np.arange(0, 7, 2, dtype=np.int64)), utf8_column([b"zero", b"two", b"four", b"six"])]
    dschema = [Field("kid", DType.INT64, True), Field("name", DType.UTF8, True)]
    fact = [Column.from_numpy(k), Column.from_numpy(ids)]
    fschema = [Field("k", DType.INT64, True), Field("id", DType.INT64, True)]
    ls = pp.ScanPlan.create(pp.MemTable.try_create(dschema, [RecordBatch(dschema, dim)], ctx))
    rs = pp.ScanPlan.create(pp.MemTable.try_create(fschema, [RecordBatch(fschema, fact)], ctx))
    join = pp.HashOuterJoin.create(ls, rs, [(pp.ColumnRef(None, "kid"), pp.ColumnRef(None, "k"))], pp.JoinType.Right, dschema + fschema)
    joined = join.execute()
    jt = joined[0].table
    jf = fields("kid", "name", "k", "id")
    res = ctx.projection(jt, [e.coalesce(e.col(1), e.lit_utf8("unknown")).flatten(jf), e.col(3).flatten(jf), e.is_null(e.col(0)).flatten(jf)]).to_host()
    label = {0: b"zero", 2: b"two", 4: b"four", 6: b"six"}
    by_id = dict(zip(res[1].to_numpy().tolist(), byte_strings(res[0])))
    assert len(by_id) == n and all(by_id[i] == label.get(int(k[i]), b"unknown") for i in range(n))
    assert res[0].validity is None and (res[2].to_numpy() == np.array([int(k[i]) not in label for i in res[1].to_numpy()])).all() and res[2].to_numpy().any()


def test_through_a_window_key_and_a_sort_key_of_every_word_type(ctx):
    """order by coalesce(d, 0) desc, then the rows' ids: the sort key is evaluated into a temporary column the output drops"""
    from naive_query_engine_amd import Column, DType, Field, RecordBatch
    from naive_query_engine_amd import physical_plan as pp

    e, n = E(), 3000
    r = cu.rng_for("sort")
    d, dmask, ids = r.integers(-50, 51, n).astype(np.int64), cu.mask_of(n, 51), np.arange(n, dtype=np.int64)
    schema = [Field("id", DType.INT64, True), Field("d", DType.INT64, True)]
    cols = [Column.from_numpy(ids), Column.from_numpy(d, dmask)]
    scan = pp.ScanPlan.create(pp.MemTable.try_create(schema, [RecordBatch(schema, cols)], ctx))
    key = e.coalesce(e.col("d"), e.lit_i64(0))
    out = pp.PhysicalSortPlan.create(scan, [pp.PhysicalSortExpr.create(key, descending=True)]).execute()[0].table.to_host()
    filled = np.where(dmask, d, 0)
    assert out[0].to_numpy().tolist() == sorted(range(n), key=lambda i: -int(filled[i])) and len(out) == 2
    # a window partitioned by the node: row_number() over (partition by coalesce(d, 0) order by id); the rows leave in input order
    from naive_query_engine_amd import WindowFunc

    win = pp.PhysicalWindowPlan.create(scan, [key], [pp.PhysicalSortExpr.create(e.col("id"))], [pp.WindowFunction.create(WindowFunc.RowNumber)])
    got = win.execute()[0].table.to_host()
    assert len(got) == 3 and (got[0].to_numpy() == ids).all()
    seen, want = {}, np.zeros(n, dtype=np.int64)
    for i in range(n):
        seen[int(filled[i])] = want[i] = seen.get(int(filled[i]), 0) + 1
    assert (got[2].to_numpy().astype(np.int64) == want).all() and want.max() > 1 and (~dmask).any()


# ----------------------------------------------------------------------------- the errors, at the C ABI, in their order
def test_the_errors_at_the_c_abi_in_their_order(ctx):
    from naive_query_engine_amd import Column, ErrorCode, PhysicalLiteralExpr, ScalarValue, Status
    from naive_query_engine_amd.arrow_host import node_column, node_conditional

    e, n = E(), 100
    cols = [Column.from_numpy(np.arange(n, dtype=np.int64)), Column.from_numpy(np.arange(n, dtype=np.uint64)), Column.from_numpy(np.arange(n) % 2 == 0),
            Column.from_numpy(np.arange(n, dtype=np.float64)), utf8_column([b"ab"] * n)]
    f = fields("i", "u", "b", "v", "s")
    t = ctx.table_from_host(cols)
    I, U, B, V, S = (e.col(k) for k in range(5))
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

    def raw(op, count, operands):
        nodes = []
        for x in operands:
            nodes += x.flatten(f)
        return nodes + [node_conditional(op, count)]

    null_typed = PhysicalLiteralExpr.create(ScalarValue.Null())
    # 1. `column` outside 1..3 — before the unknown op, the empty stack, the Null-typed operand and the non-Boolean condition
    for count in (0, -1, 4, 100):
        assert status_of(raw(99, count, [])) == Status.InvalidArgument
        assert status_of(raw(NOT, count, [null_typed])) == Status.InvalidArgument
        assert status_of(raw(NOT, count, [I])) == Status.InvalidArgument
        assert status_of(raw(IF, count, [B, I, I])) == Status.InvalidArgument
    # 2. `op` outside nqe_cond_operator
    for op in (6, 13, -1, 1000):
        for count in (1, 2, 3):
            assert status_of(raw(op, count, [])) == Status.InvalidArgument
            assert status_of(raw(op, count, [null_typed, I, V])) == Status.InvalidArgument
    # 3. `column` differs from the arity
    for op in range(6):
        for count in (1, 2, 3):
            if count != cu.ARITY[op]:
                assert status_of(raw(op, count, [null_typed, null_typed, null_typed])) == Status.InvalidArgument
                assert status_of(raw(op, count, [I, V, S])) == Status.InvalidArgument
    # 4. fewer values than the node pops
    assert status_of(raw(NOT, 1, [])) == Status.InvalidArgument
    assert status_of(raw(NULLIF, 2, [null_typed])) == Status.InvalidArgument
    assert status_of(raw(IF, 3, [I, V])) == Status.InvalidArgument
    # 5. a Null-typed operand — before 6. and 7.
    assert status_of(raw(NOT, 1, [null_typed])) == Status.NotSupported
    assert status_of(raw(IS_NULL, 1, [null_typed])) == Status.NotSupported
    assert status_of(raw(COALESCE, 2, [I, null_typed])) == Status.NotSupported
    assert status_of(raw(IF, 3, [I, null_typed, V])) == Status.NotSupported
    # 6. NOT's operand or IF's condition not Boolean
    for c in (I, U, V, S, e.lit_i64(1), e.lit_null(dtype_of("i64"))):
        assert status_of(raw(NOT, 1, [c])) == Status.IntervalError
        assert status_of(raw(IF, 3, [c, I, I])) == Status.IntervalError
    # 7. the value operands differ in dtype
    for x, y in ((I, U), (I, V), (V, S), (S, B), (B, I), (V, e.lit_i64(0)), (S, e.lit_null(dtype_of("i64")))):
        for op in (COALESCE, NULLIF):
            assert status_of(raw(op, 2, [x, y])) == Status.IntervalError
        assert status_of(raw(IF, 3, [B, x, y])) == Status.IntervalError
    # a zeroed kind-7 node and kind 8
    zeroed = node_conditional(0, 0)
    assert status_of([node_column(2), zeroed]) == Status.InvalidArgument
    eight = node_conditional(NOT, 1)
    eight.kind = 8
    assert status_of([node_column(2), eight]) == Status.InvalidArgument
    # and well-formed calls still work on this context
    assert ctx.expr_evaluate(t, e.not_(B).flatten(f)).to_host()[0].to_numpy().tolist() == [k % 2 == 1 for k in range(n)]
    assert ctx.selection(t, e.not_(B).flatten(f)).to_host()[0].length == n // 2
