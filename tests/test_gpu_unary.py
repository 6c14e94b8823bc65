"""GPU: PhysicalUnaryExpr (abs / sin / cos / tan over Float64, src/physical_plan/expression/unary.rs) through nqe_expr_evaluate,
the operators that take expression trees, and the host mirrors.  The model is numpy in float64 (np.abs bit-exact; np.sin / np.cos
within unary_util.TRIG_ULPS; + - * and compares on float64 are IEEE and bit-identical to the device's) plus the reference's
recorded vectors (tests/golden/unary_expected.json).  Every tree is run in three forms — interpreted, run-time compiled,
node-at-a-time — whose results must be bit-identical."""
import json
import os

import numpy as np
import pytest

from tests.helpers import fields
from tests.unary_util import FORMS, TRIG_ULPS, assert_clear_of_threshold, bits, environment, ulp_distance

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACCURACY = os.path.join(ROOT, "profiles", "unary", "accuracy.txt")
N = 100_003  # odd, above one 4096-row tile
SIGN = np.uint64(0x7FFFFFFFFFFFFFFF)


@pytest.fixture(scope="module")
def ctx():
    from naive_query_engine_amd import capi

    c = capi.Context(0)
    yield c
    c.close()


def record_accuracy(what, worst):
    """the maximum distance observed goes into profiles/unary/accuracy.txt (one line per case, replaced on a re-run)"""
    print(f"max ulp distance, {what}: {worst:g} (bound {TRIG_ULPS})")
    lines = []
    if os.path.exists(ACCURACY):
        with open(ACCURACY) as f:
            lines = [l for l in f.read().splitlines() if not l.startswith(what + ":")]
    lines.append(f"{what}: max {worst:g} ulp against numpy float64 (bound {TRIG_ULPS})")
    try:
        os.makedirs(os.path.dirname(ACCURACY), exist_ok=True)
        with open(ACCURACY, "w") as f:
            f.write("\n".join(sorted(lines)) + "\n")
    except OSError:
        pass  # a read-only checkout: the figure is still printed


def table(ctx, n=N, seed=5, nullable=False):
    from naive_query_engine_amd import Column

    rng = np.random.default_rng(seed)
    ids = np.arange(n, dtype=np.int64)
    v = rng.random(n) * 200.0 - 100.0
    mask = (rng.random(n) > 0.1) if nullable else None
    return ids, v, (mask if nullable else np.ones(n, dtype=bool)), ctx.table_from_host([Column.from_numpy(ids), Column.from_numpy(v, mask)])


def unary(func, e):
    from naive_query_engine_amd.expression import unop

    return unop(func, e)


def evaluate(ctx, t, expr):
    c = ctx.expr_evaluate(t, expr.flatten(fields("id", "v"))).to_host()[0]
    return c.to_numpy(), c.valid_mask()


# ----------------------------------------------------------------------------- the reference's two unit tests
def test_reference_unit_tests_abs_and_sin_of_score(ctx, csv_tables):
    from naive_query_engine_amd import DType, UnaryOperator
    from naive_query_engine_amd.expression import col

    with open(os.path.join(ROOT, "tests", "golden", "unary_expected.json")) as f:
        exp = json.load(f)
    batch = csv_tables["test_data"]
    t = ctx.table_from_host(batch.columns)
    for form, env in FORMS.items():
        with environment(**env):
            got = ctx.expr_evaluate(t, unary(UnaryOperator.Abs, col("score")).flatten(batch.fields)).to_host()[0]
            assert got.dtype == DType.FLOAT64 and (bits(got.to_numpy()) == bits(exp["abs"])).all(), form
            got = ctx.expr_evaluate(t, unary(UnaryOperator.Sin, col("score")).flatten(batch.fields)).to_host()[0]
            d = ulp_distance(got.to_numpy(), exp["sin"])
            assert d.max() <= TRIG_ULPS, (form, d)
    record_accuracy("sin(score) against the reference's recorded vector", d.max())


def test_reference_unit_tests_through_the_python_plan_mirror(csv_tables):
    from naive_query_engine_amd import DType, Field, PhysicalUnaryExpr, UnaryOperator
    from naive_query_engine_amd.expression import col
    from naive_query_engine_amd.physical_plan import MemTable, ProjectionPlan, ScanPlan

    with open(os.path.join(ROOT, "tests", "golden", "unary_expected.json")) as f:
        exp = json.load(f)
    batch = csv_tables["test_data"]
    scan = ScanPlan.create(MemTable.try_create(batch.fields, [batch]), None)
    # name / return_type as the planner passes them ("todo", Int32): stored and ignored
    plan = ProjectionPlan.create(scan, [Field("a", DType.FLOAT64, False), Field("s", DType.FLOAT64, False)],
                                 [PhysicalUnaryExpr.create(col("score"), UnaryOperator.Abs, "todo", "Int32"),
                                  PhysicalUnaryExpr.create(col("score"), UnaryOperator.Sin, "todo", "Int32")])
    out = plan.execute()
    assert len(out) == 1
    cols = out[0].table.to_host()
    assert (bits(cols[0].to_numpy()) == bits(exp["abs"])).all()
    assert ulp_distance(cols[1].to_numpy(), exp["sin"]).max() <= TRIG_ULPS


# ----------------------------------------------------------------------------- abs: bit-exact
def special_values():
    nan_pos = np.array([0x7FF8000000000000, 0x7FF0000000000001, 0x7FFFFFFFFFFFFFFF], dtype=np.uint64)
    nan_neg = nan_pos | np.uint64(0x8000000000000000)
    sub = np.array([5e-324, -5e-324, 2.2250738585072009e-308, -2.2250738585072009e-308])
    return np.concatenate([np.array([0.0, -0.0, np.inf, -np.inf, 1.5, -1.5, 1.7976931348623157e308, -1.7976931348623157e308]), sub,
                           nan_pos.view(np.float64), nan_neg.view(np.float64)])


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 8191, 1_000_001])
@pytest.mark.parametrize("nullable", [False, True])
def test_abs_is_the_sign_bit_cleared_and_nothing_else(ctx, n, nullable):
    from naive_query_engine_amd import Column, DType, UnaryOperator
    from naive_query_engine_amd.expression import col

    rng = np.random.default_rng(n + 1)
    v = rng.integers(0, 2 ** 64, n, dtype=np.uint64).view(np.float64).copy()  # random bit patterns: every exponent, NaNs included
    sp = special_values()
    v[: min(n, len(sp))] = sp[: min(n, len(sp))]
    mask = (rng.random(n) > 0.2) if nullable else None
    t = ctx.table_from_host([Column.from_numpy(v, mask)])
    exp = bits(v) & SIGN
    finite = ~np.isnan(v)
    assert (exp[finite] == bits(np.abs(v[finite]))).all()  # the model is np.abs (NaNs: compared as bits with the sign cleared)
    for form, env in FORMS.items():
        with environment(**env):
            got = ctx.expr_evaluate(t, unary(UnaryOperator.Abs, col(0)).flatten(fields("v"))).to_host()[0]
        assert got.dtype == DType.FLOAT64 and got.length == n, form
        valid = got.valid_mask()
        assert (valid == (mask if nullable else np.ones(n, dtype=bool))).all(), form
        assert (bits(got.to_numpy())[valid] == exp[valid]).all(), form


# ----------------------------------------------------------------------------- sin / cos / tan (= cos, quirk Q16)
def trig_inputs():
    dense = np.linspace(-100.0, 100.0, 400_001)
    k = np.arange(-2000, 2001, dtype=np.float64)
    half_pi = k * (np.pi / 2)  # multiples of pi/2 rounded to double
    big = np.array([1e6, -1e6, 1e15, -1e15, 1e300, -1e300, 1e22, 5e-324, -5e-324, 1e-300])
    return np.concatenate([dense, half_pi, big, np.array([0.0, -0.0])])


@pytest.mark.parametrize("name", ["Sin", "Cos", "Tan"])
def test_sin_cos_tan_within_the_specified_bound_of_numpy(ctx, name):
    from naive_query_engine_amd import Column, UnaryOperator
    from naive_query_engine_amd.expression import col

    x = trig_inputs()
    model = np.sin(x) if name == "Sin" else np.cos(x)  # Tan evaluates the cosine (quirk Q16, unary.rs:96)
    t = ctx.table_from_host([Column.from_numpy(x)])
    results = {}
    for form, env in FORMS.items():
        with environment(**env):
            results[form] = ctx.expr_evaluate(t, unary(UnaryOperator[name], col(0)).flatten(fields("v"))).to_host()[0].to_numpy()
    for form, got in results.items():
        assert (bits(got) == bits(results["interpreter"])).all(), form
    got = results["interpreter"]
    d = ulp_distance(got, model)
    record_accuracy(f"{name.lower()}(x) over [-100, 100] dense, multiples of pi/2, +-1e6, +-1e15, +-1e300", d.max())
    assert d.max() <= TRIG_ULPS, (name, x[np.argmax(d)], got[np.argmax(d)], model[np.argmax(d)])
    if name == "Sin":  # sin(-0.0) is -0.0, sin(+0.0) is +0.0
        assert bits(got[-1:])[0] == 0x8000000000000000 and bits(got[-2:-1])[0] == 0
    # +-inf and NaN give NaN
    bad = np.array([np.inf, -np.inf, np.nan])
    got = ctx.expr_evaluate(ctx.table_from_host([Column.from_numpy(bad)]), unary(UnaryOperator[name], col(0)).flatten(fields("v"))).to_host()[0].to_numpy()
    assert np.isnan(got).all()


@pytest.mark.parametrize("name", ["Sin", "Cos"])
@pytest.mark.parametrize("nullable", [False, True])
def test_hard_arguments_reach_the_stack_machine_and_the_compiled_kernel(ctx, name, nullable):
    """A bare f(column) takes the node kernel in every form, so the large arguments (+-1e15, +-1e300, 1e22), the multiples of pi/2 and
    the subnormals go through a three-step tree as well — abs(f(v * 1.0)): `* 1.0` and abs are exact — and each form is checked to
    have run the kernel it stands for."""
    from naive_query_engine_amd import Column, Operator, UnaryOperator
    from naive_query_engine_amd.expression import binop, col, lit_f64

    x = trig_inputs()
    rng = np.random.default_rng(3)
    mask = (rng.random(len(x)) > 0.1) if nullable else None
    valid = mask if nullable else np.ones(len(x), dtype=bool)
    t = ctx.table_from_host([Column.from_numpy(x, mask)])
    nodes = unary(UnaryOperator.Abs, unary(UnaryOperator[name], binop(col(0), Operator.Multiply, lit_f64(1.0)))).flatten(fields("v"))
    expected_kernel = {"interpreter": "expr_tree", "compiled": "expr_jit", "node_at_a_time": "expr_unary"}
    results = {}
    ctx.timing_enable(True)
    try:
        for form, env in FORMS.items():
            with environment(**env):
                ctx.timing_reset()
                c = ctx.expr_evaluate(t, nodes).to_host()[0]
                ran = set(ctx.timing_report())
            assert expected_kernel[form] in ran, (form, ran)
            assert not ({"expr_tree", "expr_jit", "expr_unary"} - {expected_kernel[form]}) & ran, (form, ran)
            results[form] = (c.to_numpy(), c.valid_mask())
    finally:
        ctx.timing_enable(False)
    base = results["interpreter"][0]
    for form, (g, gv) in results.items():
        assert (gv == valid).all(), form
        assert (bits(g[valid]) == bits(base[valid])).all(), form
    model = np.abs(np.sin(x) if name == "Sin" else np.cos(x))
    d = ulp_distance(base[valid], model[valid])
    record_accuracy(f"abs({name.lower()}(x * 1.0)) in the stack machine and the compiled kernel, the same inputs{', nullable' if nullable else ''}", d.max())
    assert d.max() <= TRIG_ULPS, (name, d.max())


# ----------------------------------------------------------------------------- errors, decided before any launch
def test_error_cases(ctx):
    from naive_query_engine_amd import Column, DType, ErrorCode, ScalarValue, Status, UnaryOperator
    from naive_query_engine_amd.arrow_host import node_column, node_unary
    from naive_query_engine_amd.expression import PhysicalLiteralExpr, col

    n = 100
    t = ctx.table_from_host([Column.from_numpy(np.arange(n, dtype=np.int64)), Column.from_numpy(np.arange(n, dtype=np.uint64)),
                             Column.from_numpy(np.arange(n) % 2 == 0), Column.from_list(["a"] * n, DType.UTF8), Column.from_numpy(np.ones(n))])
    f = fields("i", "u", "b", "s", "v")

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

    for func in (UnaryOperator.Abs, UnaryOperator.Sin, UnaryOperator.Cos, UnaryOperator.Tan):
        for c in range(4):  # Int64, UInt64, Boolean, Utf8: unimplemented!() (unary.rs:41)
            assert status_of(unary(func, col(c)).flatten(f)) == Status.NotSupported, (func, c)
        assert status_of(unary(func, PhysicalLiteralExpr.create(ScalarValue.Null())).flatten(f)) == Status.NotSupported
        assert status_of(unary(func, PhysicalLiteralExpr.create(ScalarValue.Int64(3))).flatten(f)) == Status.NotSupported
    for func in list(UnaryOperator)[4:]:  # the string functions: todo!() whatever the child (unary.rs:97-106)
        for c in range(5):
            assert status_of(unary(func, col(c)).flatten(f)) == Status.NotSupported, (func, c)
    assert status_of([node_unary(UnaryOperator.Abs)]) == Status.InvalidArgument              # nothing on the stack
    bad = node_unary(UnaryOperator.Abs)
    for op in (14, -1, 1000):
        bad.op = op
        assert status_of([node_column(4), bad]) == Status.InvalidArgument                      # outside nqe_unary_operator
    # and the well-formed call still works on this context
    assert (ctx.expr_evaluate(t, unary(UnaryOperator.Abs, col(4)).flatten(f)).to_host()[0].to_numpy() == 1.0).all()


def test_unary_output_shares_the_columns_validity_buffer(ctx):
    from naive_query_engine_amd import Column, UnaryOperator
    from naive_query_engine_amd.expression import col

    rng = np.random.default_rng(1)
    v = rng.random(5000)
    t = ctx.table_from_host([Column.from_numpy(v, rng.random(5000) > 0.5)])
    out = ctx.expr_evaluate(t, unary(UnaryOperator.Abs, col(0)).flatten(fields("v")))
    assert out.column_info(0).validity == t.column_info(0).validity  # reference-counted alias, no copy
    assert out.column_info(0).values != t.column_info(0).values


def test_unary_over_a_borrowed_column_copies_the_validity(ctx):
    """memory borrowed from the caller may not be aliased by an output: the bitmap is copied, the result is the same"""
    from naive_query_engine_amd import Column, DType, UnaryOperator
    from naive_query_engine_amd.arrow_host import pack_bits
    from naive_query_engine_amd.expression import col

    n = 10_007
    rng = np.random.default_rng(2)
    v = rng.random(n) * 10.0 - 5.0
    mask = rng.random(n) > 0.3
    packed = np.zeros((n + 63) // 64 * 8 + 8, dtype=np.uint8)
    pb = pack_bits(mask)
    packed[: len(pb)] = pb
    # the caller's own device memory, filled through nqe_table_pack_words (column words back to back + a row-count word)
    words = packed.view(np.uint64)
    pv, pm = ctx.device_alloc((n + 1) * 8), ctx.device_alloc((len(words) + 1) * 8)
    ctx.pack_words([ctx.table_from_host([Column.from_numpy(v)])], n, pv)
    ctx.pack_words([ctx.table_from_host([Column.from_numpy(words)])], len(words), pm)
    ctx.synchronize()
    t = ctx.table_from_device([(DType.FLOAT64, n, pv, pm)])
    for form, env in FORMS.items():
        with environment(**env):
            out = ctx.expr_evaluate(t, unary(UnaryOperator.Abs, col(0)).flatten(fields("v")))
        info = out.column_info(0)
        assert info.validity and info.validity != pm and info.values != pv, form
        c = out.to_host()[0]
        assert (c.valid_mask() == mask).all() and (bits(c.to_numpy()[mask]) == bits(np.abs(v)[mask])).all(), form
        del out
    del t
    ctx.device_free(pv)
    ctx.device_free(pm)


# ----------------------------------------------------------------------------- trees, three forms each
def in_three_forms(run):
    return {form: _with(env, run) for form, env in FORMS.items()}


def _with(env, run):
    with environment(**env):
        return run()


def host_cols(t):
    return [(c.to_numpy(), c.valid_mask()) for c in t.to_host()]


def assert_forms_identical(results):
    base = results["interpreter"]
    for form, got in results.items():
        assert len(got) == len(base), form
        for (g, gv), (b, bv) in zip(got, base):
            assert g.shape == b.shape and (gv == bv).all(), form
            gg, bb = g[gv], b[bv]
            if g.dtype == np.float64:
                assert (bits(gg) == bits(bb)).all(), form
            else:
                assert (gg == bb).all(), form


@pytest.mark.parametrize("nullable", [False, True])
def test_projection_trees(ctx, nullable):
    from naive_query_engine_amd import Operator, UnaryOperator
    from naive_query_engine_amd.expression import binop, col, lit_f64

    ids, v, mask, t = table(ctx, nullable=nullable)
    f = fields("id", "v")
    exprs = [unary(UnaryOperator.Abs, binop(col(1), Operator.Minus, lit_f64(50.0))),        # abs(v - 50.0)
             binop(unary(UnaryOperator.Sin, col(1)), Operator.Multiply, lit_f64(2.0)),       # sin(v) * 2.0
             unary(UnaryOperator.Abs, lit_f64(-3.5)),                                        # a literal child: num_rows copies of 3.5
             unary(UnaryOperator.Tan, binop(col(1), Operator.Multiply, lit_f64(0.5)))]       # tan(v * 0.5) = cos(v * 0.5) (Q16)
    results = in_three_forms(lambda: host_cols(ctx.projection(t, [e.flatten(f) for e in exprs])))
    assert_forms_identical(results)
    got = results["interpreter"]
    for k in (0, 1, 3):
        assert (got[k][1] == mask).all()
    assert got[2][1].all() and (bits(got[2][0]) == bits(np.full(N, 3.5))).all()
    assert (bits(got[0][0][mask]) == bits(np.abs(v - 50.0)[mask])).all()                     # arithmetic below abs: bit for bit
    d = ulp_distance(got[1][0][mask], (np.sin(v) * 2.0)[mask])                               # * 2.0 is exact: the bound carries through
    assert d.max() <= TRIG_ULPS, d.max()
    assert ulp_distance(got[3][0][mask], np.cos(v * 0.5)[mask]).max() <= TRIG_ULPS


@pytest.mark.parametrize("nullable", [False, True])
def test_selection_by_a_unary_predicate(ctx, nullable):
    from naive_query_engine_amd import Operator, UnaryOperator
    from naive_query_engine_amd.expression import binop, col, lit_f64

    ids, v, mask, t = table(ctx, nullable=nullable)
    f = fields("id", "v")
    pred = binop(unary(UnaryOperator.Abs, binop(col(1), Operator.Minus, lit_f64(50.0))), Operator.Lt, lit_f64(10.0))  # abs(v - 50.0) < 10.0
    assert_clear_of_threshold(np.abs(v - 50.0), 10.0, "abs(v - 50.0) < 10.0")
    results = in_three_forms(lambda: host_cols(ctx.selection(t, pred.flatten(f))))
    assert_forms_identical(results)
    (gid, gidv), (gv, gvv) = results["interpreter"]
    keep = mask & (np.abs(v - 50.0) < 10.0)
    assert (gid[gidv] == ids[keep]).all() and (bits(gv[gvv]) == bits(v[keep])).all()
    assert len(gid) == keep.sum() + (~mask).sum()  # a NULL predicate emits a NULL row (quirk Q4)


@pytest.mark.parametrize("nullable", [False, True])
def test_fused_selection_projection_with_unary_nodes(ctx, nullable):
    from naive_query_engine_amd import Operator, UnaryOperator
    from naive_query_engine_amd.expression import binop, col, lit_f64

    ids, v, mask, t = table(ctx, nullable=nullable)
    f = fields("id", "v")
    pred = binop(binop(unary(UnaryOperator.Sin, col(1)), Operator.Multiply, lit_f64(2.0)), Operator.Gt, lit_f64(0.5))  # sin(v) * 2.0 > 0.5
    assert_clear_of_threshold(np.sin(v) * 2.0, 0.5, "sin(v) * 2.0 > 0.5")
    exprs = [unary(UnaryOperator.Abs, binop(col(1), Operator.Minus, lit_f64(50.0))), col(0),
             binop(unary(UnaryOperator.Cos, col(1)), Operator.Plus, col(1))]
    results = in_three_forms(lambda: host_cols(ctx.selection_projection(t, pred.flatten(f), [e.flatten(f) for e in exprs])))
    assert_forms_identical(results)
    (ga, gav), (gid, gidv), (gc, gcv) = results["interpreter"]
    keep = mask & (np.sin(v) * 2.0 > 0.5)
    assert len(gid) == keep.sum() + (~mask).sum()
    assert (gid[gidv] == ids[keep]).all()                                                    # the row sets match exactly
    assert (bits(ga[gav]) == bits(np.abs(v - 50.0)[keep])).all()
    # cos(v) + v: one operator above the transcendental; its 5 ulp (of a value <= 1) are at most 5 * 2^-53 absolute, the sum's own rounding half an ulp of it
    assert np.abs(gc[gcv] - (np.cos(v) + v)[keep]).max() <= TRIG_ULPS * 2.0 ** -53 + 2.0 ** -46


@pytest.mark.parametrize("mod", [7, 1024])  # 7: the issue's query; 1024: the shape the run-time compiled aggregate kernel takes
@pytest.mark.parametrize("nullable", [False, True])
def test_aggregate_under_a_unary_predicate(ctx, nullable, mod):
    from naive_query_engine_amd import AggregateFunc, Column, Operator, UnaryOperator
    from naive_query_engine_amd.expression import binop, col, lit_f64, lit_i64
    from oracle import oracle as orc

    n = 300_007
    ids, v, mask, t = table(ctx, n=n, seed=9, nullable=nullable)
    f = fields("id", "v")
    pred = binop(unary(UnaryOperator.Cos, col(1)), Operator.Gt, lit_f64(0.25))               # cos(v) > 0.25
    assert_clear_of_threshold(np.cos(v), 0.25, "cos(v) > 0.25")
    key = binop(col(0), Operator.Modulos, lit_i64(mod)).flatten(f)
    aggs = [(AggregateFunc.Count, 1), (AggregateFunc.Sum, 1), (AggregateFunc.Min, 1), (AggregateFunc.Max, 1)]

    def run():
        out = ctx.aggregate(t, aggs, group_nodes=key, pred_nodes=pred.flatten(f))
        m = np.stack([c.to_numpy().astype(np.float64) for c in out.to_host()], axis=1)
        return m[np.lexsort(m.T[::-1])]

    results = in_three_forms(run)
    # the model: the same aggregate by the CPU oracle over the predicate's numpy value as a Boolean column (NULL where v is NULL)
    cols = [Column.from_numpy(ids), Column.from_numpy(v, mask if nullable else None), Column.from_numpy(np.cos(v) > 0.25, mask if nullable else None)]
    exp = orc.aggregate([cols], aggs, group_nodes=key, pred_nodes=col(2).flatten(fields("id", "v", "p")))[0]
    e = np.stack([c.to_numpy().astype(np.float64) for c in exp], axis=1)
    e = e[np.lexsort(e.T[::-1])]
    for form, g in results.items():
        assert g.shape == e.shape, (form, g.shape, e.shape)
        assert (g[:, 0] == e[:, 0]).all() and (g[:, 2] == e[:, 2]).all() and (g[:, 3] == e[:, 3]).all(), form   # counts, min, max exact
        assert np.allclose(g[:, 1], e[:, 1], rtol=1e-9, atol=0), form                                             # Float64 sums
        assert (g[:, [0, 2, 3]] == results["interpreter"][:, [0, 2, 3]]).all(), form
