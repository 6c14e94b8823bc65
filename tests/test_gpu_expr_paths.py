"""Pins the expression unit's dispatch: for a query of every path through csrc/expr.hip (a bare column or literal, the node-at-a-time
kernels, the interpreting stack machine with its (nullable, <=2 / <=4 columns, trig) instances, the same machine behind a selection, the
selection's recognised predicate shapes, the flag read-back, and the four run-time specialised kernels with their interpreting
stand-ins) the kernels launched — every label of the context's timing report with its launch count — by each of THREE executions, and
every execution's result against numpy computed here.  The expected launches are data: tests/golden/expr_paths.json, recorded once
(python -m tests.test_gpu_expr_paths --record, which refuses to overwrite an existing file) from the library as it was before expr.hip
was split into expr_shapes.hpp / expr_plan.hpp / expr_kernels.hpp; the test only ever reads it.

Every case runs in a context of its own (the specialised kernels are cached per context).  Row counts come from {1, 63, 257, 8449}: below
a ballot word, past one 256-row chunk, and past two 4096-row tiles and one 6144-row step of the fused selection with a ragged end.  The
Float64 columns hold multiples of 0.25 of small magnitude and the integers are small, so every arithmetic result is exact; the `sin` cases
compare sin(v) with such a multiple, which no sine of a non-zero multiple of 0.25 comes within ulps of (and sin(0) = 0 exactly)."""
import contextlib
import dataclasses
import json
import os
import sys

import numpy as np
import pytest

from naive_query_engine_amd import AggregateFunc, Column, DType, Operator, UnaryOperator
from naive_query_engine_amd.arrow_host import ErrorCode, Status
from naive_query_engine_amd.expression import binop, col, lit_f64, lit_i64, lit_utf8, unop
from tests.helpers import fields

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "expr_paths.json")
SWITCHES = ("NQE_NO_EXPR_TREE", "NQE_NO_JIT", "NQE_JIT_MIN_ROWS", "NQE_NO_JIT_DISK_CACHE", "NQE_JIT_SYNC", "NQE_NO_FUSED_SELECT", "NQE_NO_AGG_JIT",
            "NQE_NO_PLAN_HINTS", "NQE_NO_KEY_SAMPLE", "NQE_DEBUG")
EXECUTIONS = 3
X, O, U = binop, Operator, UnaryOperator
ID, V, W, UU, XX, NV, S, Z, NI, F2 = range(10)
FLD = fields("id", "v", "w", "u", "x", "nv", "s", "z", "ni", "f2")
# With the disk cache off the first execution of a specialised case always interprets (its kernel is being compiled), and the two records
# taken from the parent's library in separate processes agree on it: nothing is left unpinned.
FIRST_EXECUTION_NOT_PINNED = ()


def make_table(n, rng):
    """[(values, validity mask or None)], in the order of FLD"""
    quarter = lambda: rng.integers(-200, 200, n).astype(np.float64) / 4.0
    small = lambda lo, hi: rng.integers(lo, hi, n).astype(np.int64)
    mask = lambda: rng.random(n) >= 0.2
    return [(rng.permutation(n).astype(np.int64) + 1, None), (quarter(), None), (small(-50, 50), None), (small(1, 20), None), (small(-50, 50), None), (quarter(), mask()),
            (np.array(["a", "b", "cé", ""], dtype=object)[rng.integers(0, 4, n)], None), (small(0, 4), None), (small(-50, 50), mask()), (quarter(), None)]


def upload(table):
    return [Column.from_list(v.tolist(), DType.UTF8) if v.dtype == object else Column.from_numpy(v, m) for v, m in table]


@dataclasses.dataclass
class Case:
    n: int
    op: str                              # evaluate | project | select | select_project | aggregate
    exprs: list = None                   # evaluate: [e]; project / select_project: the list; aggregate: [key]
    pred: object = None
    expect: object = None                # table -> [(values, validity mask or None)] of the result; None with `raises`
    raises: Status = None
    env: dict = dataclasses.field(default_factory=dict)
    jit: bool = False                    # wait for the specialised kernel after the first execution


def kept(table, keep, outs):
    """the rows `keep` emits (predicate true or NULL) of the outputs [(values, validity mask or None)]"""
    return [(v[keep], None if m is None else m[keep]) for v, m in outs]


def valid_of(table, c):
    m = table[c][1]
    return np.ones(len(table[c][0]), dtype=bool) if m is None else m


def c(table, i):
    return table[i][0]


JIT = {"NQE_JIT_MIN_ROWS": "1000", "NQE_NO_JIT_DISK_CACHE": "1"}
NO_JIT = dict(JIT, NQE_NO_JIT="1")
E_TREE4 = X(X(X(col(ID), O.Modulos, lit_i64(1000)), O.Multiply, lit_i64(3)), O.Plus, X(col(ID), O.Divide, lit_i64(7)))
E_VV = X(X(col(V), O.Multiply, col(V)), O.Plus, X(col(V), O.Divide, lit_f64(4.0)))
P_CHAIN = X(X(X(col(ID), O.Plus, lit_i64(1)), O.Modulos, lit_i64(10)), O.Lt, lit_i64(5))
E_WX_POS = X(X(col(W), O.Plus, col(XX)), O.Gt, lit_i64(0))
E_WXU = X(X(col(W), O.Multiply, col(XX)), O.Plus, col(UU))


def x_tree4(t):
    return [((c(t, ID) % 1000) * 3 + c(t, ID) // 7, None)]


def x_vv(t):
    return c(t, V) * c(t, V) + c(t, V) / 4.0


def x_compact(pred_col, lit):
    """`select w + x > 0, w * x + u where <pred_col> < lit`: a row whose predicate is NULL is emitted as a NULL row"""
    def expect(t):
        pv = valid_of(t, pred_col)
        keep = ~pv | (c(t, pred_col) < lit)
        m = None if t[pred_col][1] is None else pv
        return kept(t, keep, [(c(t, W) + c(t, XX) > 0, m), (c(t, W) * c(t, XX) + c(t, UU), m)])
    return expect


def x_select(keep_of):
    return lambda t: kept(t, keep_of(t), t)


def x_aggregate(t):
    key, w = c(t, ID) % 600, c(t, W)
    cnt = np.bincount(key, minlength=600)
    return [(cnt.astype(np.uint64), None), (np.bincount(key, weights=w, minlength=600), None)]  # (Count: UInt64; Sum: Float64, exact for small integers)


def specialised(env):
    return {
        "tree": Case(8449, "evaluate", [E_TREE4], expect=x_tree4, env=env, jit=True),
        "projection_list": Case(8449, "select_project", [E_VV, col(ID)], X(col(W), O.Lt, lit_i64(10)),
                                expect=lambda t: kept(t, c(t, W) < 10, [(x_vv(t), None), t[ID]]), env=env, jit=True),
        "select_project_one_pass": Case(8449, "select_project", [E_VV, col(ID)], P_CHAIN,
                                        expect=lambda t: kept(t, (c(t, ID) + 1) % 10 < 5, [(x_vv(t), None), t[ID]]), env=env, jit=True),
        "aggregate": Case(8449, "aggregate", [X(col(ID), O.Modulos, lit_i64(600))], expect=x_aggregate, env=env, jit=True),
    }


CASES = {
    "bare_column": Case(63, "evaluate", [col(V)], expect=lambda t: [t[V]]),
    "bare_literal": Case(257, "evaluate", [lit_i64(7)], expect=lambda t: [(np.full(257, 7, dtype=np.int64), None)]),
    "utf8_literal": Case(63, "evaluate", [lit_utf8("héllo")], expect=lambda t: [(np.array(["héllo"] * 63, dtype=object), None)]),
    "bare_abs": Case(8449, "evaluate", [unop(U.Abs, col(V))], expect=lambda t: [(np.abs(c(t, V)), None)]),
    "bare_abs_one_row": Case(1, "evaluate", [unop(U.Abs, col(V))], expect=lambda t: [(np.abs(c(t, V)), None)]),
    "one_binary_node": Case(8449, "evaluate", [X(col(V), O.Multiply, lit_f64(2.0))], expect=lambda t: [(c(t, V) * 2.0, None)]),
    "one_binary_node_no_expr_tree": Case(8449, "evaluate", [X(col(V), O.Multiply, lit_f64(2.0))], expect=lambda t: [(c(t, V) * 2.0, None)], env={"NQE_NO_EXPR_TREE": "1"}),
    "tree_2_columns": Case(8449, "evaluate", [X(col(V), O.Plus, X(col(F2), O.Multiply, lit_f64(2.0)))], expect=lambda t: [(c(t, V) + c(t, F2) * 2.0, None)]),
    "tree_2_columns_nullable": Case(8449, "evaluate", [X(col(V), O.Plus, X(col(NV), O.Multiply, lit_f64(2.0)))], expect=lambda t: [(c(t, V) + c(t, NV) * 2.0, t[NV][1])]),
    "tree_2_columns_sin": Case(8449, "evaluate", [X(unop(U.Sin, col(V)), O.Gt, col(F2))], expect=lambda t: [(np.sin(c(t, V)) > c(t, F2), None)]),
    "tree_4_columns": Case(8449, "evaluate", [X(X(col(W), O.Plus, X(col(XX), O.Multiply, col(UU))), O.Minus, col(ID))],
                           expect=lambda t: [(c(t, W) + c(t, XX) * c(t, UU) - c(t, ID), None)]),
    "tree_4_columns_nullable": Case(257, "evaluate", [X(X(X(col(W), O.Plus, col(XX)), O.Multiply, col(UU)), O.Plus, col(NI))],
                                    expect=lambda t: [((c(t, W) + c(t, XX)) * c(t, UU) + c(t, NI), t[NI][1])]),
    "tree_4_columns_sin": Case(8449, "evaluate", [X(X(unop(U.Sin, col(V)), O.Gt, col(F2)), O.And, X(col(W), O.Lt, col(XX)))],
                               expect=lambda t: [((np.sin(c(t, V)) > c(t, F2)) & (c(t, W) < c(t, XX)), None)]),
    "tree_5_columns_node_at_a_time": Case(257, "evaluate", [X(X(X(X(col(W), O.Plus, col(XX)), O.Plus, col(UU)), O.Plus, col(ID)), O.Plus, col(Z))],
                                          expect=lambda t: [(c(t, W) + c(t, XX) + c(t, UU) + c(t, ID) + c(t, Z), None)]),
    "utf8_compare": Case(257, "evaluate", [X(col(S), O.Eq, lit_utf8("cé"))], expect=lambda t: [(c(t, S) == "cé", None)]),
    "literal_op_literal": Case(63, "evaluate", [X(lit_i64(3), O.Plus, lit_i64(4))], expect=lambda t: [(np.full(63, 7, dtype=np.int64), None)]),
    "compact_tree": Case(8449, "select_project", [E_WX_POS, E_WXU], X(col(W), O.Lt, lit_i64(10)), expect=x_compact(W, 10)),
    "compact_tree_null_predicate_rows": Case(8449, "select_project", [E_WX_POS, E_WXU], X(col(NV), O.Lt, lit_f64(10.0)), expect=x_compact(NV, 10.0)),
    "compact_tree_one_row": Case(1, "select_project", [E_WX_POS, E_WXU], X(col(W), O.Lt, lit_i64(100)), expect=x_compact(W, 100)),
    "division_that_can_fault": Case(257, "project", [X(col(ID), O.Divide, col(UU)), col(W)], expect=lambda t: [(c(t, ID) // c(t, UU), None), t[W]]),
    "division_by_zero": Case(257, "project", [X(col(ID), O.Divide, col(Z))], raises=Status.ArrowError),
    "select_and_list": Case(8449, "select", pred=X(X(col(W), O.Lt, lit_i64(10)), O.And, X(col(XX), O.GtEq, lit_i64(0))),
                            expect=x_select(lambda t: (c(t, W) < 10) & (c(t, XX) >= 0))),
    "select_general_conj": Case(8449, "select", pred=X(X(col(W), O.Lt, lit_i64(10)), O.Or, X(X(col(ID), O.Modulos, lit_i64(3)), O.Eq, lit_i64(0))),
                                expect=x_select(lambda t: (c(t, W) < 10) | (c(t, ID) % 3 == 0))),
    "select_plain_compare": Case(63, "select", pred=X(col(W), O.Lt, lit_i64(10)), expect=x_select(lambda t: c(t, W) < 10)),
}
CASES.update({f"specialised_{k}": v for k, v in specialised(JIT).items()})
CASES.update({f"no_jit_{k}": v for k, v in specialised(NO_JIT).items()})


@contextlib.contextmanager
def switches(env):
    """the switches are read per call: exactly `env` is set while a case runs, and what was set before is restored"""
    saved = {k: os.environ.pop(k, None) for k in SWITCHES}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def launches(ctx):
    return {name: cnt for name, (_, cnt) in sorted(ctx.timing_report().items())}


def assert_columns(got, exp, what):
    assert len(got) == len(exp), f"{what}: {len(got)} columns, expected {len(exp)}"
    for i, (g, (v, m)) in enumerate(zip(got, exp)):
        assert g.length == len(v), f"{what}: column {i} has {g.length} rows, expected {len(v)}"
        m = np.ones(len(v), dtype=bool) if m is None else m
        assert np.array_equal(g.valid_mask(), m), f"{what}: validity of column {i}"
        if v.dtype == object:
            assert g.dtype == DType.UTF8 and g.to_list() == [s if ok else None for s, ok in zip(v.tolist(), m.tolist())], f"{what}: column {i}"
            continue
        gv = g.to_numpy()
        assert gv.dtype == v.dtype, f"{what}: column {i} is {gv.dtype}, expected {v.dtype}"
        assert np.array_equal(gv[m], v[m]), f"{what}: values of column {i}"


def execute(ctx, t, case):
    nodes = [e.flatten(FLD) for e in case.exprs or []]
    pn = case.pred.flatten(FLD) if case.pred is not None else None
    if case.op == "evaluate":
        return ctx.expr_evaluate(t, nodes[0]).to_host()
    if case.op == "project":
        return ctx.projection(t, nodes).to_host()
    if case.op == "select":
        return ctx.selection(t, pn).to_host()
    if case.op == "select_project":
        return ctx.selection_projection(t, pn, nodes).to_host()
    out = ctx.aggregate(t, [(AggregateFunc.Count, W), (AggregateFunc.Sum, W)], group_nodes=nodes[0]).to_host()
    order = np.lexsort([col_.to_numpy() for col_ in out][::-1])  # the groups come in table order: compared as sorted (count, sum) rows
    return [Column.from_numpy(col_.to_numpy()[order]) for col_ in out]


def run_case(name):
    """runs one case in a fresh context; returns the launches of each execution, every result checked against numpy"""
    from naive_query_engine_amd import capi

    case = CASES[name]
    table = make_table(case.n, np.random.default_rng(sum(map(ord, name))))
    exp = case.expect(table) if case.expect else None
    if case.op == "aggregate":
        order = np.lexsort([v for v, _ in exp][::-1])
        exp = [(v[order], None) for v, _ in exp]
    runs = []
    with switches(case.env):
        ctx = capi.Context(0)
        try:
            t = ctx.table_from_host(upload(table))
            for rep in range(EXECUTIONS):
                ctx.timing_enable(True)
                ctx.timing_reset()
                if case.raises is not None:
                    with pytest.raises(ErrorCode) as err:
                        execute(ctx, t, case)
                    assert err.value.status == case.raises, f"{name}: execution {rep}"
                else:
                    got = execute(ctx, t, case)
                ctx.timing_enable(False)
                runs.append(launches(ctx))
                if case.raises is None:
                    assert_columns(got, exp, f"{name}: execution {rep}")
                if case.jit and rep == 0:
                    ctx.jit_wait()
            del t
        finally:
            ctx.close()
    return runs


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as f:
        return json.load(f)


def test_the_fixture_covers_exactly_these_cases(recorded):
    assert sorted(recorded) == sorted(CASES)


@pytest.mark.parametrize("name", list(CASES))
def test_expr_path(recorded, name):
    got, exp = run_case(name), recorded[name]
    assert len(got) == len(exp) == EXECUTIONS
    assert [i for i, e in enumerate(exp) if e is None] == ([0] if name in FIRST_EXECUTION_NOT_PINNED else [])
    for i, (g, e) in enumerate(zip(got, exp)):
        print(name, i, g)
        assert e is None or g == e, f"{name}: launches of execution {i}"


if __name__ == "__main__":
    if sys.argv[1:2] != ["--record"] or len(sys.argv) > 3:
        sys.exit("usage: python -m tests.test_gpu_expr_paths --record [file]")
    target = sys.argv[2] if len(sys.argv) == 3 else FIXTURE
    if os.path.exists(target):
        sys.exit(f"{target} exists: the recorded dispatch is the reference and is not rewritten")
    rec = {}
    for case_name in CASES:
        rec[case_name] = run_case(case_name)
        if case_name in FIRST_EXECUTION_NOT_PINNED:
            rec[case_name][0] = None
        print(case_name, json.dumps(rec[case_name]), flush=True)
    with open(target, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
