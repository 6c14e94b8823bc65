"""The CPU oracle against the independent model of the expression semantics (tests/expr_value_util.py) on the edge-value tables the
device suite uses: Int64 and UInt64 over their whole ranges with the range ends planted, Float64 with NaN, +-inf, +-0, subnormals and
f64::MAX — 4000 rows, plain and nullable.  Every catalogue tree goes through orc.expr_evaluate; the predicates also through
orc.selection and, with a projection behind them, orc.projection.  Compared exactly: bit for bit, signed zeros included.

Three more things are checked here:
  * the fault cases raise the same status on both sides — and do not raise when the fault sits under a NULL slot or in a dropped row;
  * THE INPUTS DISCRIMINATE: for every deliberately wrong variant of the model (WRONG_RULES: a signed compare of UInt64, floored division,
    a fused multiply-add, a lost sign of zero, ...) the trees written for that mistake (WITNESSES) differ from the true model over the
    generated table — a condition on the data, so that a kernel with that mistake cannot pass the device suite;
  * the model itself on hand-written rows.
binary.rs:108-155, selection.rs:58-107"""
import functools
import math

import pytest

from naive_query_engine_amd.arrow_host import ErrorCode
from oracle import oracle as orc
from tests import expr_value_util as ev
from tests.expr_value_util import A, B, BO, F, I, L, O, X, XX, Z
from tests.helpers import fields

N = 4000
FLD = fields(*ev.NAMES)
VARIANTS = [False, True]
VARIANT_IDS = ["plain", "nullable"]
# behind a selection: what the projection list of the predicate cases holds (a value tree, a predicate with a literal that must stay valid)
BEHIND = [ev.VALUE_TREES["contraction_bait"], ev.PRED_TREES["kleene"], ev.VALUE_TREES["int_wrap_chain"]]


@functools.lru_cache(maxsize=4)
def table(nullable, plant=frozenset()):
    """(the model's table, its columns as the oracle takes them); the catalogue's table plants no faulting divisor"""
    t = ev.make_table(N, 20 + int(nullable), nullable, plant=plant)
    return t, [t.columns()]


def nodes(tree):
    return ev.to_expr(tree).flatten(FLD)


@pytest.mark.parametrize("nullable", VARIANTS, ids=VARIANT_IDS)
@pytest.mark.parametrize("name", list(ev.VALUE_TREES) + list(ev.PRED_TREES) + list(ev.CONJ_TREES))
def test_oracle_evaluates_as_the_model(name, nullable):
    tree = dict(ev.VALUE_TREES, **ev.ALL_PREDICATES)[name]
    t, cols = table(nullable)
    ev.assert_column_matches(orc.expr_evaluate(cols, nodes(tree)), ev.model_evaluate(tree, t), f"{name} nullable={nullable}")


@pytest.mark.parametrize("nullable", VARIANTS, ids=VARIANT_IDS)
@pytest.mark.parametrize("column", list(ev.COMPARE_LITERALS))
def test_oracle_evaluates_plain_compares_as_the_model(column, nullable):
    t, cols = table(nullable)
    for name, tree in ev.PLAIN_COMPARES.items():
        if ev.columns_of(tree) == [column]:
            ev.assert_column_matches(orc.expr_evaluate(cols, nodes(tree)), ev.model_evaluate(tree, t), f"{name} nullable={nullable}")


def select_project(cols, pred, trees):
    return orc.projection(orc.selection(cols, nodes(pred), raw=True), [nodes(t) for t in trees])[0]


@pytest.mark.parametrize("nullable", VARIANTS, ids=VARIANT_IDS)
@pytest.mark.parametrize("name", list(ev.PRED_TREES) + list(ev.CONJ_TREES))
def test_oracle_selects_and_projects_as_the_model(name, nullable):
    pred = ev.ALL_PREDICATES[name]
    t, cols = table(nullable)
    ev.assert_columns_match(orc.selection(cols, nodes(pred))[0], ev.model_select(pred, t), f"selection {name} nullable={nullable}")
    ev.assert_columns_match(select_project(cols, pred, BEHIND), ev.model_select_project(pred, BEHIND, t), f"projection behind {name} nullable={nullable}")


@pytest.mark.parametrize("nullable", VARIANTS, ids=VARIANT_IDS)
@pytest.mark.parametrize("column", list(ev.COMPARE_LITERALS))
def test_oracle_selects_by_plain_compares_as_the_model(column, nullable):
    """every third plain compare of the column (the whole set is evaluated above; a selection compacts all eight columns)"""
    t, cols = table(nullable)
    mine = [(name, tree) for name, tree in ev.PLAIN_COMPARES.items() if ev.columns_of(tree) == [column]]
    for name, pred in mine[::3]:
        ev.assert_columns_match(orc.selection(cols, nodes(pred))[0], ev.model_select(pred, t), f"selection {name} nullable={nullable}")


# --------------------------------------------------------------------------- faults
@pytest.mark.parametrize("case", list(ev.FAULT_CASES))
def test_faults_raise_the_same_status(case):
    tree, _, guard = ev.FAULT_CASES[case]
    for nullable in VARIANTS:
        t = ev.fault_table(N, 31, case, nullable)
        cols = [t.columns()]
        assert ev.outcome(ev.model_evaluate, tree, t) == ("raises", ev.FAULT_STATUS), "the table plants the fault in a valid row"
        with pytest.raises(ErrorCode) as err:
            orc.expr_evaluate(cols, nodes(tree))
        assert err.value.status == ev.FAULT_STATUS
        # behind a selection that keeps the faulting rows
        keep_all = X(B, O.NotEq, I(0))
        with pytest.raises(ErrorCode) as err:
            select_project(cols, keep_all, [tree])
        assert err.value.status == ev.FAULT_STATUS
        assert ev.outcome(ev.model_select_project, keep_all, [tree], t) == ("raises", ev.FAULT_STATUS)
        # in the predicate itself
        pred = X(tree, O.Eq, L(ev.kind_of(tree), 1 if ev.kind_of(tree) == "i" else 1.0))
        with pytest.raises(ErrorCode) as err:
            orc.selection(cols, nodes(pred))
        assert err.value.status == ev.FAULT_STATUS


@pytest.mark.parametrize("case", list(ev.FAULT_CASES))
def test_faults_under_null_slots_and_in_dropped_rows_do_not_raise(case):
    tree, _, guard = ev.FAULT_CASES[case]
    t = ev.fault_table(N, 32, case, nullable=True, null_the_faults=True)
    ev.assert_column_matches(orc.expr_evaluate([t.columns()], nodes(tree)), ev.model_evaluate(tree, t), f"{case} under NULL slots")
    for nullable in VARIANTS:
        t = ev.fault_table(N, 33, case, nullable)
        got = select_project([t.columns()], guard, [tree, A])
        ev.assert_columns_match(got, ev.model_select_project(guard, [tree, A], t), f"{case} in dropped rows nullable={nullable}")


# --------------------------------------------------------------------------- the inputs discriminate
def discrimination_cases(t, tn, faulty):
    """(what, model function, arguments) of everything the device suite evaluates: trees, selections, projections behind a selection — the
    latter over the nullable table, whose NULL predicates emit NULL rows — and the fault cases"""
    for name, tree in dict(ev.VALUE_TREES, **ev.ALL_PREDICATES).items():
        yield name, ev.model_evaluate, (tree, t)
    yield "kleene behind a nullable predicate", ev.model_select_project, (X(XX, O.Lt, F(0.0)), BEHIND, tn)
    for case, ft in faulty.items():
        yield case, ev.model_evaluate, (ev.FAULT_CASES[case][0], ft)


# the trees written for each mistake: every one of them must tell the wrong variant from the model on the generated table
WITNESSES = {
    "u64_signed_compare": ["u64_compare_and_wrap", "u_Lt_2p63", "2p63m1_GtEq_u", "pre_u_minus"],
    "floored_division": ["magic_divisors", "shift_divisors", "column_divisors", "pre_a_div"],
    "saturating": ["int_wrap_chain", "i64_wrap_in_predicate", "u64_divisors", "pre_a_times"],
    "fused_multiply_add": ["contraction_bait", "four_columns_mixed"],
    "reciprocal_division": ["true_division", "fmod_column"],
    "negative_zero_is_less": ["x_Lt_p0", "n0_Lt_x", "x_GtEq_p0", "nested_pre"],
    "nan_above_inf": ["x_Gt_pinf", "x_GtEq_nan", "x_GtEq_50", "pre_x_times"],
    "fmod_divisor_sign": ["fmod_literal", "fmod_column"],
    "zero_sign_dropped": ["signed_zero", "fmod_literal"],
    "null_predicate_invalidates_literals": ["kleene behind a nullable predicate"],
    "min_over_minus_one_wraps": ["min_divided_by_minus_one_literal", "min_divided_by_minus_one_column", "min_modulus_minus_one_column"],
}


def test_the_inputs_discriminate_every_wrong_variant():
    t, tn = table(False)[0], table(True)[0]
    faulty = {case: ev.fault_table(N, 31, case) for case in ev.FAULT_CASES}
    cases = {what: (fn, args) for what, fn, args in discrimination_cases(t, tn, faulty)}
    assert sorted(WITNESSES) == sorted(ev.WRONG_RULES)
    for rule, witnesses in WITNESSES.items():
        for what in witnesses:
            fn, args = cases[what]
            assert not ev.outcomes_equal(ev.outcome(fn, *args, rules=frozenset([rule])), ev.outcome(fn, *args)), \
                f"the generated table does not tell the wrong variant `{rule}` from the model through {what}"


# --------------------------------------------------------------------------- the model itself
def test_model_states_the_edges():
    MIN, MAX, ap = ev.I64_MIN, ev.I64_MAX, ev.apply
    # wrapping integers
    assert ap(O.Plus, "i", MAX, 1) == MIN and ap(O.Minus, "i", MIN, 1) == MAX and ap(O.Multiply, "i", MIN, -1) == MIN
    assert ap(O.Minus, "i", 100, MIN) == MIN + 100 and ap(O.Multiply, "i", 1 << 62, 2) == MIN
    assert ap(O.Plus, "u", ev.U64_MAX, 1) == 0 and ap(O.Minus, "u", 0, 1) == ev.U64_MAX and ap(O.Multiply, "u", 1 << 63, 3) == 1 << 63
    # truncated division, the remainder takes the dividend's sign
    assert ap(O.Divide, "i", -7, 2) == -3 and ap(O.Modulos, "i", -7, 2) == -1 and ap(O.Divide, "i", 7, -2) == -3 and ap(O.Modulos, "i", 7, -2) == 1
    assert ap(O.Divide, "i", MIN, MIN) == 1 and ap(O.Modulos, "i", MIN + 1, MIN) == MIN + 1 and ap(O.Divide, "i", MIN, 1) == MIN and ap(O.Modulos, "i", MIN, 1) == 0
    assert ap(O.Divide, "i", MIN, MAX) == -1 and ap(O.Modulos, "i", MIN, MAX) == -1 and ap(O.Divide, "i", MIN, -8) == 1 << 60
    assert ap(O.Divide, "u", ev.U64_MAX, 1 << 63) == 1 and ap(O.Modulos, "u", ev.U64_MAX, (1 << 63) + 5) == (1 << 63) - 6
    # unsigned compares
    assert ap(O.Gt, "u", 1 << 63, (1 << 63) - 1) and not ap(O.Lt, "u", ev.U64_MAX, 0) and ap(O.Lt, "i", -1, 0)
    # one rounding per operation: x * x + x / 4 for x = 1 + 2^-27 is not the fused result
    x = 1.0 + 2.0 ** -27
    assert ap(O.Plus, "f", ap(O.Multiply, "f", x, x), -1.0) == 2.0 ** -26 and ev._fused(O.Plus, x, x, -1.0) == 2.0 ** -26 + 2.0 ** -54
    # signs of zero
    z = ap(O.Multiply, "f", ap(O.Plus, "f", -0.0, -0.0), 0.0)
    assert z == 0.0 and math.copysign(1.0, z) == -1.0
    assert math.copysign(1.0, ap(O.Multiply, "f", ap(O.Plus, "f", 0.0, -0.0), 0.0)) == 1.0
    assert math.copysign(1.0, ap(O.Modulos, "f", -5.0, 2.5)) == -1.0 and ap(O.Modulos, "f", -5.5, 2.5) == -0.5
    # fmod at infinity and NaN
    assert math.isnan(ap(O.Modulos, "f", math.inf, 2.5)) and math.isnan(ap(O.Modulos, "f", 1.0, math.nan)) and ap(O.Modulos, "f", -3.0, math.inf) == -3.0
    # the reciprocal shortcut's limits are exact; outside them the division overflows or underflows on its own
    assert ap(O.Divide, "f", 5e-324, 2.0 ** -1021) == 5e-324 * 2.0 ** 1021 and ap(O.Divide, "f", 1.0, 5e-324) == math.inf and ap(O.Divide, "f", 3.0, 2.0 ** 1023) == 3.0 * 2.0 ** -1023
    # IEEE compares
    nan = math.nan
    assert not any(ap(op, "f", nan, nan) for op in (O.Eq, O.Lt, O.LtEq, O.Gt, O.GtEq)) and ap(O.NotEq, "f", nan, nan) and ap(O.NotEq, "f", nan, 1.0)
    assert ap(O.Eq, "f", -0.0, 0.0) and not ap(O.Lt, "f", -0.0, 0.0) and ap(O.GtEq, "f", -0.0, 0.0) and not ap(O.Gt, "f", nan, math.inf)
    # faults
    for op in (O.Divide, O.Modulos):
        for kind, p, q in (("i", 5, 0), ("u", 5, 0), ("f", 5.0, 0.0), ("f", 5.0, -0.0), ("f", nan, 0.0), ("i", MIN, -1)):
            with pytest.raises(ev.Fault):
                ap(op, kind, p, q)
    assert ap(O.Divide, "i", MIN + 1, -1) == MAX and ap(O.Modulos, "i", MAX, -1) == 0

    # a table of eight rows: Kleene, NULL operands, faults under NULL slots, a selection with a NULL predicate (quirk Q4)
    import numpy as np
    n = 8
    m = lambda *bits_: np.array(bits_, dtype=bool)
    cols = {name: (np.zeros(n, dtype=ev.NP_DTYPES[ev.KINDS[name]]), None) for name in ev.NAMES}
    cols["bo"] = (m(1, 1, 1, 0, 0, 0, 1, 0), m(1, 1, 1, 1, 1, 1, 0, 0))
    cols["x"] = (np.array([-1.0, 1.0, 0.0, -1.0, 1.0, 0.0, -1.0, 1.0]), m(1, 1, 0, 1, 1, 0, 1, 1))
    cols["a"] = (np.array([MIN, 5, 5, 5, MIN, 5, 5, 5], dtype=np.int64), m(1, 1, 1, 1, 0, 1, 1, 1))
    cols["z"] = (np.array([2, 0, 0, 3, -1, 1, 1, 1], dtype=np.int64), m(1, 0, 0, 1, 1, 1, 1, 1))
    t = ev.Table(n, cols)
    r = ev.model_evaluate(X(BO, O.And, X(XX, O.Lt, F(0.0))), t)          # bo and x < 0
    assert r.valid == [True, True, False, True, True, True, False, True] and [v for v in r.vals if v is not None] == [True, False, False, False, False, False]
    r = ev.model_evaluate(ev.PRED_TREES["kleene"], t)                     # ... or true
    assert r.valid == [True] * n and r.vals == [True] * n
    r = ev.model_evaluate(X(X(BO, O.Or, L("b", None)), O.And, L("b", True)), t)   # (bo or NULL) and true: true where bo is true, else NULL
    assert r.valid == [True, True, True, False, False, False, False, False]
    r = ev.model_evaluate(X(A, O.Divide, Z), t)                          # zero divisors and MIN / -1 only under NULL slots: no fault
    assert r.valid == [True, False, False, True, False, True, True, True] and r.vals[0] == MIN // 2 and r.vals[3] == 1
    cols["z"] = (cols["z"][0], m(1, 1, 0, 1, 1, 1, 1, 1))
    assert ev.outcome(ev.model_evaluate, X(A, O.Divide, Z), ev.Table(n, cols)) == ("raises", ev.FAULT_STATUS)
    t2 = ev.Table(n, cols)
    # dropped rows never fault: z != 0 drops row 1 (row 2, a NULL predicate, is emitted as a NULL row: its zero divisor is not valid)
    out = ev.model_select_project(X(Z, O.NotEq, I(0)), [X(I(10), O.Divide, Z), X(L("b", None), O.Or, L("b", True)), A], t2)
    assert len(out[0].vals) == 7 and out[0].valid == [True, False, True, True, True, True, True] and out[0].vals[0] == 5 and out[0].vals[3] == -10
    assert out[1].valid == [True] * 7 and out[1].vals == [True] * 7      # literals stay valid in the NULL row
    assert out[2].valid == [True, False, True, False, True, True, True]  # every column is NULL there
    wrong = ev.model_select_project(X(Z, O.NotEq, I(0)), [X(L("b", None), O.Or, L("b", True))], t2, rules=frozenset(["null_predicate_invalidates_literals"]))
    assert wrong[0].valid == [True, False, True, True, True, True, True]
