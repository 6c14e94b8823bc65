"""The numpy model of tests/conditional_util.py (quirk Q28) against pyarrow.compute over random nullable arrays of all five dtypes:
case_when for IF (a NULL condition takes the else branch — not if_else, which propagates it), coalesce, is_null, is_valid, invert, and
NULLIF against case_when(equal(a, b), null, a); the Float64 NaN and +-0.0 rows by hand against the rule of binary_kernel's NQE_OP_EQ
(IEEE: NaN equals nothing, -0.0 equals +0.0).  pyarrow decides the values where valid and the validity; zeros under NULL and the presence
of a validity buffer are the model's own statements of include/nqe.h and are checked against that text's rules here."""
import numpy as np
import pyarrow as pa
import pyarrow.compute as pc
import pytest

from tests import conditional_util as cu
from tests.conditional_util import COALESCE, IF, IS_NOT_NULL, IS_NULL, KINDS, NOT, NULLIF, Val

PA = {"i64": pa.int64(), "u64": pa.uint64(), "f64": pa.float64(), "bool": pa.bool_(), "utf8": pa.binary()}
N = 4000


def to_arrow(v):
    vals = list(v.values) if v.kind == "utf8" else np.asarray(v.values).tolist()
    return pa.array([x if ok else None for x, ok in zip(vals, v.valid)], type=PA[v.kind])


def assert_same(model, arrow, what):
    """the model's rows where valid and its validity are pyarrow's; under a NULL the model holds the zero of the kind"""
    assert len(model) == len(arrow), what
    got_valid = np.array([x is not None for x in arrow.to_pylist()], dtype=bool) if len(arrow) else np.zeros(0, dtype=bool)
    assert (model.valid == got_valid).all(), (what, "validity")
    rows = arrow.to_pylist()
    for i in range(len(model)):
        m = model.values[i]
        if not model.valid[i]:
            assert m == cu.zero_of(model.kind), (what, i, "zero under NULL")
        elif model.kind == "f64" and rows[i] != rows[i]:
            assert m != m, (what, i)
        else:
            assert m == rows[i], (what, i, m, rows[i])
            if model.kind == "f64":
                assert np.signbit(m) == np.signbit(rows[i]), (what, i, "sign of zero")


def column(kind, seed, nullable=True, frac=0.3):
    return cu.make(kind, cu.values_of(kind, N, seed), cu.mask_of(N, seed, frac) if nullable else None)


@pytest.mark.parametrize("kind", KINDS)
def test_coalesce_if_and_nullif_against_pyarrow(kind):
    a, b = column(kind, 1), column(kind, 2)
    plain = column(kind, 3, nullable=False)
    c = column("bool", 4)
    A, B, P, C = to_arrow(a), to_arrow(b), to_arrow(plain), to_arrow(c)
    null = pa.nulls(N, type=PA[kind])
    assert_same(cu.coalesce(a, b), pc.coalesce(A, B), "coalesce")
    assert_same(cu.coalesce(a, plain), pc.coalesce(A, P), "coalesce(a, plain)")
    assert_same(cu.coalesce(cu.literal(kind, None, N), b), pc.coalesce(null, B), "coalesce(NULL, b)")
    # IF is case_when: a NULL condition takes the else branch
    want = pc.case_when(pa.StructArray.from_arrays([C], names=["c"]), A, B)
    assert_same(cu.if_else(c, a, b), want, "if")
    propagated = pc.if_else(C, A, B)
    assert propagated.null_count > want.null_count  # if_else would make the NULL conditions NULL: not this function
    assert_same(cu.if_else(c, a, cu.literal(kind, None, N)), pc.case_when(pa.StructArray.from_arrays([C], names=["c"]), A, null), "case without else")
    # NULLIF against case_when(equal(a, b), null, a)
    eq = pc.equal(A, B)
    assert pc.sum(pc.fill_null(eq, False)).as_py() > 0 and eq.null_count > 0  # equal pairs and NULL compares both occur
    assert_same(cu.nullif(a, b), pc.case_when(pa.StructArray.from_arrays([eq], names=["c"]), null, A), "nullif")
    # the static presence of a validity buffer, and the null_count the C ABI reports with it
    assert cu.coalesce(a, b).nullable and not cu.coalesce(a, plain).nullable and not cu.coalesce(plain, a).nullable
    assert cu.if_else(c, a, plain).nullable and cu.if_else(c, plain, a).nullable and not cu.if_else(c, plain, plain).nullable
    assert cu.nullif(plain, plain).nullable and cu.null_count_of(cu.nullif(plain, plain)) == -1 and cu.null_count_of(cu.coalesce(a, plain)) == 0
    assert not cu.coalesce(a, plain).valid.__invert__().any()


@pytest.mark.parametrize("kind", KINDS)
def test_is_null_and_is_valid_against_pyarrow(kind):
    a = column(kind, 5)
    A = to_arrow(a)
    for model, arrow in [(cu.is_null(a), pc.is_null(A)), (cu.is_not_null(a), pc.is_valid(A))]:
        assert_same(model, arrow, "is_null / is_valid")
        assert not model.nullable and model.valid.all() and model.values.any() and not model.values.all()
    lit = cu.literal(kind, None, 7)
    assert cu.is_null(lit).values.all() and not cu.is_not_null(lit).values.any()
    assert (cu.is_null(a).values == cu.not_(cu.is_not_null(a)).values).all()


def test_not_against_pyarrow():
    b, plain = column("bool", 6), column("bool", 7, nullable=False)
    assert_same(cu.not_(b), pc.invert(to_arrow(b)), "not")
    assert_same(cu.not_(plain), pc.invert(to_arrow(plain)), "not, no NULLs")
    assert cu.not_(b).nullable and not cu.not_(plain).nullable
    assert not (cu.not_(b).values & ~b.valid).any()  # the value bit under a NULL is 0
    back = cu.not_(cu.not_(b))
    assert (back.values[b.valid] == b.values[b.valid]).all() and (back.valid == b.valid).all()


def test_float64_nullif_by_hand_against_the_rule_of_op_eq():
    """binary_kernel's NQE_OP_EQ on Float64 is C's `x == y` (device_utils.hpp: apply_binary): NaN equals nothing, -0.0 equals +0.0"""
    nan, inf = float("nan"), float("inf")
    a = cu.make("f64", [nan, nan, -0.0, 0.0, 0.0, inf, inf, -inf, 1.5, 1.5, 2.0])
    b = cu.make("f64", [nan, 1.0, 0.0, -0.0, 0.0, inf, -inf, -inf, 1.5, 2.5, nan])
    r = cu.nullif(a, b)
    assert r.valid.tolist() == [True, True, False, False, False, False, True, False, False, True, True]
    assert np.isnan(r.values[0]) and np.isnan(r.values[1]) and r.values[6] == inf and r.values[9] == 1.5 and r.values[10] == 2.0
    assert (r.values[~r.valid] == 0.0).all() and not np.signbit(r.values[2])  # +0.0 under the NULL that -0.0 = +0.0 makes
    # a NULL a or b: the compare is NULL, the row is a
    a2, b2 = cu.make("f64", [1.0, 1.0, 1.0], [True, False, True]), cu.make("f64", [1.0, 1.0, 1.0], [True, True, False])
    r2 = cu.nullif(a2, b2)
    assert r2.valid.tolist() == [False, False, True] and r2.values.tolist() == [0.0, 0.0, 1.0]
    # integers compare their bits
    big = cu.make("i64", [np.iinfo(np.int64).min, np.iinfo(np.int64).max, 0])
    assert cu.nullif(big, cu.make("i64", [np.iinfo(np.int64).min, 0, 0])).valid.tolist() == [False, True, False]
    u = cu.make("u64", [(1 << 63) + 5, (1 << 64) - 1])
    assert cu.nullif(u, cu.make("u64", [(1 << 63) + 5, (1 << 63) - 1])).valid.tolist() == [False, True]


def test_identities_of_the_model():
    for kind in KINDS:
        a, b = column(kind, 8), column(kind, 9)
        eq = Val("bool", a.valid & b.valid & cu.equal_rows(kind, a.values, b.values), a.valid & b.valid, True)
        via_if, direct = cu.if_else(eq, cu.literal(kind, None, N), a), cu.nullif(a, b)
        assert (via_if.valid == direct.valid).all() and list(via_if.values) == list(direct.values)
        via_if, direct = cu.if_else(cu.is_not_null(a), a, b), cu.coalesce(a, b)
        assert (via_if.valid == direct.valid).all() and list(via_if.values) == list(direct.values)
    assert cu.ARITY == {NOT: 1, IS_NULL: 1, IS_NOT_NULL: 1, COALESCE: 2, NULLIF: 2, IF: 3}
    assert len(cu.apply(IF, column("bool", 1), column("i64", 2), column("i64", 3))) == N
