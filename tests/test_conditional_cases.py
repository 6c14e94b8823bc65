"""CPU: the case lists of tests/test_gpu_conditional.py (tests/conditional_util.py: row_count_cases, grid_cases) cannot be passed with a
constant answer — the guards are conditions on the INPUTS, so they are decided here, without a device: both values of every Boolean
result occur, both sources of every select occur, some row is NULL wherever the form carries a validity buffer, and no expected output
that a data operand reaches is constant."""
import pytest

from tests import conditional_util as cu


@pytest.mark.parametrize("kind", cu.KINDS)
def test_row_count_cases_are_guarded(kind):
    seen = set()
    for n in cu.ROW_COUNTS:
        for op, args, expected in cu.row_count_cases(kind, n):
            assert len(expected) == n
            cu.guard(op, args, expected)
            seen.add((op, tuple(a.form for a in args)))
    ops = {op for op, _ in seen}
    assert ops == ({cu.NOT} if kind == "bool" else set()) | {cu.IS_NULL, cu.IS_NOT_NULL, cu.COALESCE, cu.NULLIF, cu.IF}
    for form in cu.FORMS:  # every operand form in every position of every function
        for op in ops:
            for pos in range(cu.ARITY[op]):
                assert any(o == op and f[pos] == form for o, f in seen), (op, pos, form)


@pytest.mark.parametrize("kind", cu.KINDS)
@pytest.mark.parametrize("op", [cu.COALESCE, cu.NULLIF, cu.IF])
def test_grid_cases_are_guarded(kind, op):
    cases = cu.grid_cases(kind, op)
    assert len(cases) == len(cu.FORMS) ** cu.ARITY[op]
    for case in cases:
        cu.guard(*case)


def test_the_guard_refuses_constant_cases():
    n = 128
    a = cu.Arg("i64", "nullable", cu.make("i64", [1] * n, [True] * n))  # "nullable" without a NULL: COALESCE has one source
    b = cu.Arg("i64", "plain", cu.make("i64", list(range(n))))
    with pytest.raises(AssertionError):
        cu.guard(cu.COALESCE, [a, b], cu.coalesce(a.val, b.val))
    c = cu.Arg("bool", "plain", cu.make("bool", [True] * n))
    with pytest.raises(AssertionError):
        cu.guard(cu.IF, [c, b, b], cu.if_else(c.val, b.val, b.val))
    with pytest.raises(AssertionError):
        cu.guard(cu.NOT, [c], cu.not_(c.val))
    with pytest.raises(AssertionError):
        cu.guard(cu.NULLIF, [b, a], cu.Val("i64", b.val.values, b.val.valid, True))  # (an expected output without an equal pair)
