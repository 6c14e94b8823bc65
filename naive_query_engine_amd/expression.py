"""Host mirror of the reference's physical expressions.

Same names and constructor arguments as src/physical_plan/expression/{column,literal,binary,unary}.rs so
plans are written exactly as in the reference's tests (e.g. selection.rs:145-155):

    add_expr = PhysicalBinaryExpr.create(ColumnExpr.try_create("id", None), Operator.Plus,
                                         PhysicalLiteralExpr.create(ScalarValue.Int64(1)))

The host side only *describes* the tree; evaluation happens on the GPU through the C ABI
(nqe_expr_evaluate and the fused operator entry points), which take the flat post-order
encoding produced by `flatten()`.
"""
from __future__ import annotations

import enum
from typing import List, Optional, Sequence

from .arrow_host import (DType, ErrorCode, Field, NqeExprNode, Operator, ScalarValue, Status, UnaryOperator, node_binary, node_column,
                         node_cast, node_conditional, node_literal, node_string, node_string_args, node_string_match, node_unary)


class PhysicalExpr:
    """trait PhysicalExpr (src/physical_plan/expression/mod.rs:25-29)."""

    def flatten(self, fields: Sequence[Field]) -> List[NqeExprNode]:
        raise NotImplementedError

    def referenced_columns(self, fields: Sequence[Field]) -> List[int]:
        return [n.column for n in self.flatten(fields) if n.kind == 0]


class ColumnExpr(PhysicalExpr):
    """src/physical_plan/expression/column.rs:18-58: prefers idx, then the FIRST field whose
    name matches (quirk Q12)."""

    def __init__(self, name: Optional[str], idx: Optional[int]):
        self.name = name
        self.idx = idx

    @staticmethod
    def try_create(name: Optional[str] = None, idx: Optional[int] = None) -> "ColumnExpr":
        if name is None and idx is None:
            raise ErrorCode(Status.LogicalError, "ColumnExpr must has name or idx")
        return ColumnExpr(name, idx)

    def resolve(self, fields: Sequence[Field]) -> int:
        if self.idx is not None:
            if not 0 <= self.idx < len(fields):
                # RecordBatch::column(idx) panics out of range
                raise ErrorCode(Status.NotSupported, f"column index {self.idx} out of range")
            return self.idx
        for i, f in enumerate(fields):
            if f.name == self.name:
                return i
        raise ErrorCode(Status.LogicalError, "ColumnExpr must has name or idx")

    def flatten(self, fields):
        return [node_column(self.resolve(fields))]

    def __repr__(self):
        return f"ColumnExpr(name={self.name!r}, idx={self.idx})"


class PhysicalLiteralExpr(PhysicalExpr):
    """src/physical_plan/expression/literal.rs:17-35."""

    def __init__(self, literal: ScalarValue):
        self.literal = literal

    @staticmethod
    def create(literal: ScalarValue) -> "PhysicalLiteralExpr":
        return PhysicalLiteralExpr(literal)

    def flatten(self, fields):
        return [node_literal(self.literal)]

    def __repr__(self):
        return f"Literal({self.literal})"


class PhysicalBinaryExpr(PhysicalExpr):
    """src/physical_plan/expression/binary.rs:91-156."""

    def __init__(self, left: PhysicalExpr, op: Operator, right: PhysicalExpr):
        self.left, self.op, self.right = left, Operator(op), right

    @staticmethod
    def create(left: PhysicalExpr, op: Operator, right: PhysicalExpr) -> "PhysicalBinaryExpr":
        return PhysicalBinaryExpr(left, op, right)

    def flatten(self, fields):
        return self.left.flatten(fields) + self.right.flatten(fields) + [node_binary(self.op)]

    def __repr__(self):
        return f"({self.left!r} {self.op.name} {self.right!r})"


class PhysicalUnaryExpr(PhysicalExpr):
    """src/physical_plan/expression/unary.rs:46-109.  `name` and `return_type` are stored and, as in the reference's evaluate,
    ignored (the planner passes "todo" and Int32, planner/mod.rs:208-217): the result is Float64 whatever they say."""

    def __init__(self, expr: PhysicalExpr, func: UnaryOperator, name: str = "", return_type=None):
        self.expr, self.func, self.name, self.return_type = expr, UnaryOperator(func), name, return_type

    @staticmethod
    def create(expr: PhysicalExpr, func: UnaryOperator, name: str = "", return_type=None) -> "PhysicalUnaryExpr":
        return PhysicalUnaryExpr(expr, func, name, return_type)

    def flatten(self, fields):
        return self.expr.flatten(fields) + [node_unary(self.func)]

    def __repr__(self):
        return f"{self.func.name}({self.expr!r})"


STRING_FUNCTIONS = (UnaryOperator.Trim, UnaryOperator.LTrim, UnaryOperator.RTrim, UnaryOperator.CharacterLength, UnaryOperator.Lower,
                    UnaryOperator.Upper, UnaryOperator.Reverse)


class PhysicalStringExpr(PhysicalExpr):
    """This package's own node beside the reference's (quirk Q25): one of the string functions of `enum UnaryOperator` that really
    are unary — Trim, LTrim, RTrim, CharacterLength, Lower, Upper, Reverse — with a body, over a Utf8 operand.  PhysicalUnaryExpr over
    the same functions stays what the reference's todo!() is (NotSupported).  Any UnaryOperator is taken here and encoded as it is:
    the library refuses the others, as it refuses everything else about an expression."""

    def __init__(self, expr: PhysicalExpr, func: UnaryOperator):
        self.expr, self.func = expr, UnaryOperator(func)

    @staticmethod
    def create(expr: PhysicalExpr, func: UnaryOperator) -> "PhysicalStringExpr":
        return PhysicalStringExpr(expr, func)

    def flatten(self, fields):
        return self.expr.flatten(fields) + [node_string(self.func)]

    def __repr__(self):
        return f"{self.func.name}({self.expr!r})"


INT64_MAX = (1 << 63) - 1
STRING_ARGS_FUNCTIONS = (UnaryOperator.Repeat, UnaryOperator.Replace, UnaryOperator.Substr)


class PhysicalStringArgsExpr(PhysicalExpr):
    """This package's own node beside the reference's (quirk Q26): the three functions of `enum UnaryOperator` that take arguments —
    Substr(s, start, len), Repeat(s, n), Replace(s, from, to) — with a body, over a Utf8 operand `expr` and the argument expressions
    `args` (Int64-valued for Substr and Repeat, Utf8 literals for Replace).  Any UnaryOperator and any number of arguments are taken
    here and encoded as they are: the library refuses the others, as it refuses everything else about an expression."""

    def __init__(self, func: UnaryOperator, expr: PhysicalExpr, args: Sequence[PhysicalExpr]):
        self.func, self.expr, self.args = UnaryOperator(func), expr, list(args)

    @staticmethod
    def create(func: UnaryOperator, expr: PhysicalExpr, args: Sequence[PhysicalExpr]) -> "PhysicalStringArgsExpr":
        return PhysicalStringArgsExpr(func, expr, args)

    def flatten(self, fields):
        out = self.expr.flatten(fields)  # post-order, children left to right: the string deepest, the last argument on top
        for a in self.args:
            out = out + a.flatten(fields)
        return out + [node_string_args(self.func)]

    def __repr__(self):
        return f"{self.func.name}({', '.join(repr(e) for e in [self.expr] + self.args)})"


class MatchOperator(enum.IntEnum):
    """same order as `enum nqe_match_operator` (include/nqe.h)"""
    Like = 0
    NotLike = 1
    ILike = 2
    NotILike = 3
    StartsWith = 4
    EndsWith = 5
    Contains = 6
    StrPos = 7


class PhysicalStringMatchExpr(PhysicalExpr):
    """This package's own node beside the reference's (quirk Q27: the reference has no pattern match, sql/planner.rs:478 maps LIKE to
    unimplemented!()): `expr` LIKE / NOT LIKE / ILIKE / NOT ILIKE `pattern`, starts_with, ends_with, contains (Boolean) and strpos
    (Int64) over a Utf8 operand and a pattern expression, which the library takes only as a Utf8 literal.  Any pattern expression is
    taken here and encoded as it is: the library refuses the others, as it refuses everything else about an expression."""

    def __init__(self, op: MatchOperator, expr: PhysicalExpr, pattern: PhysicalExpr):
        self.op, self.expr, self.pattern = MatchOperator(op), expr, pattern

    @staticmethod
    def create(op: MatchOperator, expr: PhysicalExpr, pattern: PhysicalExpr) -> "PhysicalStringMatchExpr":
        return PhysicalStringMatchExpr(op, expr, pattern)

    def flatten(self, fields):
        return self.expr.flatten(fields) + self.pattern.flatten(fields) + [node_string_match(self.op)]  # post-order: the string deepest

    def __repr__(self):
        return f"{self.op.name}({self.expr!r}, {self.pattern!r})"


class CondOperator(enum.IntEnum):
    """same order as `enum nqe_cond_operator` (include/nqe.h)"""
    Not = 0
    IsNull = 1
    IsNotNull = 2
    Coalesce = 3
    NullIf = 4
    If = 5


COND_ARITY = {CondOperator.Not: 1, CondOperator.IsNull: 1, CondOperator.IsNotNull: 1, CondOperator.Coalesce: 2, CondOperator.NullIf: 2, CondOperator.If: 3}


class PhysicalConditionalExpr(PhysicalExpr):
    """This package's own node beside the reference's (quirk Q28: the reference's planner leaves IsNull, Not and Case unimplemented!(),
    sql/planner.rs): Not(b), IsNull(x), IsNotNull(x), Coalesce(a, b), NullIf(a, b) and If(c, t, e) — SQL CASE: a NULL condition takes
    the else branch — over operands of any form.  Any number of operands is taken here and encoded as it is, with the node's `column`
    field carrying that number: the library refuses a count that is not the function's arity, as it refuses everything else about an
    expression."""

    def __init__(self, op: CondOperator, operands: Sequence[PhysicalExpr]):
        self.op, self.operands = CondOperator(op), list(operands)

    @staticmethod
    def create(op: CondOperator, operands: Sequence[PhysicalExpr]) -> "PhysicalConditionalExpr":
        return PhysicalConditionalExpr(op, operands)

    def flatten(self, fields):
        out = []  # post-order, operands left to right: the first deepest (If: the condition), the last on top
        for e in self.operands:
            out = out + e.flatten(fields)
        return out + [node_conditional(self.op, len(self.operands))]

    def __repr__(self):
        return f"{self.op.name}({', '.join(repr(e) for e in self.operands)})"


class PhysicalCastExpr(PhysicalExpr):
    """src/physical_plan/expression/cast.rs:16-88, whose evaluate is thirty-odd todo!()s (quirk Q29).  Here it has a body on the device:
    arrow's cast with safe = true over Boolean, Int64, UInt64, Float64 and Utf8 — what a target type cannot represent is NULL (the rules:
    include/nqe.h).  Any `data_type` is taken and encoded as it is (the node's `dtype` field): the library refuses what is no target
    type, and Float64 -> Utf8, as it refuses everything else about an expression."""

    def __init__(self, expr: PhysicalExpr, data_type):
        self.expr, self.data_type = expr, data_type

    @staticmethod
    def create(expr: PhysicalExpr, data_type) -> "PhysicalCastExpr":
        return PhysicalCastExpr(expr, data_type)

    def flatten(self, fields):
        return self.expr.flatten(fields) + [node_cast(self.data_type)]  # post-order: `x CAST`

    def __repr__(self):
        name = DType(self.data_type).name if self.data_type in tuple(DType) else str(int(self.data_type))
        return f"CAST({self.expr!r} AS {name})"


# small conveniences for tests / bench (not part of the reference surface)
def col(i_or_name) -> ColumnExpr:
    return ColumnExpr.try_create(None, i_or_name) if isinstance(i_or_name, int) else ColumnExpr.try_create(i_or_name, None)


def lit_i64(v) -> PhysicalLiteralExpr:
    return PhysicalLiteralExpr.create(ScalarValue.Int64(v))


def lit_u64(v) -> PhysicalLiteralExpr:
    return PhysicalLiteralExpr.create(ScalarValue.UInt64(v))


def lit_f64(v) -> PhysicalLiteralExpr:
    return PhysicalLiteralExpr.create(ScalarValue.Float64(v))


def lit_bool(v) -> PhysicalLiteralExpr:
    return PhysicalLiteralExpr.create(ScalarValue.Boolean(v))


def lit_utf8(v) -> PhysicalLiteralExpr:
    return PhysicalLiteralExpr.create(ScalarValue.Utf8(v))


def binop(l, op, r) -> PhysicalBinaryExpr:
    return PhysicalBinaryExpr.create(l, op, r)


def unop(func, e) -> PhysicalUnaryExpr:
    return PhysicalUnaryExpr.create(e, func, UnaryOperator(func).name.lower(), None)


def strop(func, e) -> PhysicalStringExpr:
    return PhysicalStringExpr.create(e, func)


def _int_arg(v) -> PhysicalExpr:
    return v if isinstance(v, PhysicalExpr) else lit_i64(v)


def _utf8_arg(v) -> PhysicalExpr:
    return v if isinstance(v, PhysicalExpr) else lit_utf8(v)


def substr(e, start, length=None) -> PhysicalStringArgsExpr:
    """substr(e, start, length); length None: to the end (Int64 max — the node has no two-operand form)"""
    return PhysicalStringArgsExpr.create(UnaryOperator.Substr, e, [_int_arg(start), _int_arg(INT64_MAX if length is None else length)])


def repeat(e, n) -> PhysicalStringArgsExpr:
    return PhysicalStringArgsExpr.create(UnaryOperator.Repeat, e, [_int_arg(n)])


def replace(e, frm, to) -> PhysicalStringArgsExpr:
    return PhysicalStringArgsExpr.create(UnaryOperator.Replace, e, [_utf8_arg(frm), _utf8_arg(to)])


def _match(op, e, pattern) -> PhysicalStringMatchExpr:
    return PhysicalStringMatchExpr.create(op, e, _utf8_arg(pattern))  # a str, bytes or None becomes the Utf8 literal; an expression stays


def like(e, pattern) -> PhysicalStringMatchExpr:
    return _match(MatchOperator.Like, e, pattern)


def not_like(e, pattern) -> PhysicalStringMatchExpr:
    return _match(MatchOperator.NotLike, e, pattern)


def ilike(e, pattern) -> PhysicalStringMatchExpr:
    return _match(MatchOperator.ILike, e, pattern)


def not_ilike(e, pattern) -> PhysicalStringMatchExpr:
    return _match(MatchOperator.NotILike, e, pattern)


def starts_with(e, prefix) -> PhysicalStringMatchExpr:
    return _match(MatchOperator.StartsWith, e, prefix)


def ends_with(e, suffix) -> PhysicalStringMatchExpr:
    return _match(MatchOperator.EndsWith, e, suffix)


def contains(e, sub) -> PhysicalStringMatchExpr:
    return _match(MatchOperator.Contains, e, sub)


def strpos(e, sub) -> PhysicalStringMatchExpr:
    return _match(MatchOperator.StrPos, e, sub)


def not_(e) -> PhysicalConditionalExpr:
    return PhysicalConditionalExpr.create(CondOperator.Not, [e])


def is_null(e) -> PhysicalConditionalExpr:
    return PhysicalConditionalExpr.create(CondOperator.IsNull, [e])


def is_not_null(e) -> PhysicalConditionalExpr:
    return PhysicalConditionalExpr.create(CondOperator.IsNotNull, [e])


def coalesce(a, b, *more) -> PhysicalConditionalExpr:
    """coalesce(a, b, c, …) nests to the right: coalesce(a, coalesce(b, c)), in postfix `a b c COALESCE COALESCE`"""
    rest = coalesce(b, *more) if more else b
    return PhysicalConditionalExpr.create(CondOperator.Coalesce, [a, rest])


def nullif(a, b) -> PhysicalConditionalExpr:
    return PhysicalConditionalExpr.create(CondOperator.NullIf, [a, b])


def if_else(c, t, e) -> PhysicalConditionalExpr:
    """t where c is true, e where c is false OR NULL (SQL CASE WHEN c THEN t ELSE e END)"""
    return PhysicalConditionalExpr.create(CondOperator.If, [c, t, e])


def case_when(whens, otherwise) -> PhysicalExpr:
    """CASE WHEN c1 THEN x1 WHEN c2 THEN x2 … ELSE otherwise END: nested Ifs, in postfix `c1 x1 c2 x2 otherwise IF IF`; a CASE without
    ELSE passes lit_null(dtype) of the value type as `otherwise`"""
    out = otherwise
    for c, x in reversed(list(whens)):
        out = if_else(c, x, out)
    return out


def lit_null(dtype) -> PhysicalLiteralExpr:
    """the NULL literal of a type: ScalarValue::X(None)"""
    return PhysicalLiteralExpr.create(ScalarValue(DType(dtype), None))


def cast(e, dtype) -> PhysicalCastExpr:
    """cast(e as dtype): `dtype` a DType (or its number) that names a value type, Boolean .. Utf8"""
    if not isinstance(e, PhysicalExpr):
        raise TypeError(f"cast takes an expression, not {type(e).__name__}")
    try:
        target = DType(dtype)
    except ValueError:
        raise ValueError(f"cast: {dtype!r} is no DType") from None
    if target == DType.NULL:
        raise ValueError("cast: Null is no target type")
    return PhysicalCastExpr.create(e, target)
