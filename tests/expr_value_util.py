"""An independent model of the expression semantics (`+ - * / %`, the six compares, Kleene and / or; a selection in front), the edge-value
tables the expression value-domain suites share, the catalogue of named trees, and a comparator of a result column against the model.
Plain Python and numpy; nothing here calls the oracle or the library's evaluation.

The model (a second reading of binary.rs:108-155 and arrow's arithmetic / comparison / kleene kernels), one row at a time:
  Int64 / UInt64   + - * are Python integers reduced mod 2^64 (Int64: reinterpreted as signed); / and % truncate toward zero, the remainder
                   takes the dividend's sign; UInt64 compares are unsigned
  Float64          + - * / are ONE np.float64 operation each (rounded once, nothing fused); % is math.fmod: NaN for an infinite dividend
                   or a NaN operand, the dividend for an infinite divisor
  compares         IEEE: NaN is unequal to everything and false for the four orderings, -0.0 == 0.0
  and / or         Kleene over (value, valid); every other node is valid only if both operands are; a non-NULL literal is always valid
  faults           only from a row whose operands are BOTH valid: integer divisor 0 and Float64 divisor +-0.0 -> "Divide by zero",
                   i64::MIN / -1 and i64::MIN % -1 -> overflow; both ArrowError
  selection        a row is emitted when the predicate is true or NULL; a row emitted for a NULL predicate has every column NULL while
                   literals stay valid (quirk Q4); rows the predicate drops never fault

A tree is a tuple: ("col", name) | ("lit", kind, value or None) | (Operator, left, right); kind is "i" Int64, "u" UInt64, "f" Float64,
"b" Boolean.  to_expr turns one into the library's binop / col / lit_* expression over the columns in the order of NAMES.

`rules` names deliberately WRONG variants of the model (WRONG_RULES): the CPU suite asserts that the generated tables tell every one
of them from the true model, i.e. that a kernel with that mistake could not pass.

The comparator (assert_column_matches): dtype, length and validity exactly; Int64 / UInt64 / Boolean equal; Float64 bit for bit INCLUDING
the sign of zero; any NaN equals any NaN (payload and sign of a produced NaN differ legitimately between x86 and the GPU); values under
NULL slots are not compared.  No tolerance anywhere."""
import fractions
import functools
import math
import struct

import numpy as np

from naive_query_engine_amd import Column, DType, Operator
from naive_query_engine_amd.arrow_host import ScalarValue, Status
from naive_query_engine_amd.expression import PhysicalLiteralExpr, binop, col, lit_bool, lit_f64, lit_i64, lit_u64

O = Operator
M64 = 1 << 64
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
U64_MAX = M64 - 1
F64_MAX = 1.7976931348623157e308
INF, NAN = math.inf, math.nan
NULL_FRAC = 0.10
NAMES = ["a", "b", "u", "x", "y", "z", "zf", "bo", "id"]
KINDS = dict(a="i", b="i", u="u", x="f", y="f", z="i", zf="f", bo="b", id="i")
DTYPES = {"i": DType.INT64, "u": DType.UINT64, "f": DType.FLOAT64, "b": DType.BOOLEAN}
NP_DTYPES = {"i": np.int64, "u": np.uint64, "f": np.float64, "b": np.bool_}
COMPARES = (O.Eq, O.NotEq, O.Lt, O.LtEq, O.Gt, O.GtEq)
ARITH = (O.Plus, O.Minus, O.Multiply, O.Divide, O.Modulos)
FAULT_STATUS = Status.ArrowError
WRONG_RULES = ["u64_signed_compare", "floored_division", "saturating", "fused_multiply_add", "reciprocal_division", "negative_zero_is_less",
               "nan_above_inf", "fmod_divisor_sign", "zero_sign_dropped", "null_predicate_invalidates_literals", "min_over_minus_one_wraps"]


class Fault(Exception):
    """what a valid row raises; .status is the library's status for it"""
    status = FAULT_STATUS


# --------------------------------------------------------------------------- trees
def C(name):
    return ("col", name)


def L(kind, value):
    return ("lit", kind, value)


def X(left, op, right):
    return (op, left, right)


def I(v):
    return L("i", v)


def U(v):
    return L("u", v)


def F(v):
    return L("f", v)


def AND(*ts):
    out = ts[0]
    for t in ts[1:]:
        out = X(out, O.And, t)
    return out


def OR(*ts):
    out = ts[0]
    for t in ts[1:]:
        out = X(out, O.Or, t)
    return out


def to_expr(tree):
    """the library's expression of a tree (columns by their index in NAMES)"""
    if tree[0] == "col":
        return col(NAMES.index(tree[1]))
    if tree[0] == "lit":
        kind, v = tree[1], tree[2]
        if v is None:
            return PhysicalLiteralExpr.create({"i": ScalarValue.Int64, "u": ScalarValue.UInt64, "f": ScalarValue.Float64, "b": ScalarValue.Boolean}[kind](None))
        return {"i": lit_i64, "u": lit_u64, "f": lit_f64, "b": lit_bool}[kind](v)
    return binop(to_expr(tree[1]), tree[0], to_expr(tree[2]))


def columns_of(tree):
    """the distinct columns of a tree, in the order met"""
    if tree[0] == "col":
        return [tree[1]]
    if tree[0] == "lit":
        return []
    out = columns_of(tree[1])
    return out + [c for c in columns_of(tree[2]) if c not in out]


def steps_of(tree):
    """operator nodes: the steps of the tree's program"""
    return 0 if tree[0] in ("col", "lit") else 1 + steps_of(tree[1]) + steps_of(tree[2])


def kind_of(tree):
    if tree[0] == "col":
        return KINDS[tree[1]]
    if tree[0] == "lit":
        return tree[1]
    return "b" if tree[0] in COMPARES or tree[0] in (O.And, O.Or) else kind_of(tree[1])


# --------------------------------------------------------------------------- the model: one operation on one row
def bits(v):
    return struct.unpack("<Q", struct.pack("<d", v))[0]


def _wrap(kind, v):
    v %= M64
    return v - M64 if kind == "i" and v >= 1 << 63 else v


def _trunc_div(p, q):
    d = abs(p) // abs(q)
    return -d if (p < 0) != (q < 0) else d


def _is_pow2(q):
    m, _ = math.frexp(abs(q))
    return m == 0.5


def apply(op, kind, p, q, rules=frozenset()):
    """`p op q` of two VALID operands of `kind`; raises Fault"""
    if op in COMPARES:
        if kind == "u" and "u64_signed_compare" in rules:
            p, q = _wrap("i", p), _wrap("i", q)
        if kind == "f":
            if "nan_above_inf" in rules and (p != p or q != q):      # a total order with NaN as the largest value
                kp, kq = (2, 0.0) if p != p else (1, p), (2, 0.0) if q != q else (1, q)
                return {O.Eq: kp == kq, O.NotEq: kp != kq, O.Lt: kp < kq, O.LtEq: kp <= kq, O.Gt: kp > kq, O.GtEq: kp >= kq}[op]
            if "negative_zero_is_less" in rules and p == 0.0 and q == 0.0:
                p, q = math.copysign(1.0, p), math.copysign(1.0, q)
        return p == q if op == O.Eq else p != q if op == O.NotEq else p < q if op == O.Lt else p <= q if op == O.LtEq else p > q if op == O.Gt else p >= q
    if kind == "f":
        a, b = np.float64(p), np.float64(q)
        with np.errstate(all="ignore"):
            if op == O.Plus:
                r = float(a + b)
            elif op == O.Minus:
                r = float(a - b)
            elif op == O.Multiply:
                r = float(a * b)
            else:
                if q == 0.0:
                    raise Fault("Divide by zero")
                if op == O.Divide:
                    if "reciprocal_division" in rules and q == q and not math.isinf(q) and not _is_pow2(q):
                        r = float(a * (np.float64(1.0) / b))
                    else:
                        r = float(a / b)
                elif math.isinf(p) or p != p or q != q:
                    r = NAN
                else:
                    r = math.fmod(p, q)
                    if "fmod_divisor_sign" in rules and r == r:
                        r = math.copysign(r, q)
        if "zero_sign_dropped" in rules and r == 0.0:
            r = 0.0
        return r
    if op in (O.Plus, O.Minus, O.Multiply):
        v = p + q if op == O.Plus else p - q if op == O.Minus else p * q
        if "saturating" in rules and op != O.Minus:
            lo, hi = (I64_MIN, I64_MAX) if kind == "i" else (0, U64_MAX)
            return min(max(v, lo), hi)
        return _wrap(kind, v)
    if q == 0:
        raise Fault("Divide by zero")
    if kind == "i" and p == I64_MIN and q == -1:
        if "min_over_minus_one_wraps" in rules:
            return I64_MIN if op == O.Divide else 0
        raise Fault("Overflow happened on: i64::MIN / -1")
    if "floored_division" in rules:
        return p // q if op == O.Divide else p % q
    d = _trunc_div(p, q)
    return d if op == O.Divide else p - d * q


def _fused(op, m1, m2, c):
    """m1 * m2 +- c rounded ONCE (the wrong variant `fused_multiply_add`); None where the operands are not all finite or the result is zero"""
    if not (math.isfinite(m1) and math.isfinite(m2) and math.isfinite(c)):
        return None
    e = fractions.Fraction(m1) * fractions.Fraction(m2)
    e = e + fractions.Fraction(c) if op == O.Plus else e - fractions.Fraction(c)
    if e == 0:
        return None
    try:
        return float(e)
    except OverflowError:
        return INF if e > 0 else -INF


# --------------------------------------------------------------------------- tables
SPECIALS = [NAN, INF, -INF, 0.0, -0.0, 5e-324, -5e-324, 2.2250738585072014e-308, -2.2250738585072014e-308, 1e300, -1e300, F64_MAX, -F64_MAX,
            1.0, -1.0, 0.1, 2.5, -2.5, 50.0, 49.99999999999999]
PLANT = {
    "a": [I64_MIN, I64_MIN + 1, I64_MAX, I64_MAX - 1, -1, 0, 1, (1 << 53) + 1, -((1 << 53) + 1), 1 << 62, -(1 << 62), 1 << 32],
    "b": [I64_MIN, I64_MAX, 2, -2, 7, -7],
    "u": [0, 1, (1 << 63) - 1, 1 << 63, (1 << 63) + 1, U64_MAX],
}
ALL_FAULTS = frozenset(["z0", "zm1", "zf+0", "zf-0"])


class Table:
    """columns by name: .np[name] = (values, validity mask or None); .rows(name) = (python values, python validity)"""

    def __init__(self, n, cols):
        self.n, self.np = n, cols
        self._py = {}

    def rows(self, name):
        if name not in self._py:
            v, m = self.np[name]
            self._py[name] = (v.tolist(), [True] * self.n if m is None else m.tolist())
        return self._py[name]

    def nullable(self, name):
        return self.np[name][1] is not None

    def columns(self):
        """the library's columns, in the order of NAMES"""
        return [Column.from_numpy(*self.np[name]) for name in NAMES]


def make_table(n, seed, nullable, plant=ALL_FAULTS, null_the_faults=False):
    """The edge-value table.  Every column is plain, or (nullable) carries 10 % NULLs — but id, a permutation of 0 .. n-1 that is always
    plain (the aggregates' key column); the planted values sit at random rows — one of them the last row — and stay valid.  `plant`: which divisors that fault are planted in z / zf ("z0": zeros in z; "zm1": -1 in z exactly
    where a is i64::MIN; "zf+0" / "zf-0": the two zeros in zf); null_the_faults (nullable only): those rows are NULL in z / zf, and the
    i64::MIN rows are NULL in a — every fault then sits under a NULL slot."""
    rng = np.random.default_rng(seed)
    assert n >= 4 * len(SPECIALS)
    mask = lambda: (rng.random(n) >= NULL_FRAC) if nullable else None

    def planted(v, m, values, last=True):
        at = rng.choice(n - 1, len(values), replace=False)
        if last:
            at[0] = n - 1
        v[at] = values
        if m is not None:
            m[at] = True
        return at

    cols = {}
    a = rng.integers(I64_MIN, I64_MAX, n, dtype=np.int64, endpoint=True)
    am = mask()
    planted(a, am, np.array(PLANT["a"], dtype=np.int64))
    b = rng.integers(I64_MIN, I64_MAX, n, dtype=np.int64, endpoint=True)
    b[(b == 0) | (b == -1)] = 3
    bm = mask()
    planted(b, bm, np.array(PLANT["b"], dtype=np.int64))
    u = rng.integers(0, U64_MAX, n, dtype=np.uint64, endpoint=True)
    um = mask()
    planted(u, um, np.array(PLANT["u"], dtype=np.uint64))

    def floats(no_zero):
        v = rng.random(n) * 200.0 - 100.0
        sp = np.array([s for s in SPECIALS if not (no_zero and s == 0.0)])
        where = rng.random(n) < 0.2
        v[where] = sp[rng.integers(0, len(sp), int(where.sum()))]
        m = mask()
        planted(v, m, sp)
        return v, m

    x, xm = floats(False)
    y, ym = floats(True)
    z = rng.integers(2, 10, n).astype(np.int64) * rng.choice(np.array([-1, 1], dtype=np.int64), n)
    zm = mask()
    zf = (rng.integers(1, 40, n).astype(np.float64) / 4.0) * rng.choice(np.array([-1.0, 1.0]), n)
    zfm = mask()
    min_rows = np.nonzero(a == I64_MIN)[0]
    if "zm1" in plant:
        z[min_rows] = -1
        if zm is not None:
            zm[min_rows] = not null_the_faults
    if "z0" in plant:
        at = planted(z, zm, np.zeros(3, dtype=np.int64))
        if null_the_faults:
            zm[at] = False
    for tag, zero in (("zf+0", 0.0), ("zf-0", -0.0)):
        if tag in plant:
            at = planted(zf, zfm, np.full(3, zero))
            if null_the_faults:
                zfm[at] = False
    if null_the_faults:
        am[min_rows] = False
    bo = rng.random(n) < 0.5
    cols.update(a=(a, am), b=(b, bm), u=(u, um), x=(x, xm), y=(y, ym), z=(z, zm), zf=(zf, zfm), bo=(bo, mask()), id=(rng.permutation(n).astype(np.int64), None))
    return Table(n, cols)


# --------------------------------------------------------------------------- the model: a tree over a table
class Result:
    """one evaluated column: kind, per-row values (None under NULL), validity, and the fault each row raises (None: none)"""

    def __init__(self, kind, vals, valid, fault):
        self.kind, self.vals, self.valid, self.fault = kind, vals, valid, fault


def eval_tree(tree, table, rules=frozenset(), col_valid=None, lit_valid=None):
    """The tree on every row.  col_valid: a per-row validity laid over EVERY column (the rows a NULL predicate emits); lit_valid: the
    literals' validity per row (always valid — except under the wrong variant that invalidates them with the row)."""
    n = table.n
    if tree[0] == "col":
        vals, valid = table.rows(tree[1])
        if col_valid is not None:
            valid = [v and c for v, c in zip(valid, col_valid)]
        return Result(KINDS[tree[1]], vals, valid, [None] * n)
    if tree[0] == "lit":
        ok = tree[2] is not None
        valid = [ok] * n if (lit_valid is None or not ok) else list(lit_valid)
        return Result(tree[1], [tree[2]] * n, valid, [None] * n)
    op = tree[0]
    l, r = eval_tree(tree[1], table, rules, col_valid, lit_valid), eval_tree(tree[2], table, rules, col_valid, lit_valid)
    assert l.kind == r.kind, (tree, l.kind, r.kind)
    fault = [a or b for a, b in zip(l.fault, r.fault)]
    vals, valid = [None] * n, [False] * n
    if op in (O.And, O.Or):
        for i in range(n):
            av, bv = l.valid[i], r.valid[i]
            lb, rb = bool(av and l.vals[i]), bool(bv and r.vals[i])
            if op == O.And:
                ok = (av and bv) or (av and not lb) or (bv and not rb)
                res = lb and rb
            else:
                ok = (av and bv) or lb or rb
                res = lb or rb
            valid[i] = bool(ok)
            vals[i] = bool(res) if ok else None
        return Result("b", vals, valid, fault)
    fused = None
    if "fused_multiply_add" in rules and l.kind == "f" and op in (O.Plus, O.Minus) and tree[1][0] == O.Multiply:
        m1, m2 = eval_tree(tree[1][1], table, rules, col_valid, lit_valid), eval_tree(tree[1][2], table, rules, col_valid, lit_valid)
        fused = (m1.vals, m2.vals)
    kind = l.kind
    for i in range(n):
        if not (l.valid[i] and r.valid[i]):
            continue
        try:
            v = apply(op, kind, l.vals[i], r.vals[i], rules)
            if fused is not None:
                f = _fused(op, fused[0][i], fused[1][i], r.vals[i])
                v = v if f is None else f
        except Fault as e:
            fault[i] = fault[i] or str(e)
            continue
        vals[i], valid[i] = v, True
    # (a row that faults raises for the whole batch: its slot is never looked at)
    return Result("b" if op in COMPARES else kind, vals, valid, fault)


def _raise_first(faults, rows=None):
    for i in (range(len(faults)) if rows is None else rows):
        if faults[i]:
            raise Fault(faults[i])


def model_evaluate(tree, table, rules=frozenset()):
    """expr_evaluate: the column, or raises Fault"""
    r = eval_tree(tree, table, rules)
    _raise_first(r.fault)
    return r


@functools.lru_cache(maxsize=16)
def model_keep(pred, table, rules=frozenset()):
    """(rows emitted, predicate valid there): true or NULL; a fault of ANY row raises (the predicate is evaluated on the whole batch)"""
    p = model_evaluate(pred, table, rules)
    rows = [i for i in range(table.n) if not p.valid[i] or p.vals[i]]
    return rows, [p.valid[i] for i in rows]


def _take(r, rows):
    return Result(r.kind, [r.vals[i] for i in rows], [r.valid[i] for i in rows], [r.fault[i] for i in rows])


def model_select_project(pred, trees, table, rules=frozenset()):
    """the projection list over the rows the selection emits: a NULL-predicate row has every column NULL, literals stay valid; rows the
    predicate drops never fault"""
    rows, pvalid = model_keep(pred, table, rules)
    col_valid = [True] * table.n
    for i, ok in zip(rows, pvalid):
        col_valid[i] = ok
    lit_valid = col_valid if "null_predicate_invalidates_literals" in rules else None
    out = []
    for t in trees:
        r = _take(eval_tree(t, table, rules, col_valid, lit_valid), rows)
        _raise_first(r.fault)
        out.append(r)
    return out


def model_select(pred, table, rules=frozenset()):
    """the selection alone: every column of NAMES over the emitted rows"""
    return model_select_project(pred, [C(name) for name in NAMES], table, rules)


def outcome(fn, *args, **kw):
    """("ok", results) or ("raises", status) of a model function"""
    try:
        r = fn(*args, **kw)
    except Fault as e:
        return ("raises", e.status)
    return ("ok", r if isinstance(r, list) else [r])


def _same_value(kind, p, q):
    if kind == "f":
        return (p != p and q != q) or bits(p) == bits(q)
    return p == q


def outcomes_equal(o1, o2):
    """two model outcomes under the comparator's rules"""
    if o1[0] != o2[0]:
        return False
    if o1[0] == "raises":
        return o1[1] == o2[1]
    for r1, r2 in zip(o1[1], o2[1]):
        if r1.kind != r2.kind or r1.valid != r2.valid:
            return False
        if not all(_same_value(r1.kind, p, q) for p, q, ok in zip(r1.vals, r2.vals, r1.valid) if ok):
            return False
    return True


# --------------------------------------------------------------------------- the comparator
def assert_column_matches(got, want, what=""):
    """got: a Column (device or oracle); want: the model's Result of the same expression"""
    assert got.dtype == DTYPES[want.kind], f"{what}: dtype {got.dtype}, the model has {DTYPES[want.kind]}"
    assert got.length == len(want.vals), f"{what}: {got.length} rows, the model has {len(want.vals)}"
    ok = np.array(want.valid, dtype=bool)
    gm = got.valid_mask()
    assert np.array_equal(gm, ok), f"{what}: validity differs at rows {np.nonzero(gm != ok)[0][:8].tolist()}"
    if not len(ok):
        return
    fill = False if want.kind == "b" else 0
    e = np.array([fill if v is None else v for v in want.vals], dtype=NP_DTYPES[want.kind])
    g = got.to_numpy()
    assert g.dtype == e.dtype, f"{what}: values are {g.dtype}, expected {e.dtype}"
    if want.kind == "f":
        same = (g.view(np.uint64) == e.view(np.uint64)) | (np.isnan(g) & np.isnan(e))
    else:
        same = g == e
    bad = np.nonzero(~same & ok)[0]
    assert not len(bad), f"{what}: {len(bad)} of {int(ok.sum())} valid rows differ from the model, first rows {bad[:4].tolist()}: got {[g[i].item() for i in bad[:4]]} model {[e[i].item() for i in bad[:4]]}"


def assert_columns_match(got_cols, want, what=""):
    assert len(got_cols) == len(want), f"{what}: {len(got_cols)} columns, the model has {len(want)}"
    for i, (g, w) in enumerate(zip(got_cols, want)):
        assert_column_matches(g, w, f"{what} column {i}")


# --------------------------------------------------------------------------- the catalogue
A, B, UU, XX, Y, Z, ZF, BO, ID = (C(name) for name in NAMES)
P2 = lambda k: 2.0 ** k

VALUE_TREES = {
    "int_wrap_chain": X(X(X(A, O.Plus, I(1)), O.Multiply, I(3)), O.Minus, B),                                   # (a + 1) * 3 - b
    "int_literal_minus": X(I(100), O.Minus, A),                                                               # 100 - a
    "magic_divisors": X(X(X(A, O.Modulos, I(1000)), O.Multiply, I(3)), O.Plus, X(A, O.Divide, I(7))),           # (a % 1000) * 3 + a / 7
    "magic_divisors_wide": X(X(A, O.Divide, I(I64_MAX)), O.Minus, X(A, O.Modulos, I(-((1 << 40) + 7)))),        # a / MAX - a % -(2^40 + 7)
    "shift_divisors": X(X(A, O.Divide, I(-8)), O.Plus, X(A, O.Modulos, I(I64_MIN))),                            # a / -8 + a % MIN
    "shift_divisors_one": X(X(A, O.Divide, I(1)), O.Plus, X(A, O.Modulos, I(1))),                               # a / 1 + a % 1
    "column_divisors": X(X(A, O.Divide, B), O.Plus, X(A, O.Modulos, B)),                                       # a / b + a % b
    "u64_divisors": X(X(X(UU, O.Divide, U(10)), O.Plus, X(UU, O.Modulos, U((1 << 63) + 5))), O.Multiply, U(3)),  # (u / 10 + u % (2^63 + 5)) * 3
    "u64_shift_divisors": X(X(UU, O.Divide, U(1 << 63)), O.Plus, X(UU, O.Modulos, U(1 << 20))),                  # u / 2^63 + u % 2^20
    "contraction_bait": X(X(XX, O.Multiply, XX), O.Plus, X(XX, O.Divide, F(4.0))),                              # x * x + x / 4.0
    "fmod_literal": X(X(XX, O.Multiply, F(-2.0)), O.Minus, X(XX, O.Modulos, F(2.5))),                           # x * -2.0 - x % 2.5
    "fmod_column": X(X(XX, O.Divide, Y), O.Plus, X(XX, O.Modulos, Y)),                                         # x / y + x % y
    "reciprocal_limits": X(X(XX, O.Divide, F(P2(1021))), O.Multiply, X(XX, O.Divide, F(-P2(-1021)))),           # x / 2^1021 * (x / -2^-1021)
    "reciprocal_outside": X(X(XX, O.Divide, F(5e-324)), O.Minus, X(XX, O.Divide, F(P2(1023)))),                 # x / 5e-324 - x / 2^1023
    "true_division": X(X(XX, O.Divide, F(3.0)), O.Plus, X(XX, O.Divide, F(0.1))),                               # x / 3.0 + x / 0.1
    "signed_zero": X(X(XX, O.Plus, F(-0.0)), O.Multiply, F(0.0)),                                              # (x + -0.0) * 0.0
    "null_literal": X(X(A, O.Plus, I(None)), O.Multiply, I(3)),                                                # (a + NULL) * 3
    "four_columns_int": X(X(X(A, O.Plus, B), O.Multiply, X(Z, O.Minus, I(1))), O.Plus, X(A, O.Modulos, B)),      # a, b, z — and u below — 3-4 distinct columns
    "four_columns_mixed": X(X(X(XX, O.Multiply, Y), O.Plus, ZF), O.Minus, X(XX, O.Divide, Y)),                  # x * y + zf - x / y   (3 columns)
}
PRED_TREES = {
    "u64_compare_and_wrap": X(X(UU, O.Gt, U(1 << 63)), O.Or, X(X(UU, O.Plus, U(1)), O.Lt, UU)),                  # u > 2^63 or (u + 1) < u
    "i64_wrap_in_predicate": X(X(X(A, O.Plus, I(1)), O.Gt, A), O.And, X(X(A, O.Multiply, I(2)), O.LtEq, B)),     # (a + 1) > a and (a * 2) <= b
    "nan_inf_in_predicate": X(X(X(XX, O.Multiply, F(2.0)), O.Gt, F(100.0)), O.Or, X(X(XX, O.Minus, XX), O.NotEq, F(0.0))),  # x * 2.0 > 100.0 or (x - x) != 0.0
    "float_columns_in_predicate": X(X(XX, O.Lt, Y), O.And, X(X(XX, O.Plus, Y), O.GtEq, F(-0.0))),               # x < y and (x + y) >= -0.0
    "kleene": X(X(BO, O.And, X(XX, O.Lt, F(0.0))), O.Or, L("b", True)),                                        # (bo and x < 0.0) or true
    "kleene_null_literal": X(X(BO, O.Or, L("b", None)), O.And, X(XX, O.GtEq, F(-0.0))),                         # (bo or NULL) and x >= -0.0
    "four_columns_predicate": AND(X(A, O.Lt, B), X(XX, O.GtEq, Y), X(X(A, O.Minus, B), O.Gt, I(0))),             # a < b and x >= y and a - b > 0   (4 columns)
}

COMPARE_LITERALS = {
    "a": [("min", I64_MIN), ("min1", I64_MIN + 1), ("m1", -1), ("0", 0), ("max1", I64_MAX - 1), ("max", I64_MAX)],
    "u": [("0", 0), ("1", 1), ("2p63m1", (1 << 63) - 1), ("2p63", 1 << 63), ("max", U64_MAX)],
    "x": [("p0", 0.0), ("n0", -0.0), ("pinf", INF), ("ninf", -INF), ("nan", NAN), ("pden", 5e-324), ("nden", -5e-324), ("fmax", F64_MAX), ("50", 50.0)],
}
# col cmp lit and lit cmp col, all six operators, every literal
PLAIN_COMPARES = {}
for _c, _lits in COMPARE_LITERALS.items():
    for _tag, _v in _lits:
        for _op in COMPARES:
            PLAIN_COMPARES[f"{_c}_{_op.name}_{_tag}"] = X(C(_c), _op, L(KINDS[_c], _v))
            PLAIN_COMPARES[f"{_tag}_{_op.name}_{_c}"] = X(L(KINDS[_c], _v), _op, C(_c))

# compares behind one fault-free arithmetic step: the tests match_conj accepts
PRE_TESTS = {
    "a_plus": X(X(A, O.Plus, I(1)), O.Gt, I(5)),                    # (a + 1) > 5
    "a_times": X(X(A, O.Multiply, I(2)), O.LtEq, I(10)),            # (a * 2) <= 10
    "lit_minus_a": X(X(I(100), O.Minus, A), O.GtEq, I(7)),          # (100 - a) >= 7
    "u_minus": X(X(UU, O.Minus, U(1)), O.Lt, U(10)),                # (u - 1) < 10
    "a_mod": X(X(A, O.Modulos, I(3)), O.Eq, I(0)),                  # (a % 3) = 0
    "a_div": X(X(A, O.Divide, I(7)), O.NotEq, I(0)),                # (a / 7) != 0
    "x_times": X(X(XX, O.Multiply, F(2.0)), O.Gt, F(100.0)),        # (x * 2.0) > 100.0
    "x_plus_huge": X(X(XX, O.Plus, F(1e300)), O.LtEq, F(INF)),      # (x + 1e300) <= inf
}
_T = PRE_TESTS
CONJ_TREES = dict({f"pre_{k}": v for k, v in PRE_TESTS.items()}, **{
    # straight lists of plain range tests (no arithmetic step): 2 and 4 source columns
    "list_and_2_plain": AND(X(A, O.Gt, I(0)), X(B, O.Lt, I(0))),
    "list_or_4_plain": OR(X(XX, O.Lt, F(0.0)), X(UU, O.Gt, U(1 << 63)), X(A, O.LtEq, I(I64_MAX - 1)), X(Y, O.GtEq, F(-0.0))),
    # lists with arithmetic steps (the truth-table form): 1, 2, 3 and 4 source columns
    "list_and_2_pre_1col": AND(_T["a_plus"], _T["a_mod"]),
    "list_or_2_pre_2col": OR(_T["a_times"], _T["x_times"]),
    "list_and_3_pre_3col": AND(_T["lit_minus_a"], _T["u_minus"], _T["x_plus_huge"]),
    "list_or_4_pre_4col": OR(_T["a_plus"], _T["u_minus"], _T["x_times"], X(B, O.Lt, I(0))),
    "list_and_4_pre": AND(_T["a_div"], _T["a_plus"], _T["x_plus_huge"], X(UU, O.GtEq, U(1))),
    # nested and / or: the truth-table form
    "nested_pre": OR(AND(_T["a_plus"], _T["a_mod"]), X(XX, O.Lt, F(0.0))),
    "nested_plain": OR(AND(X(A, O.Gt, I(0)), X(B, O.Lt, I(0))), X(XX, O.Gt, F(50.0))),
})
ALL_PREDICATES = dict(PRED_TREES, **PLAIN_COMPARES, **CONJ_TREES)

# col [op lit]{1,4}: the chains the consumer kernels evaluate from the streamed word (SimpleExpr); the first four are `x * mul + add`
AFFINE_CHAINS = {
    "a_plus": X(A, O.Plus, I(I64_MAX)),                          # a + MAX
    "lit_minus_a": X(I(100), O.Minus, A),                        # 100 - a
    "a_minus": X(A, O.Minus, I(I64_MIN)),                        # a - MIN
    "u_times": X(UU, O.Multiply, U((1 << 63) + 1)),              # u * (2^63 + 1)
}
WORD_CHAINS = {
    "a_div_magic": X(A, O.Divide, I(7)),
    "a_mod_shift": X(A, O.Modulos, I(-8)),
    "a_div_min": X(A, O.Divide, I(I64_MIN)),
    "u_mod_shift": X(UU, O.Modulos, U(1 << 20)),
    "u_div_magic": X(UU, O.Divide, U(10)),
    "x_div_pow2": X(XX, O.Divide, F(4.0)),
    "x_div_true": X(XX, O.Divide, F(3.0)),
    "x_mod": X(XX, O.Modulos, F(2.5)),
    "x_signed_zero": X(X(XX, O.Plus, F(-0.0)), O.Multiply, F(0.0)),
    "a_chain_3": X(X(X(A, O.Modulos, I(1000)), O.Multiply, I(3)), O.Plus, I(7)),
    "a_chain_4": X(X(X(X(A, O.Plus, I(1)), O.Multiply, I(3)), O.Minus, I(5)), O.Divide, I(7)),
    "x_chain_lit_left": X(F(1e300), O.Multiply, X(F(2.5), O.Minus, XX)),
}
BOOL_CHAINS = {"x_times_cmp": PRE_TESTS["x_times"], "a_mod_cmp": PRE_TESTS["a_mod"], "u_cmp": X(U(1 << 63), O.LtEq, UU)}
# chains that fault on the catalogue's own table (a holds i64::MIN and 0, x both zeros): (tree, a plain compare that drops the faulting rows)
CHAIN_FAULTS = {
    "a_over_minus_one": (X(A, O.Divide, I(-1)), X(A, O.Gt, I(I64_MIN))),
    "a_mod_minus_one": (X(A, O.Modulos, I(-1)), X(A, O.Gt, I(I64_MIN))),
    "lit_over_a": (X(I(100), O.Divide, A), X(A, O.NotEq, I(0))),
    "lit_mod_a": (X(I(100), O.Modulos, A), X(A, O.NotEq, I(0))),
    "lit_over_x": (X(F(1.0), O.Divide, XX), X(XX, O.NotEq, F(0.0))),
}


def chain_steps(tree):
    """the steps of `col [op lit]{0,4}` (either side, no NULL literal, no and / or: expr_plan.hpp match_simple), None for any other tree"""
    if tree[0] == "col":
        return 0
    if tree[0] == "lit" or tree[0] in (O.And, O.Or):
        return None
    l, r = tree[1], tree[2]
    if r[0] == "lit" and r[2] is not None and l[0] != "lit":
        sub = l
    elif l[0] == "lit" and l[2] is not None and r[0] != "lit":
        sub = r
    else:
        return None
    k = chain_steps(sub)
    return None if k is None or k >= 4 else k + 1


# The fault cases: (tree, what make_table plants, a plain compare that DROPS every faulting row, the column made NULL by null_the_faults)
FAULT_CASES = {
    "int_divide_by_zero": (X(A, O.Divide, Z), "z0", X(Z, O.NotEq, I(0))),
    "int_modulus_by_zero": (X(A, O.Modulos, Z), "z0", X(Z, O.NotEq, I(0))),
    "f64_divide_by_positive_zero": (X(XX, O.Divide, ZF), "zf+0", X(ZF, O.NotEq, F(0.0))),
    "f64_divide_by_negative_zero": (X(XX, O.Divide, ZF), "zf-0", X(ZF, O.NotEq, F(0.0))),
    "f64_modulus_by_negative_zero": (X(XX, O.Modulos, ZF), "zf-0", X(ZF, O.NotEq, F(0.0))),
    "min_divided_by_minus_one_column": (X(A, O.Divide, Z), "zm1", X(A, O.Gt, I(I64_MIN))),
    "min_modulus_minus_one_column": (X(A, O.Modulos, Z), "zm1", X(A, O.Gt, I(I64_MIN))),
    "min_divided_by_minus_one_literal": (X(A, O.Divide, I(-1)), None, X(A, O.Gt, I(I64_MIN))),
}


def fault_table(n, seed, case, nullable=False, null_the_faults=False):
    """the table of one fault case: nothing but that case's divisors is planted"""
    plant = FAULT_CASES[case][1]
    return make_table(n, seed, nullable, plant=frozenset([plant] if plant else []), null_the_faults=null_the_faults)


def widen(tree, steps=3):
    """the same value, bit for bit, and the same faults through a tree of at least `steps` steps (the run-time specialised kernels take
    programs of three or more): `* 1` and `- 0` are appended in turn (-0.0 - 0.0 is -0.0; NaN stays NaN)"""
    kind = kind_of(tree)
    one, zero = {"i": (I(1), I(0)), "u": (U(1), U(0)), "f": (F(1.0), F(0.0))}[kind]
    while steps_of(tree) < steps:
        tree = X(tree, O.Minus, zero) if steps_of(tree) % 2 else X(tree, O.Multiply, one)
    return tree
