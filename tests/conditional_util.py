"""The numpy model of an NQE_EXPR_CONDITIONAL node (quirk Q28: not, is_null, is_not_null, coalesce, nullif, if) — the yardstick of
tests/test_conditional_model.py (which checks it against pyarrow) and tests/test_gpu_conditional.py (which checks the device against it).

A value is a `Val`: `values` (a numpy array of the dtype's kind; for Utf8 a list of bytes), `valid` (bool[n]) and `nullable` — whether the
column carries a validity buffer at all, which follows from the STATIC form of the expression and never from the data.  Every function
returns exactly what include/nqe.h states: the values where valid, ZERO (0, False, b"") under a NULL row, the validity, and whether a
validity buffer is present (then null_count is -1, else 0)."""
from dataclasses import dataclass

import numpy as np

NOT, IS_NULL, IS_NOT_NULL, COALESCE, NULLIF, IF = range(6)
ARITY = {NOT: 1, IS_NULL: 1, IS_NOT_NULL: 1, COALESCE: 2, NULLIF: 2, IF: 3}
ROW_COUNTS = [0, 1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1023, 1025, 70001]
KINDS = ("i64", "u64", "f64", "bool", "utf8")
NP = {"i64": np.int64, "u64": np.uint64, "f64": np.float64, "bool": np.bool_}


@dataclass
class Val:
    kind: str  # one of KINDS
    values: object
    valid: np.ndarray
    nullable: bool

    def __len__(self):
        return len(self.valid)


def zero_of(kind):
    return b"" if kind == "utf8" else NP[kind](0)


def make(kind, values, valid=None, nullable=None):
    """a column: `valid` None = no validity buffer — nor does an uploaded column keep a bitmap that marks every row valid (a column of no
    rows among them)"""
    n = len(values)
    v = np.ones(n, dtype=bool) if valid is None else np.asarray(valid, dtype=bool)
    vals = list(values) if kind == "utf8" else np.asarray(values, dtype=NP[kind])
    return Val(kind, vals, v, bool((~v).any()) if nullable is None else nullable)


def literal(kind, value, n):
    """a literal expanded to n rows; value None = the NULL literal (nullable, every row NULL)"""
    null = value is None
    fill = zero_of(kind) if null else value
    vals = [fill] * n if kind == "utf8" else np.full(n, fill, dtype=NP[kind])
    return Val(kind, vals, np.full(n, not null, dtype=bool), null)


def _select(kind, take_a, a, b, valid):
    """values: a's where take_a else b's, zero where not valid"""
    if kind == "utf8":
        return [(a[i] if take_a[i] else b[i]) if valid[i] else b"" for i in range(len(valid))]
    out = np.where(take_a, a, b).astype(NP[kind])
    out[~valid] = zero_of(kind)
    return out


def equal_rows(kind, a, b):
    """NQE_OP_EQ on the values (validity aside): IEEE for Float64 (NaN equals nothing, -0.0 equals +0.0), bytes for Utf8"""
    if kind == "utf8":
        return np.array([x == y for x, y in zip(a, b)], dtype=bool)
    with np.errstate(invalid="ignore"):
        return np.asarray(a) == np.asarray(b)


def not_(b):
    assert b.kind == "bool"
    return Val("bool", ~b.values & b.valid, b.valid.copy(), b.nullable)


def is_null(x):
    return Val("bool", ~x.valid, np.ones(len(x), dtype=bool), False)


def is_not_null(x):
    return Val("bool", x.valid.copy(), np.ones(len(x), dtype=bool), False)


def coalesce(a, b):
    assert a.kind == b.kind
    valid = a.valid | b.valid
    return Val(a.kind, _select(a.kind, a.valid, a.values, b.values, valid), valid, a.nullable and b.nullable)


def if_else(c, t, e):
    """t where c is valid and true; e where c is false OR NULL"""
    assert c.kind == "bool" and t.kind == e.kind
    pick = np.asarray(c.values, dtype=bool) & c.valid
    valid = np.where(pick, t.valid, e.valid)
    return Val(t.kind, _select(t.kind, pick, t.values, e.values, valid), valid, t.nullable or e.nullable)


def nullif(a, b):
    """IF(a = b, NULL, a): a NULL a or b makes the compare NULL, so the row is a"""
    assert a.kind == b.kind
    eq = a.valid & b.valid & equal_rows(a.kind, a.values, b.values)
    valid = a.valid & ~eq
    return Val(a.kind, _select(a.kind, np.ones(len(a), dtype=bool), a.values, a.values, valid), valid, True)


def apply(op, *operands):
    return {NOT: not_, IS_NULL: is_null, IS_NOT_NULL: is_not_null, COALESCE: coalesce, NULLIF: nullif, IF: if_else}[op](*operands)


def null_count_of(v):
    """what the C ABI reports: -1 (unknown) with a validity buffer, 0 without"""
    return -1 if v.nullable else 0


# ----------------------------------------------------------------------------- deterministic inputs
def rng_for(*key):
    """a generator seeded by the key's text (the same on every machine and in every process)"""
    return np.random.default_rng(sum((i + 1) * ord(ch) for i, ch in enumerate("|".join(str(k) for k in key))))


STR_LENGTHS = (0, 1, 7, 8, 9, 31, 32, 33)


def values_of(kind, n, seed, small=True):
    """n values of a kind; `small`: few distinct values, so that equal pairs occur (NULLIF)"""
    r = rng_for(kind, n, seed)
    if kind == "i64":
        return r.integers(-3, 4, n).astype(np.int64) if small else r.integers(-(1 << 62), 1 << 62, n).astype(np.int64)
    if kind == "u64":
        return r.integers(0, 5, n).astype(np.uint64) if small else r.integers(0, 1 << 63, n).astype(np.uint64) * np.uint64(2) + np.uint64(1)
    if kind == "f64":
        return r.integers(-3, 4, n).astype(np.float64) / 2.0 if small else r.standard_normal(n)
    if kind == "bool":
        return r.integers(0, 2, n).astype(bool)
    lens = r.integers(0, len(STR_LENGTHS), n)
    tags = r.integers(0, 3, n)
    return [bytes([97 + int(t)]) * STR_LENGTHS[int(k)] for k, t in zip(lens, tags)]


def mask_of(n, seed, frac=0.3):
    """~frac NULL"""
    return rng_for("mask", n, seed).random(n) >= frac


# ----------------------------------------------------------------------------- operand forms and case lists
# the forms an operand takes: a column without validity, one with (~30 % NULL), one that is all NULL, a non-NULL literal, the NULL literal,
# a subtree (an operator node over a nullable column that leaves its values as they are)
FORMS = ("plain", "nullable", "allnull", "lit", "litnull", "sub")
DATA_FORMS = ("plain", "nullable", "sub")
LITERALS = {"i64": -2, "u64": 3, "f64": 0.5, "bool": True, "utf8": b"unknown"}


@dataclass
class Arg:
    kind: str
    form: str
    val: Val  # what the node sees of the operand
    lit: object = None  # the literal's value (None: the NULL literal)


def make_arg(kind, form, n, seed, like=None):
    """`like`: an Arg whose values about half the rows copy (so that NULLIF meets equal pairs)"""
    if form == "lit":
        value = LITERALS[kind] if kind != "bool" else bool(seed % 2)
        return Arg(kind, form, literal(kind, value, n), value)
    if form == "litnull":
        return Arg(kind, form, literal(kind, None, n), None)
    values = values_of(kind, n, seed)
    if like is not None and like.form not in ("litnull",):
        same = rng_for("like", kind, n, seed).random(n) < 0.5
        if kind == "utf8":
            values = [like.val.values[i] if same[i] else values[i] for i in range(n)]
        else:
            values = np.where(same, like.val.values, values).astype(NP[kind])
    if form == "plain":
        return Arg(kind, form, make(kind, values))
    if form == "allnull":
        return Arg(kind, form, make(kind, values, np.zeros(n, dtype=bool)))
    return Arg(kind, form, make(kind, values, mask_of(n, seed)))  # nullable, sub


DIAGONAL = [("nullable", "nullable")] + [(FORMS[i], FORMS[(i + 1) % len(FORMS)]) for i in range(len(FORMS))]
DIAGONAL_IF = [("nullable", "nullable", "nullable"), ("plain", "plain", "plain")] + [(FORMS[i], FORMS[(i + 2) % len(FORMS)], FORMS[(i + 4) % len(FORMS)]) for i in range(len(FORMS))] + \
              [(FORMS[i], FORMS[(i + 1) % len(FORMS)], FORMS[(i + 1) % len(FORMS)]) for i in range(len(FORMS))]


def build_case(op, kind, forms, n, seed=0):
    """(op, [Arg, …], expected Val) of one node"""
    if op in (NOT, IS_NULL, IS_NOT_NULL):
        args = [make_arg("bool" if op == NOT else kind, forms[0], n, seed + 1)]
    elif op == IF:
        args = [make_arg("bool", forms[0], n, seed + 1), make_arg(kind, forms[1], n, seed + 2), make_arg(kind, forms[2], n, seed + 3)]
    else:
        a = make_arg(kind, forms[0], n, seed + 2)
        args = [a, make_arg(kind, forms[1], n, seed + 3, like=a if op == NULLIF else None)]
    return op, args, apply(op, *[a.val for a in args])


def row_count_cases(kind, n):
    """the diagonal of the operand forms for every function of a kind at one row count (the long Utf8 lists are cut: the model is Python)"""
    cut = 3 if (kind == "utf8" and n > 2000) else None
    out = [build_case(op, kind, f, n) for op in (COALESCE, NULLIF) for f in DIAGONAL[:cut]]
    out += [build_case(IF, kind, f, n) for f in DIAGONAL_IF[: (cut and 4)]]
    out += [build_case(op, kind, (f,), n) for op in (IS_NULL, IS_NOT_NULL) for f in FORMS]
    if kind == "bool":
        out += [build_case(NOT, kind, (f,), n) for f in FORMS]
    return out


def grid_cases(kind, op, n=257):
    """every combination of the operand forms of one function at one row count"""
    import itertools

    return [build_case(op, kind, f, n, seed=7 * i) for i, f in enumerate(itertools.product(FORMS, repeat=ARITY[op]))]


def _rows(v):
    vals = v.values if v.kind == "utf8" else np.asarray(v.values).view(np.uint64 if v.kind != "bool" else np.uint8).tolist()
    return set(zip(vals, v.valid.tolist()))


def guard(op, args, expected):
    """the conditions on the INPUTS that keep a case from passing with a constant answer.  Every case of 63 rows and more: the expected
    output is not constant unless every operand is constant by construction (a literal, an all-NULL column).  Cases over data operands
    (plain / nullable / subtree) besides: both values of a Boolean result occur, both sources of a select occur, and some row is NULL
    wherever the form carries a validity buffer."""
    n = len(expected)
    if n < 63:
        return
    what = (op, [a.form for a in args], expected.kind, n)
    data = [a.form in DATA_FORMS for a in args]
    # the operands whose rows reach the output: a literal condition picks one branch, a literal first operand decides COALESCE and NULLIF
    if op == IF:
        c = args[0]
        reach = [c.form in DATA_FORMS, not (c.form in ("litnull", "allnull") or (c.form == "lit" and not c.lit)), not (c.form == "lit" and c.lit)]
        reach[0] = reach[0] and (data[1] or data[2])  # (a data condition over two constants may still pick two different constants: not required)
    elif op == COALESCE:
        reach = [True, args[0].form in ("litnull", "allnull")]
    elif op == NULLIF:
        reach = [True, False]
    else:
        reach = [not (op in (IS_NULL, IS_NOT_NULL) and args[0].form == "plain")]
    if any(d and r for d, r in zip(data, reach)):
        assert len(_rows(expected)) >= 2, ("constant expected output", what)
    if not all(data):
        return
    if expected.kind == "bool" and not (op in (IS_NULL, IS_NOT_NULL) and args[0].form == "plain"):
        seen = set(np.asarray(expected.values)[expected.valid].tolist())
        assert seen == {True, False}, ("a Boolean result with one value", what)
    if op == COALESCE and args[0].form != "plain":
        assert args[0].val.valid.any() and (~args[0].val.valid & args[1].val.valid).any(), ("one source only", what)
    if op == IF:
        pick = np.asarray(args[0].val.values, dtype=bool) & args[0].val.valid
        assert pick.any() and (~pick).any(), ("one branch only", what)
        if args[0].form != "plain":
            assert (~args[0].val.valid).any(), ("no NULL condition", what)
    if op == NULLIF:
        assert (~expected.valid & args[0].val.valid).any() and expected.valid.any(), ("no equal pair, or nothing else", what)
    if expected.nullable:
        assert (~expected.valid).any(), ("no NULL row where the form allows one", what)
