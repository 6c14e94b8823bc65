"""The numpy / Python model of a cast (quirk Q29: NQE_EXPR_CAST) and the case lists of its tests.  The model restates the table of
include/nqe.h in Python's own terms — math.trunc and exact integers for Float64 -> integer, float(int) for integer -> Float64 (correctly
rounded, ties to even), regular expressions over bytes and int() / float() for the parsers, str() for the texts — and is written
without reading cast_parts.hpp.  tests/test_cast_model.py checks it against pyarrow.compute.cast wherever pyarrow has an answer.

A value set is a Val: `values` (a numpy array; a list of bytes for Utf8), `valid`, and `nullable` — whether the column carries a
validity buffer at all, which for a result is a property of the static form (include/nqe.h), not of the rows.

The rows of every from -> to pair come in two lists.  ARROW_ROWS are inputs the model calls valid AND pyarrow converts: edge values plus
seeded random ones; test_cast_model.py sends every one of them through pyarrow.  HAND_ROWS are (input, expected) pairs written by hand,
expected None = NULL: the rows pyarrow raises on (it has no NULL-on-failure cast), and the integer strings with a leading `+`, which this
library's grammar takes ([+-]digits+, the CSV reader's) and pyarrow's does not.  pair_rows() interleaves them so that at least half of
any prefix of two or more rows are ARROW_ROWS."""
import math
import re
import zlib

import numpy as np

KINDS = ("bool", "i64", "u64", "f64", "utf8")
NP = {"i64": np.int64, "u64": np.uint64, "f64": np.float64, "bool": np.bool_}
I64_MIN, I64_MAX, U64_MAX = -(1 << 63), (1 << 63) - 1, (1 << 64) - 1
NAN, INF = float("nan"), float("inf")
PAIRS = [(f, t) for f in KINDS for t in KINDS if f != t and (f, t) != ("f64", "utf8")]


class Val:
    def __init__(self, kind, values, valid=None, nullable=None):
        self.kind = kind
        self.values = list(values) if kind == "utf8" else np.asarray(values, dtype=NP[kind])
        n = len(self.values)
        self.valid = np.ones(n, dtype=bool) if valid is None else np.asarray(valid, dtype=bool)
        self.nullable = (valid is not None) if nullable is None else nullable

    def __len__(self):
        return len(self.values)


def zero_of(kind):
    return {"i64": 0, "u64": 0, "f64": 0.0, "bool": False, "utf8": b""}[kind]


def fallible(frm, to):
    """can a valid operand give NULL?  (the result then always carries a validity buffer, null_count -1)"""
    return frm != to and (frm == "utf8" or (frm, to) in (("i64", "u64"), ("u64", "i64"), ("f64", "i64"), ("f64", "u64")))


_INT = re.compile(rb"[+-]?[0-9]+")
_UINT = re.compile(rb"\+?[0-9]+")
_FLOAT = re.compile(rb"[+-]?(?:(?:[0-9]+(?:\.[0-9]*)?|\.[0-9]+)(?:[eE][+-]?[0-9]+)?|[nN][aA][nN]|[iI][nN][fF](?:[iI][nN][iI][tT][yY])?)")


def cast_one(frm, to, v):
    """one valid value -> the value in `to`, or None where `to` cannot represent it"""
    if frm == "f64" and to in ("i64", "u64"):
        x = float(v)
        if x != x or x in (INF, -INF):
            return None
        t = math.trunc(x)  # an exact Python integer: -0.5 -> 0
        lo, hi = (I64_MIN, I64_MAX) if to == "i64" else (0, U64_MAX)
        return t if lo <= t <= hi else None
    if frm in ("i64", "u64") and to in ("i64", "u64"):
        lo, hi = (I64_MIN, I64_MAX) if to == "i64" else (0, U64_MAX)
        return int(v) if lo <= int(v) <= hi else None
    if frm in ("i64", "u64") and to == "f64":
        return float(int(v))  # Python rounds an integer to the nearest binary64, ties to even
    if to == "bool" and frm != "utf8":
        return bool(float(v) != 0.0) if frm == "f64" else int(v) != 0  # NaN != 0: true; -0.0 == 0: false
    if frm == "bool" and to != "utf8":
        return float(bool(v)) if to == "f64" else int(bool(v))
    if to == "utf8":
        return (b"true" if v else b"false") if frm == "bool" else str(int(v)).encode()
    s = bytes(v)
    if to == "i64":
        return int(s) if _INT.fullmatch(s) and I64_MIN <= int(s) <= I64_MAX else None
    if to == "u64":
        return int(s) if _UINT.fullmatch(s) and int(s) <= U64_MAX else None
    if to == "f64":
        return float(s.decode()) if _FLOAT.fullmatch(s) else None
    return {b"true": True, b"false": False}.get(s.lower())


def cast(val, to):
    """the model: `val` (a Val) cast to `to`"""
    if val.kind == to:
        return val  # the operand itself
    assert (val.kind, to) in PAIRS, (val.kind, to)
    out, valid = [], np.zeros(len(val), dtype=bool)
    for i in range(len(val)):
        r = cast_one(val.kind, to, val.values[i]) if val.valid[i] else None
        valid[i] = r is not None
        out.append(zero_of(to) if r is None else r)
    return Val(to, out, valid, nullable=fallible(val.kind, to) or val.nullable)


def rng_for(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def mask_of(n, seed, frac=0.3):
    m = rng_for("mask", seed).random(n) >= frac
    if n >= 1:
        m[0] = False  # (an uploaded bitmap that marks every row valid is dropped: a nullable column holds a NULL)
    if n >= 2:
        m[1] = True
    return m


def _next(x, toward):
    return float(np.nextafter(x, toward))


def _random_rows(frm, to, count):
    r = rng_for("rows", frm, to)
    if frm == "bool":
        return [bool(b) for b in r.integers(0, 2, count)]
    if to == "bool" and frm in ("i64", "u64"):
        return [int(x) for x in r.choice([0, 0, 1, 2, 1 << 40, I64_MAX], count)]
    if frm == "i64":
        lo, hi = (0, I64_MAX) if to == "u64" else (I64_MIN, I64_MAX)
        big = [int(x) for x in r.integers(lo, hi, count // 2, dtype=np.int64)]
        return big + [int(x) for x in r.integers(0 if to == "u64" else -1000, 1000, count - count // 2)]
    if frm == "u64":
        hi = I64_MAX if to == "i64" else U64_MAX
        return [int(x) for x in r.integers(0, hi, count // 2, dtype=np.uint64)] + [int(x) for x in r.integers(0, 1000, count - count // 2)]
    if frm == "f64":
        if to == "bool":
            return [float(x) for x in r.choice([0.0, -0.0, 1.5, -2.0, 1e-300, NAN, INF], count)]
        small = [float(x) for x in (r.integers(-4000, 4000, count // 2) / 4.0)]
        wide = [float(x) for x in r.integers(0, 1 << 61, count - count // 2) * r.choice([1.0, -1.0, 0.5, 2.0], count - count // 2)]
        return [x if to == "i64" else abs(x) for x in small + wide]  # (below 2^63 in magnitude: valid rows of either target)
    # Utf8: texts of the target's own grammar
    if to == "bool":
        return [bytes(x) for x in r.choice([b"true", b"false", b"TRUE", b"False", b"tRuE", b"fALSE"], count)]
    if to in ("i64", "u64"):
        out = []
        for k in range(count):
            digits = int(r.integers(1, 20 if to == "u64" else 19))
            v = int(r.integers(0, 10 ** digits, dtype=np.uint64)) if digits < 20 else int(r.integers(0, U64_MAX, dtype=np.uint64))
            s = str(v).encode()
            out.append(b"-" + s if to == "i64" and k % 3 == 0 else b"00" + s if k % 7 == 0 else s)
        return out
    out = []
    for k in range(count):
        m, e = int(r.integers(0, 10 ** int(r.integers(1, 19)))), int(r.integers(-30, 30))
        forms = [b"%d" % m, b"%d.%d" % (m, m % 1000), b"-%d.5" % m, b"%de%d" % (m, e), b"%d.%dE%+d" % (m % 100, m, e), b".%d" % m, b"%d." % m]
        out.append(forms[k % len(forms)])
    return out


_LONG40 = b"1234567890123456789012345678901234567890"
_LONG400 = bytes(ord("1") + (k * 7) % 9 for k in range(400))

# inputs the model calls valid and pyarrow converts: the edges first
_ARROW_EDGES = {
    ("f64", "i64"): [0.0, -0.0, 0.5, -0.5, 1.5, -1.5, 2.5, -2.0 ** 63, _next(-2.0 ** 63, 0.0), _next(2.0 ** 63, 0.0), 2.0 ** 53 + 2, 5e-324, -5e-324, 1e18],
    ("f64", "u64"): [0.0, -0.0, 0.5, -0.5, _next(-1.0, 0.0), 1.5, 2.5, _next(2.0 ** 64, 0.0), 2.0 ** 63, _next(2.0 ** 63, INF), 5e-324, -5e-324, 1e19],
    ("i64", "f64"): [0, 1, -1, 2 ** 53, 2 ** 53 + 1, 2 ** 53 + 2, 2 ** 53 + 3, -(2 ** 53) - 1, I64_MAX, I64_MAX - 511, I64_MAX - 512, I64_MAX - 513, I64_MIN, I64_MIN + 1],
    ("u64", "f64"): [0, 1, 2 ** 53 + 1, 2 ** 53 + 3, I64_MAX, 1 << 63, (1 << 63) + 1024, (1 << 63) + 1025, (1 << 63) + 3072, U64_MAX, U64_MAX - 1023, U64_MAX - 1024, U64_MAX - 1022,
                     U64_MAX - 3071, U64_MAX - 3072, U64_MAX - 3070],
    ("i64", "u64"): [0, 1, I64_MAX, I64_MAX - 1, 12345],
    ("u64", "i64"): [0, 1, I64_MAX, I64_MAX - 1, 12345],
    ("bool", "i64"): [True, False], ("bool", "u64"): [True, False], ("bool", "f64"): [True, False], ("bool", "utf8"): [True, False],
    ("i64", "bool"): [0, 1, 0, -1, 2, 0, I64_MIN, I64_MAX, 0, 1 << 32, 256, 0], ("u64", "bool"): [0, 1, 0, 2, 1 << 63, 0, U64_MAX, 1 << 32, 0, 256],
    ("f64", "bool"): [0.0, 1.0, -0.0, -1.0, NAN, 0.0, INF, -INF, -0.0, 5e-324, 0.5, 0.0],
    ("i64", "utf8"): [0, 1, -1, 9, 10, -9, -10, I64_MAX, I64_MIN, I64_MIN + 1] + [10 ** k for k in range(19)] + [10 ** k - 1 for k in range(1, 19)] + [-(10 ** k) for k in range(19)],
    ("u64", "utf8"): [0, 1, 9, 10, U64_MAX, 1 << 63, I64_MAX] + [10 ** k for k in range(20)] + [10 ** k - 1 for k in range(1, 20)],
    ("utf8", "i64"): [b"0", b"7", b"-7", b"007", b"-0", b"9223372036854775807", b"-9223372036854775808", b"0000000000000000000000000000000000000012", b"-00000000000000000000000000000000000000012",
                      b"0" * 399 + b"5"],
    ("utf8", "u64"): [b"0", b"7", b"007", b"18446744073709551615", b"9223372036854775808", b"0000000000000000000000000000000000000012", b"0" * 399 + b"5", b"00018446744073709551615"],
    ("utf8", "f64"): [b"0", b"-0", b"1.5", b"-1.5", b"+1.5", b"1.", b".5", b"1e3", b"1E3", b"1e+3", b"1e-3", b"nan", b"NaN", b"+nan", b"inf", b"-inf", b"Infinity", b"+INFINITY", b"1e400", b"-1e400",
                      b"1e-400", b"9007199254740993", b"9007199254740992.5", b"0.1", b"1e23", b"8.5e22", b"1.7976931348623157e308", b"2.2250738585072011e-308", b"4.9e-324", b"2.4703282292062328e-324",
                      b"2.4703282292062327e-324", b"9223372036854775807", b"18446744073709551615", b"12345678901234567890", _LONG40, b"0." + _LONG40, _LONG40 + b"e-20", _LONG400, b"0." + _LONG400,
                      _LONG400[:200] + b"." + _LONG400[200:], _LONG400 + b"e-391", b"9007199254740993" + b"0" * 384 + b"e-384", b"9007199254740993" + b"0" * 383 + b"1e-384"],
    ("utf8", "bool"): [b"true", b"false", b"TRUE", b"FALSE", b"True", b"False", b"tRuE"],
}

# (input, expected): None = NULL.  Rows pyarrow has no answer for (it raises), and the integers with a leading `+`
HAND_ROWS = {
    ("f64", "i64"): [(NAN, None), (INF, None), (-INF, None), (2.0 ** 63, None), (_next(2.0 ** 63, INF), None), (_next(-2.0 ** 63, -INF), None), (1e19, None), (-1e19, None), (1e300, None), (2.0 ** 64, None)],
    ("f64", "u64"): [(NAN, None), (INF, None), (-INF, None), (-1.0, None), (_next(-1.0, -INF), None), (-1.5, None), (2.0 ** 64, None), (_next(2.0 ** 64, INF), None), (-2.0 ** 63, None), (1e300, None), (-1e-300 - 2, None)],
    ("i64", "u64"): [(-1, None), (I64_MIN, None), (-12345, None), (I64_MIN + 1, None)],
    ("u64", "i64"): [(1 << 63, None), (U64_MAX, None), ((1 << 63) + 12345, None)],
    ("utf8", "i64"): [(b"", None), (b" ", None), (b"+", None), (b"-", None), (b" 1", None), (b"1 ", None), (b"9223372036854775808", None), (b"-9223372036854775809", None), (b"1e3", None), (b"1.0", None),
                      (b"99999999999999999999", None), (b"12a", None), (b"--1", None), (b"0x10", None), (b"1" * 40, None), (b"1" * 400, None),
                      (b"+7", 7), (b"+0", 0), (b"+9223372036854775807", I64_MAX)],
    ("utf8", "u64"): [(b"", None), (b"+", None), (b"-", None), (b"-0", None), (b"-7", None), (b" 1", None), (b"1 ", None), (b"18446744073709551616", None), (b"99999999999999999999", None), (b"1e3", None),
                      (b"1.0", None), (b"12a", None), (b"1" * 40, None), (b"1" * 400, None), (b"+7", 7), (b"+18446744073709551615", U64_MAX)],
    ("utf8", "f64"): [(b"", None), (b" ", None), (b"+", None), (b"-", None), (b".", None), (b"e5", None), (b"1e", None), (b"1e+", None), (b" 1.5", None), (b"1.5 ", None), (b"1.2.3", None), (b"1,5", None),
                      (b"0x1p3", None), (b"infinit", None), (b"nanx", None), (b"--1", None), (b"1e5.5", None), (b"abc", None), (b"1_0", None), (_LONG400 + b"x", None)],
    ("utf8", "bool"): [(b"", None), (b"1", None), (b"0", None), (b"t", None), (b"f", None), (b"yes", None), (b" true", None), (b"true ", None), (b"truee", None), (b"fals", None)],
}


def arrow_rows(frm, to):
    edges = _ARROW_EDGES[(frm, to)]
    want = max(24, 2 * len(HAND_ROWS.get((frm, to), [])) + 8) - len(edges)
    return list(edges) + (_random_rows(frm, to, max(8, want)) if frm != "bool" else [True, False, False, True] * 4)


def pair_rows(frm, to):
    """[(input, expected, through_arrow)]: two ARROW_ROWS, one HAND_ROW, … then the rest — at least half of any prefix of two or more
    rows are ARROW_ROWS; `expected` is the model's for an ARROW_ROW and the hand-written one for a HAND_ROW"""
    arrow = [(v, cast_one(frm, to, v), True) for v in arrow_rows(frm, to)]
    hand = [(v, x, False) for v, x in HAND_ROWS.get((frm, to), [])]
    out = []
    while arrow or hand:
        out += arrow[:2]
        arrow = arrow[2:]
        if hand:
            out.append(hand.pop(0))
    return out


def pair_column(frm, to, n, nullable=False, seed=0):
    """an n-row operand of `frm` for the cast to `to`, cycling through pair_rows; nullable: ~30 % NULLs"""
    rows = pair_rows(frm, to)
    values = [rows[i % len(rows)][0] for i in range(n)]
    return Val(frm, values, mask_of(n, (frm, to, n, seed)) if nullable else None)


def guard(frm, to, expected):
    """no constant answer passes: with enough rows the expected column holds two different values, and NULLs and values where it can"""
    n = len(expected)
    if n < 8:
        return
    vals = [expected.values[i] for i in range(n) if expected.valid[i]]
    keys = {bytes(v) if expected.kind == "utf8" else (float(v).hex() if expected.kind == "f64" else int(v)) for v in vals}
    assert len(keys) >= 2, (frm, to, "the expected values are constant")
    if fallible(frm, to):
        assert expected.valid.any() and not expected.valid.all(), (frm, to, "a fallible cast whose expected validity is constant")


def null_count_of(operand_form, operand, frm, to):
    """what the C ABI reports: -1 with a buffer of the result's own (fallible); else the operand's — an uploaded column's NULLs are counted
    when the table is created, an expanded NULL literal's are its rows, a binary node's result says -1 with a buffer and 0 without (a
    string node carries its operand's count)"""
    if frm != to and fallible(frm, to):
        return -1
    if operand_form == "litnull":
        return len(operand)
    if operand_form == "lit" or not operand.nullable:
        return 0
    return int((~operand.valid).sum()) if operand_form == "nullable" or frm == "utf8" else -1
