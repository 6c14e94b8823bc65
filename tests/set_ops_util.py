"""The yardstick of the DISTINCT / set-operator tests (quirk Q24): a row-at-a-time Python model.  Nothing here touches the device or
the library.

Tuple equality, per key column (tuple_keys): Int64 / UInt64 the integer; Float64 with -0.0 = +0.0 and every NaN one value; Boolean
the bit; Utf8 the bytes; a NULL equals a NULL whatever lies under it and differs from every value; the empty string is a value.
Tuples compare position by position.
  distinct(cols, key_cols)   the rows that are the FIRST occurrence of their tuple, in input order, every column taken from that row
  set_op(left, right, op)    every column a key.  INTERSECT: the rows of distinct(left) whose tuple occurs in right; EXCEPT: the
                             rest; UNION: distinct(concat(left, right))
Rows are copied (order_by_util.take: Float64 bit for bit), so the device has to agree exactly (order_by_util.assert_same_rows)."""
import math

import numpy as np

import order_by_util as obu
from naive_query_engine_amd import Column, DType, SetOp

EDGE_ROWS = [0, 1, 2, 63, 64, 65, 2048, 2049, 4095, 4096, 4097, 12289]  # the mask word, the 4096-row tile, a capacity doubling, several tiles


def _value_key(dtype, v):
    if v is None:
        return ("null",)
    if dtype == DType.FLOAT64:
        return ("nan",) if math.isnan(v) else ("f", v + 0.0)  # (-0.0 + 0.0 is +0.0)
    if dtype == DType.UTF8:
        return ("s", bytes(v))
    if dtype == DType.BOOLEAN:
        return ("b", bool(v))
    return ("i", int(v))


def tuple_keys(cols, key_cols=None):
    """one hashable per row: equal exactly when the rows' tuples over `key_cols` (None: every column) are equal under Q24"""
    key_cols = range(len(cols)) if key_cols is None else key_cols
    per_col = [[_value_key(cols[c].dtype, v) for v in obu.column_values(cols[c])] for c in key_cols]
    n = cols[0].length if cols else 0
    return list(zip(*per_col)) if per_col else [()] * n


def distinct_rows(cols, key_cols=None):
    """the input rows a DISTINCT keeps, ascending"""
    seen, rows = set(), []
    for i, k in enumerate(tuple_keys(cols, key_cols)):
        if k not in seen:
            seen.add(k)
            rows.append(i)
    return rows


def distinct(cols, key_cols=None):
    return obu.take(cols, distinct_rows(cols, key_cols))


def set_op_rows(left, right, op):
    """(source columns, the rows of the source the operator keeps)"""
    op = SetOp(op)
    if op == SetOp.Union:
        both = obu.concat_columns([left, right])
        return both, distinct_rows(both)
    in_right = set(tuple_keys(right))
    lk = tuple_keys(left)
    rows = [i for i in distinct_rows(left) if (lk[i] in in_right) == (op == SetOp.Intersect)]
    return left, rows


def set_op(left, right, op):
    src, rows = set_op_rows(left, right, op)
    return obu.take(src, rows)


# ----------------------------------------------------------------------------- seeded tables
def key_columns(rng, shape, n, distinct_tuples):
    """the key columns of one of the named key shapes, holding about `distinct_tuples` different tuples (n: every row its own)"""
    d = max(1, min(n, distinct_tuples)) if n else 1
    ids = rng.integers(0, d, n) if d < n else rng.permutation(n)
    u = lambda a: Column.from_numpy(np.asarray(a).astype(np.uint64))
    i = lambda a: Column.from_numpy(np.asarray(a).astype(np.int64))
    if shape == "i64":
        return [i(ids * 7 - 3)]
    if shape == "words2":
        return [i(ids % 5 - 2), u(ids // 5)]
    if shape == "words4":
        return [i(ids % 3), u(ids // 3 % 3), i(-(ids // 9 % 3)), u(ids // 27)]
    if shape == "words5":
        return [i(ids % 3), u(ids // 3 % 3), i(-(ids // 9 % 3)), u(ids // 27 % 3), i(ids // 81)]
    assert shape == "five_dtypes"
    # every tuple id fixes the five values AND which of them are NULL, so `d` bounds the number of different tuples
    nulls = lambda salt: ((ids * 2654435761 + salt) >> 3) % 4 != 0
    f = np.array([0.0, -0.0, np.nan, 1.5, -np.inf, 2.0 ** -1074], dtype=np.float64)
    words = obu.WORDS
    return [Column.from_numpy((ids * 3 - 1).astype(np.int64), nulls(1)), Column.from_numpy((ids // 2).astype(np.uint64), nulls(2)),
            Column.from_numpy(f[ids % f.size] + (ids // f.size), nulls(3)), Column.from_numpy((ids % 2).astype(bool), nulls(4)),
            obu.utf8_column([words[int(t) % len(words)] + str(int(t) // len(words)).encode() if ok else None for t, ok in zip(ids, nulls(5))], null_bytes=b"zz")]


KEY_SHAPES = ["i64", "words2", "words4", "words5", "five_dtypes"]


def payload_columns(rng, n):
    """two payload columns outside the keys: the row number, and a Utf8 column with NULLs"""
    return [Column.from_numpy(np.arange(n, dtype=np.int64)), obu.random_column(rng, DType.UTF8, n, True)]


def random_table(rng, n, dtypes, null_fraction, distinct=5):
    cols = []
    for dt in dtypes:
        c = obu.random_column(rng, dt, n, False, distinct)
        if null_fraction > 0:
            mask = rng.random(n) >= null_fraction
            if dt == DType.UTF8:
                vals = obu.column_values(c)
                c = obu.utf8_column([v if ok else None for v, ok in zip(vals, mask.tolist())], null_bytes=b"q")
                if c.validity is None and n:
                    c.validity = obu.pack_bits(np.ones(n, dtype=bool))
            else:
                c = Column.from_numpy(c.to_numpy(), mask)
        cols.append(c)
    return cols


# ----------------------------------------------------------------------------- golden queries (tests/golden/set_ops_expected.json)
def golden_load(golden_dir):
    """(the document, {table name: (fields, columns)}): the CSV tables the queries name and the hand-made tables of the file itself"""
    import json
    import os

    from naive_query_engine_amd import Field, read_csv

    with open(os.path.join(golden_dir, "set_ops_expected.json")) as f:
        doc = json.load(f)
    tables = {}
    for name in doc["csv_tables"]:
        batch = read_csv(os.path.join(golden_dir, name + ".csv"))
        tables[name] = (list(batch.fields), list(batch.columns))
    for name, t in doc["tables"].items():
        fields = [Field(n, DType[dt], True) for n, dt in t["fields"]]
        cols = [Column.from_list([r[i] for r in t["rows"]], f.dtype) for i, f in enumerate(fields)]
        tables[name] = (fields, cols)
    return doc, tables


def golden_input(tables, spec):
    """(fields, columns) of {"table": name, "columns": [names] or null}"""
    fields, cols = tables[spec["table"]]
    if spec["columns"] is None:
        return fields, cols
    idx = [[f.name for f in fields].index(c) for c in spec["columns"]]
    return [fields[i] for i in idx], [cols[i] for i in idx]


def golden_model(tables, q):
    """(field names, rows) of a golden query by the model"""
    if q["kind"] == "distinct":
        fields, cols = golden_input(tables, q["input"])
        names = [f.name for f in fields]
        out = distinct(cols, None if q["on"] is None else [names.index(c) for c in q["on"]])
    else:
        fields, cols = golden_input(tables, q["left"])
        out = set_op(cols, golden_input(tables, q["right"])[1], SetOp[q["op"]])
    return [f.name for f in fields], [list(r) for r in zip(*[c.to_list() for c in out])]
