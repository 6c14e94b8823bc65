"""The yardstick of the ORDER BY tests (quirk Q18): a pure-Python model — Python's stable `sorted` over one key tuple per row — and a
seeded table generator.  The oracle has no sort; nothing here touches the device or the library.

The order of one key (column, descending, nulls_first):
  NULL rows first or last as nulls_first says, whatever `descending` says; among themselves they tie
  Int64 signed, UInt64 unsigned, Boolean false < true
  Float64 as OrderedFloat: -0.0 ties with +0.0, every NaN ties with every NaN and is greater than +inf
  Utf8 by bytes (memcmp; the shorter string first on a common prefix)
  descending reverses the values
Keys are lexicographic, the first most significant; rows that tie on every key keep their input order.

sort_indices_np is the same order by one stable np.lexsort, for the tables of 10^6 rows of tests/test_gpu_order_by_sizes.py;
tests/test_large_models_host.py holds it against sort_indices."""
import math

import numpy as np

from naive_query_engine_amd import Column, DType
from naive_query_engine_amd.arrow_host import pack_bits


# ----------------------------------------------------------------------------- columns
def utf8_column(items, null_bytes=b""):
    """items: bytes / str / None per row; a NULL row's offsets span `null_bytes` (arrow allows a non-empty span under a NULL)"""
    raw = [null_bytes if s is None else (s.encode() if isinstance(s, str) else bytes(s)) for s in items]
    offs = np.zeros(len(raw) + 1, dtype=np.int32)
    if raw:
        offs[1:] = np.cumsum([len(b) for b in raw])
    col = Column(DType.UTF8, len(raw), offs, None, np.frombuffer(b"".join(raw), dtype=np.uint8).copy())
    if any(s is None for s in items):
        col.validity = pack_bits(np.array([s is not None for s in items], dtype=bool))
    return col


def column_values(col):
    """one Python value per row, None for NULL: int, float, bool, or bytes for Utf8"""
    m = col.valid_mask().tolist()
    if col.dtype == DType.UTF8:
        raw = col.data.tobytes() if col.data is not None else b""
        offs = col.values.tolist()
        return [raw[offs[i]:offs[i + 1]] if m[i] else None for i in range(col.length)]
    vals = col.to_numpy().tolist()
    return [v if ok else None for v, ok in zip(vals, m)]


def concat_columns(parts):
    """the columns of several batches, one after the other (the model's concat_batches)"""
    out = []
    for cols in zip(*parts):
        dt = cols[0].dtype
        vals = [v for c in cols for v in column_values(c)]
        if dt == DType.UTF8:
            out.append(utf8_column(vals))
            continue
        mask = np.array([v is not None for v in vals], dtype=bool)
        if dt == DType.BOOLEAN:
            arr = np.array([bool(v) for v in vals], dtype=bool)
        elif dt == DType.FLOAT64:
            arr = np.concatenate([c.to_numpy() for c in cols]) if vals else np.zeros(0, np.float64)  # bit for bit
        else:
            arr = np.array([v or 0 for v in vals], dtype={DType.INT64: np.int64, DType.UINT64: np.uint64}[dt])
        out.append(Column.from_numpy(arr, None if mask.all() and all(c.validity is None for c in cols) else mask))
    return out


# ----------------------------------------------------------------------------- the model
def _value_key(dtype, v, descending):
    if dtype == DType.UTF8:
        # descending: every byte inverted and a terminator above all of them, so that the LONGER string comes first on a common prefix
        return tuple(255 - b for b in v) + (256,) if descending else tuple(v)
    if dtype == DType.FLOAT64:
        k = (1, 0.0) if math.isnan(v) else (0, v + 0.0)
        return (-k[0], -k[1]) if descending else k
    k = int(v)
    return -k if descending else k


def row_keys(cols, keys):
    """one tuple per row: for every key (null rank, value key)"""
    per_key = []
    for col, desc, nulls_first in keys:
        c = cols[col]
        vals = column_values(c)
        null_rank, valid_rank = (0, 1) if nulls_first else (1, 0)
        per_key.append([(null_rank, 0) if v is None else (valid_rank, _value_key(c.dtype, v, desc)) for v in vals])
    return list(zip(*per_key)) if per_key else []


def sort_indices(cols, keys, fetch=None):
    """the model's lexsort_to_indices: input row numbers in output order"""
    keys = normalise_keys(keys)
    n = cols[0].length if cols else 0
    rk = row_keys(cols, keys)
    order = sorted(range(n), key=rk.__getitem__)
    return order if fetch is None else order[:fetch]


def normalise_keys(keys):
    return [(k, False, True) if isinstance(k, int) else tuple(k) + (False, True)[len(k) - 1:] for k in keys]


# ----------------------------------------------------------------------------- the same model, vectorised
def _utf8_ranks(col):
    """the dense rank of every row's string in memcmp order (a NULL row: 0).  The strings become one fixed-width byte row each, zero
    padded, so a string and the same string followed by NUL bytes would tie: embedded NULs are refused."""
    n = col.length
    if n == 0:
        return np.zeros(0, dtype=np.int64)
    offs = np.asarray(col.values, dtype=np.int64)
    lens = np.where(col.valid_mask(), np.diff(offs), 0)
    width = max(1, int(lens.max()))
    rows = np.repeat(np.arange(n, dtype=np.int64), lens)
    within = np.arange(rows.size, dtype=np.int64) - np.repeat(np.cumsum(lens) - lens, lens)
    data = np.asarray(col.data, dtype=np.uint8) if col.data is not None else np.zeros(0, dtype=np.uint8)
    picked = data[np.repeat(offs[:-1], lens) + within]
    if (picked == 0).any():
        raise ValueError("sort_indices_np: a Utf8 key holds a NUL byte; use sort_indices")
    buf = np.zeros((n, width), dtype=np.uint8)
    buf[rows, within] = picked
    return np.unique(buf.view(f"S{width}").ravel(), return_inverse=True)[1].astype(np.int64).ravel()


def key_arrays(cols, keys):
    """per key, most significant array first: arrays over the rows whose lexicographic order is the key's order and on which two rows
    agree exactly when they tie on the key (Float64 arrays compare -0.0 = +0.0; a NaN is a flag of its own, never a value)"""
    out = []
    for col, desc, nulls_first in normalise_keys(keys):
        c = cols[col]
        ok = c.valid_mask()
        arrs = []
        if c.validity is not None and not ok.all():
            arrs.append(np.where(ok, 1, 0).astype(np.int8) if nulls_first else np.where(ok, 0, 1).astype(np.int8))
        if c.dtype == DType.UTF8:
            r = _utf8_ranks(c)
            arrs.append(np.where(ok, -r if desc else r, 0))
        elif c.dtype == DType.FLOAT64:
            v = c.to_numpy().astype(np.float64)
            nan = ok & np.isnan(v)
            v = np.where(ok & ~nan, v, 0.0)
            arrs.append(np.where(nan, -1, 0).astype(np.int8) if desc else nan.astype(np.int8))  # NaN: above +inf
            arrs.append(-v if desc else v)
        elif c.dtype == DType.BOOLEAN:
            v = c.to_numpy().astype(np.uint8)
            arrs.append(np.where(ok, 1 - v if desc else v, 0).astype(np.uint8))
        else:
            v = ~c.to_numpy() if desc else c.to_numpy().copy()  # ~v reverses the order of either integer type and cannot overflow
            v[~ok] = 0
            arrs.append(v)
        out.append(arrs)
    return out


def sort_indices_np(cols, keys, fetch=None):
    """sort_indices by one stable np.lexsort (fast enough for 10^6 rows): the same order, as an int64 array.  Utf8 keys must hold no NUL
    byte.  tests/test_large_models_host.py holds it against sort_indices."""
    n = cols[0].length if cols else 0
    arrs = [a for per_key in key_arrays(cols, keys) for a in per_key]
    order = np.lexsort(arrs[::-1]).astype(np.int64) if arrs and n else np.arange(n, dtype=np.int64)  # lexsort: the LAST array is the most significant
    return order if fetch is None else order[:fetch]


def take(cols, idx):
    """arrow take over host columns, Float64 bit for bit"""
    idx = np.asarray(idx, dtype=np.int64)
    out = []
    for c in cols:
        mask = c.valid_mask()[idx] if c.validity is not None else None
        if c.dtype == DType.UTF8:
            vals = column_values(c)
            t = utf8_column([vals[i] for i in idx.tolist()])
            if c.validity is not None and t.validity is None:
                t.validity = pack_bits(np.ones(len(idx), dtype=bool))
            out.append(t)
        else:
            out.append(Column.from_numpy(c.to_numpy()[idx], mask))
    return out


def order_by(cols, keys, fetch=None):
    return take(cols, sort_indices(cols, keys, fetch))


def assert_same_rows(got, exp, what=""):
    """value for value and NULL for NULL; Float64 bit for bit (NaN payloads and the sign of zero survive a take)"""
    assert len(got) == len(exp), f"{what}: {len(got)} columns, expected {len(exp)}"
    for i, (g, e) in enumerate(zip(got, exp)):
        w = f"{what} column {i}"
        assert g.dtype == e.dtype and g.length == e.length, f"{w}: {g.dtype}[{g.length}] vs {e.dtype}[{e.length}]"
        # (whether a column WITHOUT NULLs carries a bitmap is not compared: an upload drops an all-ones bitmap, and a 0-row one has no address)
        gm, em = g.valid_mask(), e.valid_mask()
        assert (gm == em).all(), f"{w}: validity differs at rows {np.nonzero(gm != em)[0][:8]}"
        if g.dtype == DType.UTF8:
            gv, ev = column_values(g), column_values(e)
            bad = [j for j in range(g.length) if gv[j] != ev[j]]
            assert not bad, f"{w}: rows {bad[:8]}: {[gv[j] for j in bad[:4]]} vs {[ev[j] for j in bad[:4]]}"
            continue
        a, b = g.to_numpy()[em], e.to_numpy()[em]
        if g.dtype == DType.FLOAT64:
            a, b = a.view(np.uint64), b.view(np.uint64)
        bad = np.nonzero(a != b)[0]
        assert bad.size == 0, f"{w}: valid rows {bad[:8]} differ: {a[bad][:4]} vs {b[bad][:4]}"


# ----------------------------------------------------------------------------- seeded tables
SPECIAL_F64 = np.array([0.0, -0.0, np.inf, -np.inf, 5e-324, -5e-324, 2.2250738585072009e-308, 1.0, -1.0, 1.5, -2.5], dtype=np.float64)
NAN_BITS = np.array([0x7ff8000000000000, 0xfff8000000000000, 0x7ff0000000000001, 0xfff0000000000001, 0x7fffffffffffffff, 0xffffffffffffffff,
                     0x7ff8000000001234], dtype=np.uint64)
WORDS = [b"", b"a", b"a\0", b"ab", b"b", b"abcdefg", b"abcdefgh", b"abcdefghi", b"abcdefgh\0", b"abcdefghijklmnop", b"abcdefghijklmnopq",
         b"abcdefghijklmnoq", "é".encode(), b"\x7f", "ÿz".encode(), b"abcdefghijklmnopqrstuvwx-1", b"abcdefghijklmnopqrstuvwx-2", b"Z"]


def random_column(rng, dtype, n, nullable, distinct=None):
    """a seeded column with the dtype's awkward values mixed in; `distinct`: about that many different values (heavy ties)"""
    mask = rng.random(n) > 0.2 if nullable else None
    if dtype == DType.INT64:
        if distinct:
            arr = rng.integers(-distinct // 2, distinct // 2 + 1, n).astype(np.int64)
        else:
            arr = rng.integers(np.iinfo(np.int64).min, np.iinfo(np.int64).max, n, dtype=np.int64, endpoint=True)
            if n:
                arr[rng.integers(0, n, min(n, 4))] = [np.iinfo(np.int64).min, np.iinfo(np.int64).max, 0, -1][:min(n, 4)]
    elif dtype == DType.UINT64:
        arr = rng.integers(0, distinct, n).astype(np.uint64) if distinct else rng.integers(0, np.iinfo(np.uint64).max, n, dtype=np.uint64, endpoint=True)
    elif dtype == DType.FLOAT64:
        pool = np.concatenate([SPECIAL_F64.view(np.uint64), NAN_BITS]).view(np.float64)
        arr = pool[rng.integers(0, pool.size, n)].copy() if distinct else np.where(rng.random(n) < 0.3, pool[rng.integers(0, pool.size, n)], rng.normal(0, 1e3, n))
    elif dtype == DType.BOOLEAN:
        arr = rng.random(n) < 0.5
    else:
        words = WORDS[:distinct] if distinct else WORDS
        pick = rng.integers(0, len(words), n).tolist()
        items = [words[p] for p in pick]
        if mask is not None:
            items = [s if ok else None for s, ok in zip(items, mask.tolist())]
        return utf8_column(items, null_bytes=b"zz")
    return Column.from_numpy(np.ascontiguousarray(arr), mask)


ALL_DTYPES = [DType.INT64, DType.UINT64, DType.FLOAT64, DType.BOOLEAN, DType.UTF8]


def random_table(seed, n=None, ncols=None):
    """(columns, keys): a seeded table of every dtype with and without validity, and a key list over it"""
    rng = np.random.default_rng(seed)
    n = int(rng.choice([0, 1, 2, 63, 64, 65, 257, 1000, 4096, 4097, 5000])) if n is None else n
    ncols = int(rng.integers(2, 7)) if ncols is None else ncols
    cols = []
    for _ in range(ncols):
        dt = ALL_DTYPES[int(rng.integers(0, len(ALL_DTYPES)))]
        distinct = int(rng.choice([0, 2, 5, 17]))
        cols.append(random_column(rng, dt, n, bool(rng.random() < 0.5), distinct or None))
    cols.append(Column.from_numpy(np.arange(n, dtype=np.int64)))  # the row number: stability shows in it
    nkeys = int(rng.integers(1, 4))
    keys = [(int(rng.integers(0, ncols)), bool(rng.random() < 0.5), bool(rng.random() < 0.5)) for _ in range(nkeys)]
    return cols, keys
