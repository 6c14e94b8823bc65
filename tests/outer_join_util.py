"""The yardstick of the outer hash join tests (quirk Q19): a numpy / dict model of "HashJoin honouring join_type".  Nothing here
touches the device or the library.

Match relation (the inner hash join's, Q11 included): left = build side, right = probe side, key validity IGNORED — the raw 8-byte
slot of an Int64 / UInt64 key (also under a NULL), the bytes between the offsets of a Utf8 key.
  probe-preserving: probe-row-major (x, y) pairs, the matches of a probe row in ascending build row, a probe row without a match
                    gives (-1, y)
  build-preserving: the build rows that matched in none of the probe batches, ascending, as (x, -1)
A NULL-extended cell holds 0 / false / the empty string under a NULL; an output column has a validity bitmap iff its source has
NULLs or the batch contains a NULL-extended row on that side."""
import numpy as np

from naive_query_engine_amd import Column, DType
from naive_query_engine_amd.arrow_host import pack_bits

_WORD = {DType.INT64: np.int64, DType.UINT64: np.uint64, DType.FLOAT64: np.float64}


# ----------------------------------------------------------------------------- columns
def utf8_column(items):
    """items: bytes / str / None per row (a NULL row has a zero-length span)"""
    raw = [b"" if s is None else (s.encode() if isinstance(s, str) else bytes(s)) for s in items]
    offs = np.zeros(len(raw) + 1, dtype=np.int32)
    if raw:
        offs[1:] = np.cumsum([len(b) for b in raw])
    col = Column(DType.UTF8, len(raw), offs, None, np.frombuffer(b"".join(raw), dtype=np.uint8).copy())
    if any(s is None for s in items):
        col.validity = pack_bits(np.array([s is not None for s in items], dtype=bool))
    return col


def utf8_raw(col):
    """the bytes between the offsets of every row, also under a NULL"""
    raw = col.data.tobytes() if col.data is not None else b""
    offs = np.asarray(col.values).tolist()
    return [raw[offs[i]:offs[i + 1]] for i in range(col.length)]


def has_nulls(col):
    return col.validity is not None and not col.valid_mask().all()


def key_slots(col):
    """what the join compares, per row: the raw 8-byte slot as an unsigned integer, or the bytes of a Utf8 key"""
    if col.dtype == DType.UTF8:
        return utf8_raw(col)
    assert col.dtype in (DType.INT64, DType.UINT64)
    return np.ascontiguousarray(col.values[:col.length]).view(np.uint64).tolist()


# ----------------------------------------------------------------------------- the model
def positions(build_key):
    """raw key slot -> build rows, ascending"""
    pos = {}
    for r, k in enumerate(key_slots(build_key)):
        pos.setdefault(k, []).append(r)
    return pos


def probe_pairs(build_key, probe_key, keep_probe):
    """([x], [y]) of one probe batch; x = -1: NULL-extended"""
    pos = positions(build_key)
    xs, ys = [], []
    for y, k in enumerate(key_slots(probe_key)):
        m = pos.get(k)
        if m:
            xs.extend(m)
            ys.extend([y] * len(m))
        elif keep_probe:
            xs.append(-1)
            ys.append(y)
    return xs, ys


def matched_mask(build_key, probe_keys):
    """bool per build row: matched in some probe batch"""
    pos = positions(build_key)
    hit = np.zeros(build_key.length, dtype=bool)
    for pk in probe_keys:
        for k in set(key_slots(pk)):
            for r in pos.get(k, ()):
                hit[r] = True
    return hit


def unmatched_rows(build_key, probe_keys):
    return np.nonzero(~matched_mask(build_key, probe_keys))[0].tolist()


def take_null(cols, idx):
    """arrow `take` over host columns with a NULL index (-1): the cell holds 0 / false / the empty string under a NULL; the output has a
    validity bitmap iff the source has NULLs or some index is -1.  Float64 bit for bit."""
    idx = np.asarray(idx, dtype=np.int64)
    isnull = idx < 0
    safe = np.where(isnull, 0, idx)
    out = []
    for c in cols:
        src_mask = c.valid_mask()
        mask = (src_mask[safe] if c.length else np.zeros(idx.size, dtype=bool)) & ~isnull
        need = has_nulls(c) or bool(isnull.any())
        if c.dtype == DType.UTF8:
            raw = utf8_raw(c)
            items = [raw[i] if ok else None for i, ok in zip(safe.tolist(), mask.tolist())]
            t = utf8_column(items)
            t.validity = pack_bits(mask) if need else None
            out.append(t)
            continue
        src = c.to_numpy()
        if c.dtype == DType.BOOLEAN:
            vals = (src[safe] if c.length else np.zeros(idx.size, dtype=bool)) & mask
        else:
            vals = (src[safe] if c.length else np.zeros(idx.size, dtype=_WORD[c.dtype])).copy()
            vals.view(np.uint64)[~mask] = 0
        out.append(Column.from_numpy(vals, mask if need else None))
    return out


def null_columns(dtypes, m):
    """m rows of NULL per dtype (no bitmap at 0 rows: no NULL-extended row)"""
    out = []
    mask = np.zeros(m, dtype=bool) if m else None
    for dt in dtypes:
        dt = DType(dt)
        if dt == DType.UTF8:
            c = utf8_column([b""] * m)
            c.validity = pack_bits(mask) if m else None
        elif dt == DType.BOOLEAN:
            c = Column.from_numpy(np.zeros(m, dtype=bool), mask)
        else:
            c = Column.from_numpy(np.zeros(m, dtype=_WORD[dt]), mask)
        out.append(c)
    return out


def outer_probe(left, lkey, right, rkey, keep_probe):
    """the output columns of one probe batch: every left column taken by x, then every right column by y"""
    xs, ys = probe_pairs(left[lkey], right[rkey], keep_probe)
    return take_null(left, xs) + take_null(right, ys)


def unmatched_batch(left, lkey, probe_keys, right_dtypes):
    """the final batch of the build-preserving join"""
    rows = unmatched_rows(left[lkey], probe_keys)
    return take_null(left, rows) + null_columns(right_dtypes, len(rows))


def column_values(col):
    """one Python value per row, None for NULL (bytes for Utf8; Float64 as its bit pattern so that NaN compares)"""
    m = col.valid_mask().tolist()
    if col.dtype == DType.UTF8:
        raw = utf8_raw(col)
        return [raw[i] if m[i] else None for i in range(col.length)]
    vals = col.to_numpy()
    if col.dtype == DType.FLOAT64:
        vals = np.ascontiguousarray(vals).view(np.uint64)
    return [v if ok else None for v, ok in zip(vals.tolist(), m)]


def rows_of(cols):
    return list(zip(*[column_values(c) for c in cols])) if cols else []


def assert_same_columns(got, exp, what="", presence=True, zero_rows=None):
    """bit for bit: dtype, length, validity (and whether a bitmap is present — not compared at 0 rows, where a bitmap has no address)
    and the values of the valid rows; zero_rows: per column None or a bool mask of the NULL-extended rows, whose cells must hold
    0 / false / the empty string"""
    assert len(got) == len(exp), f"{what}: {len(got)} columns, expected {len(exp)}"
    for i, (g, e) in enumerate(zip(got, exp)):
        w = f"{what} column {i}"
        assert g.dtype == e.dtype and g.length == e.length, f"{w}: {g.dtype}[{g.length}] vs {e.dtype}[{e.length}]"
        if presence and e.length:
            assert (g.validity is not None) == (e.validity is not None), f"{w}: validity bitmap {'present' if g.validity is not None else 'absent'}"
        gm, em = g.valid_mask(), e.valid_mask()
        assert (gm == em).all(), f"{w}: validity differs at rows {np.nonzero(gm != em)[0][:8]}"
        zr = None if zero_rows is None or zero_rows[i] is None else np.asarray(zero_rows[i], dtype=bool)
        look = em if zr is None else (em | zr)
        if g.dtype == DType.UTF8:
            gv, ev = utf8_raw(g), utf8_raw(e)
            bad = [j for j in np.nonzero(look)[0].tolist() if gv[j] != ev[j]]
            assert not bad, f"{w}: rows {bad[:8]}: {[gv[j] for j in bad[:4]]} vs {[ev[j] for j in bad[:4]]}"
            continue
        a, b = g.to_numpy(), e.to_numpy()
        if g.dtype != DType.BOOLEAN:
            a, b = np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64)
        bad = np.nonzero((a != b) & look)[0]
        assert bad.size == 0, f"{w}: rows {bad[:8]} differ: {a[bad][:4]} vs {b[bad][:4]}"
