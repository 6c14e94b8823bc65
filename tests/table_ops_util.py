"""The model and the cases of the table-primitive tests: take, slice, concat, pack / unpack (csrc/context.hip).

Plain numpy and Python, no device and no library.  A column is an MCol: the five dtypes of the hot path with one bool per row for
validity (None: no bitmap, which counts as all valid).  Values of the 8-byte types are kept as their uint64 bit patterns, so NaN
payloads, the sign of zero and subnormals are compared as bits; Boolean values are one bool per row; Utf8 values are Python bytes.

The case lists live here so that the CPU test of the model (tests/test_table_ops_model.py) and the device test
(tests/test_gpu_table_ops.py) walk the same rows, offsets and part lists."""
import numpy as np

from naive_query_engine_amd import Column, DType

WORD_DTYPES = (DType.INT64, DType.UINT64, DType.FLOAT64)
WORD_NP = {DType.INT64: np.int64, DType.UINT64: np.uint64, DType.FLOAT64: np.float64}
ALL_DTYPES = (DType.INT64, DType.UINT64, DType.FLOAT64, DType.BOOLEAN, DType.UTF8)

# every row count at which a byte, a ballot word or the 64-word step of a bitmap kernel begins or ends
ROWS = [0, 1, 7, 8, 9, 63, 64, 65, 127, 128, 129, 4095, 4096, 4097]
# past 256 CUs x 8 blocks x 256 threads (the cap of every grid-stride loop), and 600 001 % 64 == 1: it ends inside a ballot word
SECOND_STEP = 600_001

I64_EDGES = np.array([-(1 << 63), (1 << 63) - 1, -1, 0, 1, 1 << 31, -(1 << 31) - 1, (1 << 53) + 1], dtype=np.int64).view(np.uint64)
U64_EDGES = np.array([(1 << 64) - 1, 0, 1, 1 << 63, (1 << 63) - 1, 1 << 32], dtype=np.uint64)
F64_EDGES = np.array([0x7FF8000000000000, 0x7FF0000000000001, 0xFFF8000000000BAD, 0x7FF4DEADBEEF0001,  # NaNs: quiet, signalling, negative, payload
                      0x8000000000000000, 0x0000000000000000,                                          # -0.0, +0.0
                      0x0000000000000001, 0x000FFFFFFFFFFFFF, 0x8000000000000001,                      # subnormals
                      0x7FF0000000000000, 0xFFF0000000000000, 0x3FF0000000000000], dtype=np.uint64)    # +inf, -inf, 1.0
UTF8_EDGES = [b"", b"a", b"seven77", b"eight888", b"nine99999", b"fifteen 1234567", b"sixteen 12345678", b"seventeen 1234567",
              bytes((i * 7 + 3) % 251 + 1 for i in range(3001)),  # a few KB: several 8-byte words and a tail per lane
              "héllo wörld ✓ 日本語".encode("utf-8"), b"nul\x00inside", b"\x00"]


class MCol:
    """one model column: dtype, values (uint64 bit patterns / bool / list of bytes) and mask (bool per row, or None)"""

    __slots__ = ("dtype", "values", "mask")

    def __init__(self, dtype, values, mask=None):
        self.dtype = DType(dtype)
        self.values = values
        self.mask = None if mask is None else np.asarray(mask, dtype=bool)
        assert self.mask is None or len(self.mask) == len(values)

    def __len__(self):
        return len(self.values)

    def valid(self):
        return np.ones(len(self), dtype=bool) if self.mask is None else self.mask

    @property
    def null_count(self):
        return 0 if self.mask is None else int((~self.mask).sum())


# ----------------------------------------------------------------------------- the primitives
def take(col, idx):
    idx = np.asarray(idx, dtype=np.int64)
    assert len(idx) == 0 or (idx.min() >= 0 and idx.max() < len(col))
    vals = [col.values[i] for i in idx] if col.dtype == DType.UTF8 else col.values[idx]
    return MCol(col.dtype, vals, None if col.mask is None else col.mask[idx])


def slice_(col, off, ln):
    assert 0 <= off and 0 <= ln and off + ln <= len(col)
    return MCol(col.dtype, col.values[off:off + ln], None if col.mask is None else col.mask[off:off + ln])


def concat(parts):
    dt = parts[0].dtype
    assert all(p.dtype == dt for p in parts)
    if dt == DType.UTF8:
        vals = [s for p in parts for s in p.values]
    else:
        vals = np.concatenate([p.values for p in parts])
    mask = None
    if any(p.mask is not None for p in parts):
        mask = np.concatenate([p.valid() for p in parts])  # a part without a mask counts as all valid
    return MCol(dt, vals, mask)


def pack_model(cols, stride, before):
    """the documented layout over a copy of `before` (what the destination held): dst[c*stride + r] = cols[c][r], and the header
    word dst[ncols*stride] = rows; every other word is left as it was"""
    rows = len(cols[0])
    assert all(len(c) == rows for c in cols) and rows <= stride and len(before) >= len(cols) * stride + 1
    out = np.array(before, dtype=np.uint64)
    for c, v in enumerate(cols):
        out[c * stride:c * stride + rows] = v
    out[len(cols) * stride] = rows
    return out


def unpack_model(buf, counts, ncols, stride):
    """len(counts) packed parts of ncols*stride + 1 words back to back -> ncols columns, the parts concatenated per column"""
    part_words = ncols * stride + 1
    assert len(buf) >= len(counts) * part_words and all(0 <= k <= stride for k in counts)
    return [np.concatenate([buf[p * part_words + c * stride:p * part_words + c * stride + k] for p, k in enumerate(counts)]).astype(np.uint64)
            for c in range(ncols)]


# ----------------------------------------------------------------------------- bitmaps
def pack_bitmap(bits, padding=0, rng=None):
    """bool[n] -> LSB-first uint8[ceil(n/8)]; the unused high bits of the last byte are `padding`: 0, 1 or "random" """
    bits = np.asarray(bits, dtype=bool)
    n = len(bits)
    out = np.packbits(bits, bitorder="little")
    if n % 8:
        pad_mask = np.uint8((0xFF << (n % 8)) & 0xFF)
        if padding == 1:
            out[-1] |= pad_mask
        elif padding == "random":
            out[-1] |= np.uint8(rng.integers(0, 256)) & pad_mask
        else:
            assert padding == 0
    return out


def unpack_bitmap(buf, n):
    """the first n bits of an LSB-first bitmap as bool[n]: bit i is (buf[i >> 3] >> (i & 7)) & 1"""
    buf = np.asarray(buf, dtype=np.uint8)
    i = np.arange(n, dtype=np.int64)
    return ((buf[i >> 3] >> (i & 7).astype(np.uint8)) & 1).astype(bool)


# ----------------------------------------------------------------------------- data
def _random_strings(rng, n):
    lens = rng.integers(0, 13, n)
    offs = np.concatenate([[0], np.cumsum(lens)])
    pool = rng.integers(97, 123, int(offs[-1])).astype(np.uint8).tobytes()
    return [pool[a:b] for a, b in zip(offs[:-1].tolist(), offs[1:].tolist())]


def _plant(vals, edges, n):
    """the edge values at the first rows and again at the last rows, as far as n has room"""
    k = min(len(edges), n)
    for i in range(k):
        vals[i] = edges[i]
    if n >= 2 * len(edges):
        for i, e in enumerate(edges):
            vals[n - len(edges) + i] = e


def make_column(rng, dtype, n, nullable, big_strings=True):
    dtype = DType(dtype)
    if dtype in WORD_DTYPES:
        vals = rng.integers(1, 1 << 63, n, dtype=np.uint64) | np.uint64(1)  # never zero: a zeroed NULL slot shows
        if dtype == DType.FLOAT64:
            vals = (rng.standard_normal(n) * 1e3).view(np.uint64) | np.uint64(1)
        _plant(vals, {DType.INT64: I64_EDGES, DType.UINT64: U64_EDGES, DType.FLOAT64: F64_EDGES}[dtype], n)
    elif dtype == DType.BOOLEAN:
        vals = rng.random(n) < 0.5
    else:
        vals = _random_strings(rng, n)
        _plant(vals, UTF8_EDGES if big_strings else [e for e in UTF8_EDGES if len(e) < 100], n)
    mask = None
    if nullable:
        mask = rng.random(n) > 0.25
        if n:
            mask[int(rng.integers(0, n))] = False  # at least one NULL: an all-valid bitmap is dropped on upload
        for i in np.flatnonzero(~mask):  # something under every NULL that a copy would carry along
            if dtype in WORD_DTYPES and vals[i] == 0:
                vals[i] = np.uint64(0xDEAD)
            elif dtype == DType.BOOLEAN:
                vals[i] = True
            elif dtype == DType.UTF8 and not vals[i]:
                vals[i] = b"under-null"
    return MCol(dtype, vals, mask)


def make_table(seed, n, nullable, big_strings=True):
    """one column of each of the five dtypes, edge values planted; `nullable`: a mask with at least one NULL on every column (for n > 0)"""
    rng = np.random.default_rng(seed)
    return [make_column(rng, dt, n, nullable, big_strings) for dt in ALL_DTYPES]


def to_column(col):
    """the host Arrow column of an MCol, with whatever lies under the NULLs kept"""
    n = len(col)
    validity = None if col.mask is None else pack_bitmap(col.mask)
    if col.dtype == DType.UTF8:
        lens = np.fromiter((len(s) for s in col.values), dtype=np.int64, count=n)
        offs = np.zeros(n + 1, dtype=np.int32)
        np.cumsum(lens, out=offs[1:])
        data = np.frombuffer(b"".join(col.values), dtype=np.uint8).copy()
        return Column(DType.UTF8, n, offs, validity, data)
    if col.dtype == DType.BOOLEAN:
        return Column(DType.BOOLEAN, n, pack_bitmap(col.values), validity)
    return Column(col.dtype, n, np.ascontiguousarray(col.values, dtype=np.uint64).view(WORD_NP[col.dtype]), validity)


def to_columns(table):
    return [to_column(c) for c in table]


def _utf8_bytes(offs, data, rows):
    """the bytes of the given rows of an Arrow Utf8 column, back to back (a gather without a Python loop)"""
    starts, lens = offs[:-1][rows], (offs[1:] - offs[:-1])[rows]
    total = int(lens.sum())
    if total == 0:
        return b""
    first = np.cumsum(lens) - lens
    pos = np.repeat(starts - first, lens) + np.arange(total, dtype=np.int64)
    return np.asarray(data, dtype=np.uint8)[pos].tobytes()


def assert_column(got, exp, under_null, what):
    """a host Column (what the device produced) against an MCol, bit for bit.  under_null == "zero": a NULL slot holds a zero word,
    a false bit or an empty string (what take promises); "any": only validity and the valid rows are compared (copies)"""
    assert under_null in ("zero", "any")
    assert got.dtype == exp.dtype, f"{what}: dtype {got.dtype!r} != {exp.dtype!r}"
    n = len(exp)
    assert got.length == n, f"{what}: {got.length} rows, expected {n}"
    mask = exp.valid()
    gm = got.valid_mask()
    assert (gm == mask).all(), f"{what}: validity differs at rows {np.flatnonzero(gm != mask)[:8]}"
    if exp.dtype == DType.UTF8:
        offs = np.asarray(got.values, dtype=np.int64)
        assert len(offs) == n + 1 and offs[0] >= 0 and (np.diff(offs) >= 0).all(), f"{what}: offsets are not ascending"
        data = got.data if got.data is not None else np.zeros(0, np.uint8)
        assert offs[-1] <= len(data), f"{what}: the last offset {offs[-1]} is past the {len(data)} data bytes"
        elens = np.fromiter((len(s) for s in exp.values), dtype=np.int64, count=n)
        glens = np.diff(offs)
        if under_null == "zero":
            elens = np.where(mask, elens, 0)
            assert offs[0] == 0 and (glens == elens).all(), f"{what}: string lengths differ at rows {np.flatnonzero(glens != elens)[:8]}"
        else:
            assert (glens[mask] == elens[mask]).all(), f"{what}: string lengths differ at valid rows {np.flatnonzero((glens != elens) & mask)[:8]}"
        ebytes = b"".join(s for s, ok in zip(exp.values, mask.tolist()) if ok)
        assert _utf8_bytes(offs, data, mask) == ebytes, f"{what}: string bytes differ"
        return
    if exp.dtype == DType.BOOLEAN:
        g, e = unpack_bitmap(got.values, n), np.asarray(exp.values, dtype=bool)
        zero = False
    else:
        g, e = np.ascontiguousarray(got.values)[:n].view(np.uint64), np.asarray(exp.values, dtype=np.uint64)
        zero = np.uint64(0)
    if under_null == "zero":
        e = np.where(mask, e, zero)
        bad = g != e
    else:
        bad = (g != e) & mask
    assert not bad.any(), f"{what}: values differ at rows {np.flatnonzero(bad)[:8]}: {g[bad][:4]} != {e[bad][:4]}"


def assert_table(got, exp, under_null, what):
    assert len(got) == len(exp), f"{what}: {len(got)} columns, expected {len(exp)}"
    for i, (g, e) in enumerate(zip(got, exp)):
        assert_column(g, e, under_null, f"{what}, column {i} ({e.dtype.name})")


def from_column(col):
    """a host Column as an MCol (for yardsticks that hand Columns back)"""
    n = col.length
    mask = None if col.validity is None else unpack_bitmap(col.validity, n)
    if col.dtype == DType.UTF8:
        raw = bytes(np.asarray(col.data if col.data is not None else np.zeros(0, np.uint8), dtype=np.uint8).tobytes())
        offs = np.asarray(col.values, dtype=np.int64)
        return MCol(col.dtype, [raw[offs[i]:offs[i + 1]] for i in range(n)], mask)
    if col.dtype == DType.BOOLEAN:
        return MCol(col.dtype, unpack_bitmap(col.values, n), mask)
    return MCol(col.dtype, np.ascontiguousarray(col.values)[:n].view(np.uint64).copy(), mask)


# ----------------------------------------------------------------------------- cases
SLICE_SRC_ROWS = 4161  # 65 words and one bit


def slice_cases(rows=SLICE_SRC_ROWS):
    """(offset, length): every off % 64 of {0, 1, 7, 8, 9, 31, 63} in the first, the second and the 65th word, crossed with lengths
    around a word (clamped to the table), then the slice that ends at the last row and the whole table"""
    cases = []
    for k in (0, 1, 64):
        for r in (0, 1, 7, 8, 9, 31, 63):
            off = 64 * k + r
            assert off < rows
            for ln in (0, 1, 63, 64, 65, 129):
                cases.append((off, min(ln, rows - off)))
            cases.append((off, rows - off))  # ends exactly at the last row
    cases.append((rows, 0))
    cases.append((0, rows))
    return list(dict.fromkeys(cases))


# part lengths; the running destination bit offset (mod 64) of each part is in the comment
CONCAT_PARTS = [
    [1, 63],                              # 0, 1 -> ends exactly on the word edge
    [63, 1, 64],                          # 0, 63, 0
    [63, 130],                            # 0, 63: one bit before the edge and longer than 64 -> every ballot word is split in two
    [127, 130, 3],                        # 0, 63 (second word), 1
    [7, 129],                             # 0, 7
    [8, 200, 1],                          # 0, 8, 16
    [0, 5, 3],                            # an empty part first
    [5, 0, 3],                            # ... in the middle
    [5, 3, 0],                            # ... last
    [1, 6, 1, 55, 1, 64, 65, 63, 9],      # nine parts: 0, 1, 7, 8, 63, 0, 0, 1, 0
    [64, 64],                             # whole words only: the spill word gets an all-zero OR
    [4097, 4095],                         # more than one block per part: 0, 1
]
# which parts carry a mask: every part, none, only one (the others must come out as ones), and every part with one of them all NULL
MASK_MODES = ["all", "none", "one", "zero_part"]


def concat_offsets(lengths):
    return [int(x) % 64 for x in np.concatenate([[0], np.cumsum(lengths)[:-1]])]


def concat_parts(seed, lengths, mode):
    """the tables of one concat case"""
    rng = np.random.default_rng(seed)
    pick = int(rng.integers(0, len(lengths)))
    while lengths[pick] == 0:
        pick = (pick + 1) % len(lengths)
    parts = []
    for k, n in enumerate(lengths):
        nullable = mode in ("all", "zero_part") or (mode == "one" and k == pick)
        t = make_table(int(rng.integers(0, 1 << 31)), n, nullable, big_strings=False)
        if mode == "zero_part" and k == pick:
            for c in t:
                c.mask[:] = False
        parts.append(t)
    return parts
