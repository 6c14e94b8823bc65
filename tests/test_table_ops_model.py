"""The model of the table-primitive tests (tests/table_ops_util.py) held to yardsticks of its own, on the CPU:

  the oracle      the model's slice is orc.limit(orc.offset(...)), the project's restatement of the reference's RecordBatch::slice
                  use (limit.rs / offset.rs), at every (offset, length) the device test walks;
  numpy           the LSB-first bitmap helpers round-trip at every row count of ROWS with garbage in the padding bits, against
                  np.packbits / np.unpackbits;
  itself          unpack(pack(x)) == x for the documented exchange layout, and pack leaves every word it does not own alone."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import table_ops_util as tu  # noqa: E402
from naive_query_engine_amd import DType  # noqa: E402
from oracle import oracle as orc  # noqa: E402


@pytest.mark.parametrize("nullable", [True, False])
def test_model_slice_is_the_oracles_limit_of_offset(nullable):
    table = tu.make_table(11 + nullable, tu.SLICE_SRC_ROWS, nullable)
    cols = tu.to_columns(table)
    cases = tu.slice_cases()
    assert len(cases) > 100 and {off % 64 for off, _ in cases} >= {0, 1, 7, 8, 9, 31, 63}
    for off, ln in cases:
        exp = [tu.slice_(c, off, ln) for c in table]
        batches = orc.limit(orc.offset([cols], off), ln)
        rows = sum(b[0].length for b in batches)
        assert rows == ln, (off, ln, rows)
        if ln == 0:
            continue  # (the oracle hands back no batch or an empty one: there is nothing else to compare)
        got = [tu.concat([tu.from_column(b[i]) for b in batches]) for i in range(len(table))]
        for g, e in zip(got, exp):
            # validity and the valid rows: what lies under a NULL is the copy's own business
            tu.assert_column(tu.to_column(g), e, "any", f"slice({off}, {ln}) {e.dtype.name}")
            assert (g.valid() == e.valid()).all()


def test_model_take_and_concat_agree_with_slice():
    """take by a run of row numbers is the slice; the concat of a table's slices is the table"""
    table = tu.make_table(5, 300, True)
    for c in table:
        for off, ln in [(0, 300), (63, 65), (299, 1), (7, 0)]:
            a, b = tu.take(c, np.arange(off, off + ln)), tu.slice_(c, off, ln)
            tu.assert_column(tu.to_column(a), b, "any", "take of a run")
            assert list(a.values) == list(b.values) if c.dtype == DType.UTF8 else (a.values == b.values).all()
        whole = tu.concat([tu.slice_(c, 0, 64), tu.slice_(c, 64, 0), tu.slice_(c, 64, 236)])
        tu.assert_column(tu.to_column(whole), c, "any", "concat of the slices")
    # a part without a mask counts as all valid
    a, b = tu.MCol(DType.BOOLEAN, np.array([True, False])), tu.MCol(DType.BOOLEAN, np.array([True]), np.array([False]))
    assert tu.concat([a, b]).mask.tolist() == [True, True, False] and tu.concat([a, a]).mask is None


@pytest.mark.parametrize("n", tu.ROWS)
def test_bitmap_helpers_round_trip_with_garbage_padding(n):
    rng = np.random.default_rng(n)
    bits = rng.random(n) < 0.5
    for padding in (0, 1, "random"):
        buf = tu.pack_bitmap(bits, padding, rng)
        assert buf.dtype == np.uint8 and len(buf) == (n + 7) // 8
        assert (tu.unpack_bitmap(buf, n) == bits).all()
        if n:
            assert (np.unpackbits(buf, bitorder="little")[:n].astype(bool) == bits).all()
        if n % 8:
            pad = int(buf[-1]) >> (n % 8)
            if padding == 1:
                assert pad == (0xFF >> (n % 8))
            elif padding == 0:
                assert pad == 0
    # bit i of byte i >> 3, least significant first
    if n:
        one = np.zeros(n, dtype=bool)
        one[n - 1] = True
        assert int(tu.pack_bitmap(one)[-1]) == 1 << ((n - 1) & 7)


def test_concat_cases_reach_every_bit_offset():
    seen = set()
    for lengths in tu.CONCAT_PARTS:
        assert 2 <= len(lengths) <= 9
        seen |= {o for o, n in zip(tu.concat_offsets(lengths), lengths) if n}
    assert seen >= {0, 1, 7, 8, 63}, seen
    assert any(len(p) == 9 for p in tu.CONCAT_PARTS) and any(len(p) == 2 for p in tu.CONCAT_PARTS)
    assert any(o == 63 and n > 64 for p in tu.CONCAT_PARTS for o, n in zip(tu.concat_offsets(p), p))
    for pos in (0, 1, 2):
        assert any(len(p) == 3 and p[pos] == 0 for p in tu.CONCAT_PARTS)
    for mode in tu.MASK_MODES:
        parts = tu.concat_parts(3, [5, 0, 3], mode)
        masks = [t[0].mask is not None for t in parts]
        assert sum(masks) == {"all": 3, "none": 0, "one": 1, "zero_part": 3}[mode]
        if mode == "zero_part":
            assert any(len(t[0]) and not t[0].mask.any() for t in parts)


@pytest.mark.parametrize("rows,extra", [(0, 0), (1, 0), (255, 0), (256, 3), (257, 3), (0, 3)])
def test_pack_unpack_model_round_trips(rows, extra):
    rng = np.random.default_rng(rows + extra)
    stride, ncols = rows + extra, 3
    cols = [rng.integers(0, 1 << 63, rows, dtype=np.uint64) for _ in range(ncols)]
    before = np.full(ncols * stride + 2, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    buf = tu.pack_model(cols, stride, before)
    assert buf[ncols * stride] == rows and buf[ncols * stride + 1] == before[-1]
    for c in range(ncols):
        assert (buf[c * stride + rows:(c + 1) * stride] == before[0]).all()  # the gap up to the stride is not written
    back = tu.unpack_model(buf, [rows], ncols, stride)
    assert all((b == c).all() for b, c in zip(back, cols))
    # two parts back to back, the second shorter
    short = [c[:rows // 2] for c in cols]
    two = np.concatenate([buf[:ncols * stride + 1], tu.pack_model(short, stride, before)[:ncols * stride + 1]])
    back = tu.unpack_model(two, [rows, rows // 2], ncols, stride)
    assert all((b == np.concatenate([c, s])).all() for b, c, s in zip(back, cols, short))
