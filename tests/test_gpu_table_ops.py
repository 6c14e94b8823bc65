"""The table primitives under every operator — take, slice, concat, pack / unpack, count_valid (csrc/context.hip) — against the
plain numpy model of tests/table_ops_util.py (held to the oracle in tests/test_table_ops_model.py), at every bit and word edge.

Everything goes through capi.Context and every comparison is exact: values bit for bit (Float64 by bit pattern), validity bit for
bit, row counts, and a null_count that is either -1 or the true count.  What is pinned beyond the values:

  bit offsets          bitmap_slice reads at off % 64 in {0, 1, 7, 8, 9, 31, 63} of the first, second and 65th word;
  two-word placement   bitmap_place at a running destination offset of {0, 1, 7, 8, 63} mod 64, parts that end on a word edge, parts
                       that start one bit before it and are longer than a word, empty parts, all-NULL parts, parts without a bitmap;
  under a NULL         take writes a zero word, a false bit, an empty string; slice and concat copy, so only validity and the valid
                       rows are pinned there;
  the tail             count_valid reads the last partial word byte by byte and ignores the padding bits of a borrowed bitmap;
  the second grid step one case per kernel at SECOND_STEP rows (the grids are capped at 8 blocks of 256 threads per CU), and one
                       pack / unpack past their own cap of 1024 blocks;
  arguments            the bounds of slice compared without a wrapping addition, concat's and pack / unpack's refusals, which
                       launch nothing and leave the context usable.

count_valid has no case beyond its first grid step: its loop runs over 64-bit words, so that would take over 33 million rows."""
import os
import sys

import numpy as np
import pytest
import torch  # before the library is loaded: the two then share one HIP runtime in this process (the borrowed-memory tests need both)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import table_ops_util as tu  # noqa: E402
from naive_query_engine_amd import Column, DType, ErrorCode, Status  # noqa: E402

pytestmark = pytest.mark.gpu

INT64_MIN, INT64_MAX = -(1 << 63), (1 << 63) - 1


@pytest.fixture(scope="module")
def ctx():
    from naive_query_engine_amd import capi

    return capi.default_context()


class Launches:
    """the kernel launches of the context while the block runs, by name"""

    def __init__(self, ctx):
        self.ctx = ctx

    def __enter__(self):
        self.ctx.timing_enable(True)
        self.ctx.timing_reset()
        return self

    def names(self):
        return set(self.ctx.timing_report())

    def __exit__(self, *exc):
        self.ctx.timing_enable(False)
        self.ctx.timing_reset()


def upload(ctx, table):
    return ctx.table_from_host(tu.to_columns(table))


def index_table(ctx, idx):
    return ctx.table_from_host([Column.from_numpy(np.asarray(idx, dtype=np.int64))])


def check(table, exp, under_null, what):
    """a device table against the model's columns: rows bit for bit, num_rows, and a null_count that is unknown or true"""
    tu.assert_table(table.to_host(), exp, under_null, what)
    assert table.num_rows == len(exp[0]), f"{what}: num_rows {table.num_rows}"
    for i, e in enumerate(exp):
        info = table.column_info(i)
        assert int(info.length) == len(e), f"{what}: length of column {i}"
        assert int(info.null_count) in (-1, e.null_count), f"{what}: column {i} reports null_count {info.null_count}, the true count is {e.null_count}"
        if not info.validity:
            assert e.null_count == 0, f"{what}: column {i} has no validity bitmap but {e.null_count} NULLs"


def raises(status):
    class Ctx:
        def __enter__(self):
            self.cm = pytest.raises(ErrorCode)
            self.info = self.cm.__enter__()
            return self

        def __exit__(self, *exc):
            out = self.cm.__exit__(*exc)
            assert out and self.info.value.status == status, f"expected {status!r}, got {self.info.value!r}"
            return out

    return Ctx()


# one table of SECOND_STEP + 1 rows shared by the second-grid-step cases of slice and concat (never modified)
@pytest.fixture(scope="module")
def big():
    return tu.make_table(77, tu.SECOND_STEP + 1, True)


# --------------------------------------------------------------------------- slice
@pytest.mark.parametrize("nullable", [True, False], ids=["nulls", "no_nulls"])
def test_slice_at_every_bit_offset(ctx, nullable):
    src = tu.make_table(21 + nullable, tu.SLICE_SRC_ROWS, nullable)
    t = upload(ctx, src)
    assert all((t.column_info(i).validity is not None) == nullable for i in range(5))
    with Launches(ctx) as launches:
        for off, ln in tu.slice_cases():
            out = ctx.slice(t, off, ln)
            # slice copies: what lies under a NULL is not pinned, validity and the valid rows are (and a null_count that is not wrong,
            # also for the many short slices here that hold no NULL at all)
            check(out, [tu.slice_(c, off, ln) for c in src], "any", f"slice({off}, {ln}) nullable={nullable}")
        names = launches.names()
    assert {"bitmap_slice", "utf8_take_lengths", "utf8_take_copy", "iota_i64"} <= names, sorted(names)


def test_slice_second_grid_step(ctx, big):
    t = upload(ctx, big)
    with Launches(ctx) as launches:
        out = ctx.slice(t, 1, tu.SECOND_STEP)
        names = launches.names()
    check(out, [tu.slice_(c, 1, tu.SECOND_STEP) for c in big], "any", f"slice(1, {tu.SECOND_STEP})")
    assert {"bitmap_slice", "utf8_take_lengths", "utf8_take_copy"} <= names, sorted(names)


# --------------------------------------------------------------------------- concat
@pytest.mark.parametrize("mode", tu.MASK_MODES)
def test_concat_at_every_destination_offset(ctx, mode):
    with Launches(ctx) as launches:
        for k, lengths in enumerate(tu.CONCAT_PARTS):
            parts = tu.concat_parts(100 * k + len(mode), lengths, mode)
            tables = [upload(ctx, p) for p in parts]
            out = ctx.concat(tables)
            exp = [tu.concat([p[i] for p in parts]) for i in range(5)]
            if mode == "none":
                assert all(e.mask is None for e in exp)
            check(out, exp, "any", f"concat of {lengths} (bit offsets {tu.concat_offsets(lengths)}), masks: {mode}")
            if mode != "none":  # a part without a bitmap came out as ones next to parts with one
                assert all(out.column_info(i).validity for i in range(5))
        names = launches.names()
    assert {"bitmap_place", "utf8_rebase"} <= names, sorted(names)


def test_concat_of_one_owned_table_shares_its_buffers(ctx):
    src = tu.make_table(31, 129, True)
    t = upload(ctx, src)
    with Launches(ctx) as launches:
        out = ctx.concat([t])
        assert launches.names() == set()
    check(out, src, "any", "concat of one library-owned table")
    for i in range(5):
        a, b = t.column_info(i), out.column_info(i)
        assert a.values == b.values and a.validity == b.validity and a.data == b.data, f"column {i} was copied"
        assert int(b.null_count) == src[i].null_count


def test_concat_of_one_borrowed_table_copies(ctx):
    n = 129
    src = [tu.make_column(np.random.default_rng(32), DType.INT64, n, True), tu.make_column(np.random.default_rng(33), DType.FLOAT64, n, False)]
    host = tu.to_columns(src)
    tv0, tm0, tv1 = (torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).cuda() for a in (host[0].values, host[0].validity, host[1].values))
    torch.cuda.synchronize()
    bt = ctx.table_from_device([(DType.INT64, n, tv0.data_ptr(), tm0.data_ptr()), (DType.FLOAT64, n, tv1.data_ptr(), None)])
    assert int(bt.column_info(0).null_count) == src[0].null_count
    out = ctx.concat([bt])
    ctx.synchronize()
    assert out.column_info(0).values != tv0.data_ptr() and out.column_info(1).values != tv1.data_ptr()
    assert out.column_info(0).validity and out.column_info(0).validity != tm0.data_ptr()
    # the borrowed memory is the caller's again: overwrite it, the output must not change
    for tensor in (tv0, tm0, tv1):
        tensor.fill_(0x5A)
    torch.cuda.synchronize()
    check(out, src, "any", "concat of one borrowed table")
    assert int(out.column_info(0).null_count) == src[0].null_count
    del bt


def test_concat_second_grid_step(ctx, big):
    first = tu.make_table(78, 1, True)
    second = [tu.slice_(c, 1, tu.SECOND_STEP) for c in big]
    tables = [upload(ctx, first), upload(ctx, second)]
    with Launches(ctx) as launches:
        out = ctx.concat(tables)
        names = launches.names()
    check(out, [tu.concat([a, b]) for a, b in zip(first, second)], "any", f"concat of 1 + {tu.SECOND_STEP} rows")
    assert {"bitmap_place", "utf8_rebase"} <= names, sorted(names)


# --------------------------------------------------------------------------- take
def take_indices(rng, m, n):
    """(name, int64[m]) over a source of n rows"""
    out = [("all_last", np.full(m, n - 1, dtype=np.int64)), ("random", rng.integers(0, n, m).astype(np.int64))]
    if m == n:
        out += [("identity", np.arange(m, dtype=np.int64)), ("reversed", np.arange(m, dtype=np.int64)[::-1].copy())]
    return out


@pytest.mark.parametrize("nullable", [True, False], ids=["nulls", "no_nulls"])
def test_take_at_every_row_count(ctx, nullable):
    rng = np.random.default_rng(41 + nullable)
    with Launches(ctx) as launches:
        for m in tu.ROWS:  # includes m == 0 and m % 64 == 0 for Utf8: the slot of the scan's total is written by two different branches
            for n in sorted({max(m, 1), 3}):
                src = tu.make_table(1000 + m + n, n, nullable, big_strings=m <= 129)
                t = upload(ctx, src)
                for name, idx in take_indices(rng, m, n):
                    out = ctx.take(t, index_table(ctx, idx))
                    # take promises a zero word, a false bit and an empty string under every NULL
                    check(out, [tu.take(c, idx) for c in src], "zero", f"take {name}, m={m} out of {n} rows, nullable={nullable}")
        names = launches.names()
    assert {"take_words", "take_bits", "utf8_take_lengths", "utf8_take_copy"} <= names, sorted(names)


def test_take_second_grid_step(ctx):
    src = tu.make_table(43, 4097, True)
    t = upload(ctx, src)
    idx = np.random.default_rng(44).integers(0, 4097, tu.SECOND_STEP).astype(np.int64)
    idx[-1] = 4096
    with Launches(ctx) as launches:
        out = ctx.take(t, index_table(ctx, idx))
        names = launches.names()
    check(out, [tu.take(c, idx) for c in src], "zero", f"take of {tu.SECOND_STEP} rows out of 4097")
    assert {"take_words", "take_bits", "utf8_take_lengths", "utf8_take_copy"} <= names, sorted(names)


@pytest.mark.parametrize("nullable", [True, False], ids=["nulls", "no_nulls"])
@pytest.mark.parametrize("bad", [-1, 65, INT64_MIN], ids=["minus_one", "n", "int64_min"])
def test_take_out_of_bounds_index_in_the_last_position(ctx, bad, nullable):
    n = 65
    src = tu.make_table(45, n, nullable)
    t = upload(ctx, src)
    idx = np.arange(n, dtype=np.int64)[::-1].copy()
    idx[-1] = bad
    with raises(Status.ArrowError):
        ctx.take(t, index_table(ctx, idx))
    # the error flag is reset: a correct take right after it, on the same context, succeeds and is right
    idx[-1] = n - 1
    check(ctx.take(t, index_table(ctx, idx)), [tu.take(c, idx) for c in src], "zero", f"take after the failure with index {bad}")


# --------------------------------------------------------------------------- borrowed bitmaps
def borrow_boolean(ctx, torch, n, values, validity):
    """a Boolean column and its validity borrowed from the inside of one uint8 tensor of 0xFF bytes, each at an odd address;
    `values` / `validity`: packed bitmaps.  -> (table, tensor)"""
    nb = (n + 7) // 8
    assert len(values) == len(validity) == nb
    pos_v = 1
    pos_m = pos_v + nb + (1 if (pos_v + nb) % 2 == 0 else 0)
    host = np.full(pos_m + nb + 64, 0xFF, dtype=np.uint8)
    host[pos_v:pos_v + nb] = values
    host[pos_m:pos_m + nb] = validity
    tensor = torch.from_numpy(host).cuda()
    torch.cuda.synchronize()
    base = tensor.data_ptr()
    assert base % 8 == 0 and (base + pos_v) % 2 == 1 and (base + pos_m) % 2 == 1
    return ctx.table_from_device([(DType.BOOLEAN, n, base + pos_v, base + pos_m)]), tensor


@pytest.mark.parametrize("n", [n for n in tu.ROWS if n % 8])
def test_borrowed_bitmaps_at_byte_alignment_with_ones_in_the_padding(ctx, n):
    """Alignment: include/nqe.h describes Boolean values and validity as `ceil(length/8) B` LSB-first bitmaps and asks for no
    alignment (only the 8-byte types are arrays of 64-bit values), so the weakest it permits is one byte: both bitmaps start at an
    odd address inside a larger tensor.  Every byte around them and the padding bits of their last byte are ones, so a kernel that
    reads a whole last word, or rounds the address down, counts or copies bits that are not there."""
    rng = np.random.default_rng(50 + n)
    src = tu.make_column(rng, DType.BOOLEAN, n, True)
    bt, tensor = borrow_boolean(ctx, torch, n, tu.pack_bitmap(src.values, 1), tu.pack_bitmap(src.mask, 1))
    with Launches(ctx) as launches:
        bt2, tensor2 = borrow_boolean(ctx, torch, n, tu.pack_bitmap(src.values, 1), tu.pack_bitmap(src.mask, 1))
        assert "count_valid" in launches.names()
    what = f"borrowed Boolean column of {n} rows"
    # null_count ignores the padding bits (the byte-wise tail of count_valid)
    assert int(bt.column_info(0).null_count) == src.null_count == int(bt2.column_info(0).null_count), what
    assert bt.column_info(0).validity
    for off, ln in sorted({(0, n), (1, n - 1), (n // 2, n - n // 2), (n - 1, 1)}):
        check(ctx.slice(bt, off, ln), [tu.slice_(src, off, ln)], "any", f"{what}: slice({off}, {ln})")
    other = tu.make_column(rng, DType.BOOLEAN, 7, True)
    ot = upload(ctx, [other])
    check(ctx.concat([bt, ot]), [tu.concat([src, other])], "any", f"{what}: concat as the first part")
    check(ctx.concat([ot, bt]), [tu.concat([other, src])], "any", f"{what}: concat as the second part")
    check(ctx.concat([bt]), [src], "any", f"{what}: concat alone")
    for name, idx in take_indices(rng, n, n):
        check(ctx.take(bt, index_table(ctx, idx)), [tu.take(src, idx)], "zero", f"{what}: take {name}")
    ctx.synchronize()
    del bt, bt2, tensor, tensor2


@pytest.mark.parametrize("n", [n for n in tu.ROWS if n % 8])
def test_borrowed_validity_is_dropped_or_kept_by_its_real_bits_only(ctx, n):
    values = np.random.default_rng(60 + n).random(n) < 0.5
    ones = np.ones(n, dtype=bool)
    # every real bit is one, the padding bits are zero: no NULLs, the bitmap is dropped
    bt, tensor = borrow_boolean(ctx, torch, n, tu.pack_bitmap(values, 1), tu.pack_bitmap(ones, 0))
    info = bt.column_info(0)
    assert not info.validity and int(info.null_count) == 0, f"{n} rows, all valid"
    check(ctx.slice(bt, 0, n), [tu.MCol(DType.BOOLEAN, values)], "any", f"{n} rows, all valid")
    # the only zero is the last real bit, the padding bits are ones: one NULL, the bitmap is kept
    last = ones.copy()
    last[n - 1] = False
    bt2, tensor2 = borrow_boolean(ctx, torch, n, tu.pack_bitmap(values, 1), tu.pack_bitmap(last, 1))
    info = bt2.column_info(0)
    assert info.validity and int(info.null_count) == 1, f"{n} rows, the last one NULL"
    check(ctx.slice(bt2, 0, n), [tu.MCol(DType.BOOLEAN, values, last)], "any", f"{n} rows, the last one NULL")
    ctx.synchronize()
    del bt, bt2, tensor, tensor2


# --------------------------------------------------------------------------- pack / unpack
SENTINEL = 0x7EED000000000000


class Scratch:
    """device words from ctx.device_alloc.  Everything goes through the library: fill() writes SENTINEL + i into word i (the row-number
    generator of nqe_synth_fill), read() borrows the words as a UInt64 column and downloads it"""

    def __init__(self, ctx, words):
        self.ctx, self.words = ctx, words
        self.ptr = ctx.device_alloc(words * 8)

    def fill(self):
        self.ctx.synth_fill(0, 0, SENTINEL, self.words, 1, 0, self.ptr)
        before = np.uint64(SENTINEL) + np.arange(self.words, dtype=np.uint64)
        assert (self.read() == before).all()
        return before

    def read(self):
        view = self.ctx.table_from_device([(DType.UINT64, self.words, self.ptr, None)])
        return view.download_column(0).to_numpy().copy()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.ctx.synchronize()
        self.ctx.device_free(self.ptr)


def word_tables(ctx, rng, rows, split):
    """tables of plain 8-byte columns without NULLs, `split` columns each, the dtypes in turn -> (tables, the columns' words)"""
    tables, words = [], []
    for ncols in split:
        cols = [tu.make_column(rng, tu.WORD_DTYPES[(len(words) + j) % 3], rows, False) for j in range(ncols)]
        tables.append(upload(ctx, cols))
        words += [c.values for c in cols]
    return tables, words


@pytest.mark.parametrize("split", [(1,), (30, 18)], ids=["one_column", "48_columns_in_two_tables"])
@pytest.mark.parametrize("rows", [0, 1, 255, 256, 257])
def test_pack_words_layout_header_and_untouched_words(ctx, rows, split):
    rng = np.random.default_rng(70 + rows)
    tables, cols = word_tables(ctx, rng, rows, split)
    ncols = len(cols)
    for stride in (rows, rows + 3):
        with Scratch(ctx, ncols * stride + 2) as buf:  # one word past the header
            before = buf.fill()
            with Launches(ctx) as launches:
                ctx.pack_words(tables, stride, buf.ptr)
                assert launches.names() == {"pack_words"}
            got = buf.read()
            exp = tu.pack_model(cols, stride, before)
            assert got[ncols * stride] == rows, f"header word, rows={rows} stride={stride}"
            assert got[ncols * stride + 1] == before[-1], "the word past the end was written"
            assert (got == exp).all(), f"rows={rows} stride={stride} ncols={ncols}: words {np.flatnonzero(got != exp)[:8]} differ"
            # and back: one part of `rows` rows
            out = ctx.unpack_words(buf.ptr, [rows], [tu.WORD_DTYPES[c % 3] for c in range(ncols)], stride) if stride else None
            if out is not None:
                check(out, [tu.MCol(tu.WORD_DTYPES[c % 3], v) for c, v in enumerate(cols)], "any", f"unpack of the packed buffer, rows={rows} stride={stride}")


def test_pack_words_refusals_launch_nothing(ctx):
    rng = np.random.default_rng(71)
    t49, _ = word_tables(ctx, rng, 4, (30, 19))
    t5, _ = word_tables(ctx, rng, 5, (1,))
    t4, _ = word_tables(ctx, rng, 4, (1,))
    nullable = upload(ctx, [tu.make_column(rng, DType.INT64, 4, True)])
    boolean = upload(ctx, [tu.make_column(rng, DType.BOOLEAN, 4, False)])
    with Scratch(ctx, 49 * 8 + 2) as buf:
        before = buf.fill()
        with Launches(ctx) as launches:
            with raises(Status.NotSupported):
                ctx.pack_words(t49, 8, buf.ptr)  # 49 columns
            with raises(Status.NotSupported):
                ctx.pack_words([nullable], 8, buf.ptr)
            with raises(Status.NotSupported):
                ctx.pack_words([boolean], 8, buf.ptr)
            with raises(Status.InvalidArgument):
                ctx.pack_words(t5, 4, buf.ptr)  # rows > stride
            with raises(Status.InvalidArgument):
                ctx.pack_words(t4 + t5, 8, buf.ptr)  # tables of different row counts
            with raises(Status.InvalidArgument):
                ctx.pack_words([], 8, buf.ptr)
            with raises(Status.InvalidArgument):
                ctx.pack_words(t4, -1, buf.ptr)
            assert launches.names() == set()
        assert (buf.read() == before).all()
        ctx.pack_words(t4, 4, buf.ptr)  # the context is still usable
        assert buf.read()[4] == 4


@pytest.mark.parametrize("counts", [[5], [0], [0, 5], [3, 5], [5, 0], [i % 6 for i in range(64)], [0] * 64, [5] * 64],
                         ids=["1_full", "1_empty", "2_empty_full", "2_short_full", "2_full_empty", "64_mixed", "64_empty", "64_full"])
def test_unpack_words_parts(ctx, counts):
    ncols, stride = 3, 5
    dtypes = [DType.FLOAT64, DType.INT64, DType.UINT64]
    with Scratch(ctx, len(counts) * (ncols * stride + 1)) as buf:
        src = buf.fill()  # every word differs from every other: a wrong index shows
        with Launches(ctx) as launches:
            out = ctx.unpack_words(buf.ptr, counts, dtypes, stride)
            assert launches.names() == ({"unpack_words"} if sum(counts) else set())
        exp = [tu.MCol(dt, v) for dt, v in zip(dtypes, tu.unpack_model(src, counts, ncols, stride))]
        check(out, exp, "any", f"unpack of {len(counts)} parts, counts {counts[:8]}")
        assert out.dtypes() == dtypes and all(int(out.column_info(i).null_count) == 0 and not out.column_info(i).validity for i in range(ncols))
        ctx.synchronize()
        del out


def test_unpack_words_refusals_launch_nothing(ctx):
    with Scratch(ctx, 65 * 16) as buf:
        buf.fill()
        with Launches(ctx) as launches:
            with raises(Status.InvalidArgument):
                ctx.unpack_words(buf.ptr, [1] * 65, [DType.INT64] * 3, 5)  # 65 parts
            with raises(Status.InvalidArgument):
                ctx.unpack_words(buf.ptr, [6], [DType.INT64] * 3, 5)  # a count past the stride
            with raises(Status.InvalidArgument):
                ctx.unpack_words(buf.ptr, [-1], [DType.INT64] * 3, 5)
            with raises(Status.InvalidArgument):
                ctx.unpack_words(buf.ptr, [], [DType.INT64] * 3, 5)
            with raises(Status.NotSupported):
                ctx.unpack_words(buf.ptr, [2], [DType.INT64, DType.BOOLEAN], 5)
            assert launches.names() == set()
        assert ctx.unpack_words(buf.ptr, [1] * 64, [DType.INT64] * 3, 5).num_rows == 64


def test_pack_and_unpack_past_their_own_grid_cap(ctx):
    """both kernels cap their grid at 1024 blocks of 256 threads: 262 144 words per step"""
    rng = np.random.default_rng(73)
    rows, stride = 100_001, 100_004
    tables, cols = word_tables(ctx, rng, rows, (2, 1))
    assert rows * 3 > 262_144
    part = 3 * stride + 1
    with Scratch(ctx, 2 * part + 1) as buf:
        before = buf.fill()
        with Launches(ctx) as launches:
            ctx.pack_words(tables, stride, buf.ptr)
            ctx.pack_words(tables[::-1], stride, buf.ptr + part * 8)  # the second part: the columns in the other table order
            counts = [rows, 43_691]
            out = ctx.unpack_words(buf.ptr, counts, [tu.WORD_DTYPES[c % 3] for c in range(3)], stride)
            assert launches.names() == {"pack_words", "unpack_words"}
        got = buf.read()
        second = [cols[2], cols[0], cols[1]]
        exp = np.concatenate([tu.pack_model(cols, stride, before[:part]), tu.pack_model(second, stride, before[part:])])
        assert (got == exp).all(), f"words {np.flatnonzero(got != exp)[:8]} differ"
        assert sum(counts) * 3 > 262_144
        unpacked = tu.unpack_model(got, counts, 3, stride)
        check(out, [tu.MCol(tu.WORD_DTYPES[c % 3], v) for c, v in enumerate(unpacked)], "any", "unpack of two large parts")
        assert all((u[:rows] == c).all() and (u[rows:] == s[:counts[1]]).all() for u, c, s in zip(unpacked, cols, second))
        ctx.synchronize()
        del out


# --------------------------------------------------------------------------- argument errors of slice and concat
@pytest.fixture(scope="module")
def words_only(ctx):
    """plain 8-byte columns without NULLs: a slice of them is host-side copies only, so a refused slice has launched nothing"""
    src = [tu.make_column(np.random.default_rng(80 + i), dt, 100, False) for i, dt in enumerate(tu.WORD_DTYPES)]
    return src, upload(ctx, src)


@pytest.mark.parametrize("off,ln", [(-1, 5), (0, -1), (INT64_MIN, 0), (0, INT64_MIN), (50, 51), (100, 1), (101, 0), (0, 101), (INT64_MAX, 0), (0, INT64_MAX)])
def test_slice_out_of_bounds_is_refused(ctx, words_only, off, ln):
    src, t = words_only
    with Launches(ctx) as launches:
        with raises(Status.ArrowError):
            ctx.slice(t, off, ln)
        assert launches.names() == set()
    check(ctx.slice(t, 99, 1), [tu.slice_(c, 99, 1) for c in src], "any", "slice after a refused one")
    check(ctx.slice(t, 100, 0), [tu.slice_(c, 100, 0) for c in src], "any", "the empty slice at the end")


@pytest.mark.parametrize("off,ln", [(1 << 62, 1 << 62), (1, INT64_MAX)], ids=["2p62_2p62", "1_int64max"])
def test_slice_bounds_do_not_wrap(ctx, words_only, off, ln):
    """offset + length wraps to a negative number for these pairs; a check by signed addition lets them through and hands back a
    "table" of `ln` rows over empty buffers.  The call must raise — nothing here looks at a table that a wrong NQE_OK returned."""
    src, t = words_only
    with raises(Status.ArrowError):
        ctx.slice(t, off, ln)
    check(ctx.slice(t, 1, 99), [tu.slice_(c, 1, 99) for c in src], "any", "slice after a refused one")


def test_concat_argument_errors(ctx, words_only):
    src, t = words_only
    two = upload(ctx, src[:2])
    swapped = upload(ctx, [src[1], src[0], src[2]])
    with raises(Status.InvalidArgument):
        ctx.concat([])
    with raises(Status.ArrowError):
        ctx.concat([t, two])  # differing column counts
    with raises(Status.ArrowError):
        ctx.concat([t, swapped])  # differing dtypes
    check(ctx.concat([t, t]), [tu.concat([c, c]) for c in src], "any", "concat after the refused ones")
