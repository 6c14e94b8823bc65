"""GPU CSV ingest at every chunk, workgroup and carry edge of the record splitter (csrc/csv.hip), and at the row counts where the
per-record stages change.  The files come from tests/csv_util.py (tests/test_csv_split_model.py shows on the CPU that they enter
every edge in every automaton state and that each modelled kernel mistake mis-splits at least one of them); every file goes
through nqe_csv_infer_schema + nqe_csv_read and must equal the oracle's sequential reader exactly: names, dtypes, nullable flags,
row count, Int64 values, Float64 bit patterns, Boolean values, validity, Utf8 offsets and bytes.  No tolerance anywhere.

Errors: the status against the oracle, the record number in the message against the construction (the numbering the library
prints: data row + 1, + 1 again with a header)."""
import functools
import os
import re

import numpy as np
import pytest

from naive_query_engine_amd import Column, DType, ErrorCode, Status
from oracle import oracle as orc
from tests import csv_util as cu

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ctx():
    from naive_query_engine_amd import capi

    c = capi.Context(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def scan_chunk() -> int:
    src = open(os.path.join(ROOT, "naive_query_engine_amd", "csrc", "sort.hip")).read()
    return int(re.search(r"constexpr int SCAN_CHUNK = (\d+);", src).group(1))


@functools.lru_cache(maxsize=None)
def groups():
    return cu.all_cases(scan_chunk())


def assert_columns_identical(got, exp, what):
    assert len(got) == len(exp), f"{what}: {len(got)} columns, expected {len(exp)}"
    for i, (g, e) in enumerate(zip(got, exp)):
        w = f"{what}: column {i}"
        assert g.dtype == e.dtype, f"{w}: dtype {g.dtype.name}, expected {e.dtype.name}"
        assert g.length == e.length, f"{w}: {g.length} rows, expected {e.length}"
        gm, em = g.valid_mask(), e.valid_mask()
        assert np.array_equal(gm, em), f"{w}: validity differs at rows {np.nonzero(gm != em)[0][:8]}"
        if em.all():
            assert g.validity is None, f"{w}: a validity buffer although no row is NULL"
        if g.length == 0:
            continue
        if g.dtype == DType.UTF8:
            go, eo = np.asarray(g.values[: g.length + 1]), np.asarray(e.values[: e.length + 1])
            assert np.array_equal(go, eo), f"{w}: Utf8 offsets differ first at row {np.nonzero(go != eo)[0][:1]}"
            total = int(eo[-1]) if eo.size else 0
            gd = g.data[:total] if g.data is not None else np.zeros(0, np.uint8)
            ed = e.data[:total] if e.data is not None else np.zeros(0, np.uint8)
            assert np.array_equal(gd, ed), f"{w}: Utf8 bytes differ first at byte {np.nonzero(gd != ed)[0][:1]}"
        elif g.dtype == DType.BOOLEAN:
            gv, ev = g.to_numpy()[em], e.to_numpy()[em]
            assert np.array_equal(gv, ev), f"{w}: Boolean values differ at {np.nonzero(gv != ev)[0][:8]}"
        else:
            gv, ev = g.to_numpy()[em].view(np.uint64), e.to_numpy()[em].view(np.uint64)   # Float64 as bit patterns
            assert np.array_equal(gv, ev), f"{w}: values differ at {np.nonzero(gv != ev)[0][:8]}"


def opts(kw):
    return kw.get("has_header", True), kw.get("delimiter", ","), kw.get("max_read_records", 3), kw.get("batch_size", 1_000_000)


def read_both(ctx, label, data, kw):
    """→ (dtypes, host columns) of the device reader after they equalled the oracle's, or None when both fail alike"""
    has_header, delim, sample, batch = opts(kw)
    try:
        names, nullable, exp = orc.csv_read(data, **kw)
    except ErrorCode as want:
        with pytest.raises(ErrorCode) as got:
            _, dts, _ = ctx.csv_infer_schema(data, has_header, delim, sample, batch)
            ctx.csv_read(data, dts, has_header, delim, batch)
        assert got.value.status == want.status, f"{label}: {got.value} where the oracle says {want}"
        return None
    gn, gd, gnull = ctx.csv_infer_schema(data, has_header, delim, sample, batch)
    assert gn == names, f"{label}: names {gn}, expected {names}"
    assert gd == [c.dtype for c in exp], f"{label}: dtypes {gd}"
    assert gnull == nullable, f"{label}: nullable {gnull}, expected {nullable}"
    got = ctx.csv_read(data, gd, has_header, delim, batch).to_host()
    assert_columns_identical(got, exp, label)
    return gd, got


@pytest.mark.parametrize("group", cu.GROUPS)
def test_every_case_matches_the_oracle(ctx, group):
    cases = groups()[group]
    assert cases
    if group.startswith("carry"):
        assert sum(len(groups()[g]) for g in cu.GROUPS if g.startswith("carry")) <= cu.MAX_BIG_FILES
    for label, data, kw in cases:
        read_both(ctx, label, data, kw)


def test_a_boolean_column_without_null_has_no_validity_buffer_and_all_empty_strings_no_bytes(ctx):
    label, data, kw = next(c for c in groups()["rows"] if c[0].startswith("rows=257 "))
    dts, got = read_both(ctx, label, data, kw)
    names = data.split(b"\n", 1)[0].split(b",")
    nb, e, w = got[names.index(b"nb")], got[names.index(b"e")], got[names.index(b"w")]
    assert nb.dtype == DType.BOOLEAN and nb.validity is None
    assert e.dtype == DType.UTF8 and (e.data is None or e.data.size == 0) and not np.asarray(e.values).any()
    assert w.dtype == DType.INT64 and np.nonzero(~w.valid_mask())[0].tolist() == [63]   # the last bit of a word is the only NULL


def test_more_columns_than_the_limit_is_an_invalid_argument(ctx):
    data = cu.too_many_columns_case()
    _, dts, _ = ctx.csv_infer_schema(data)
    assert len(dts) == cu.MAX_COLS + 1
    with pytest.raises(ErrorCode) as e:
        ctx.csv_read(data, dts)
    assert e.value.status == Status.InvalidArgument


# ----------------------------------------------------------------------------- the image already on the device
def device_cases():
    g = groups()
    out = [g[f"slide_{edge}"][0] for edge in cu.SLIDE_EDGES[:-1]] + [g["carry_slide"][0]]
    return out + [c for c in g["eof"] if len(c[1]) < 200]


def test_device_resident_image_equals_the_host_image_and_nothing_is_read_past_its_end(ctx):
    """device_ptr= / nbytes=: the holder buffer goes on after nbytes with quotes and newlines (up to the next multiple of 8, and
    eight bytes more); a kernel that read one byte too many would see another record or an open quote"""
    ran = 0
    for label, data, kw in device_cases():
        host = read_both(ctx, label, data, kw)
        if host is None:
            continue                                    # (the two one-byte files that are no table)
        dts, exp = host
        has_header, delim, _, batch = opts(kw)
        tail = (-len(data)) % 8 + 8
        padded = data + (b'"\n' * 8)[:tail]
        assert len(padded) % 8 == 0 and len(padded) >= len(data) + 8
        holder = ctx.table_from_host([Column.from_numpy(np.frombuffer(padded, dtype=np.uint64).copy())])
        t = ctx.csv_read(None, dts, has_header, delim, batch, device_ptr=int(holder.column_info(0).values), nbytes=len(data))
        assert_columns_identical(t.to_host(), exp, f"device-resident image, {label}")
        ran += 1
    assert ran >= len(cu.SLIDE_EDGES) + 30


# ----------------------------------------------------------------------------- errors: which record the message names
ROWS = 600                                              # three workgroups of csv_fields_kernel
DTYPES = [DType.INT64, DType.UTF8, DType.FLOAT64]
BAD_INT, BAD_FLOAT, SHORT = "bad_int", "bad_float", "short"


def error_table(faults: dict, has_header=True, rows=ROWS) -> bytes:
    """rows of i Int64, u Utf8, f Float64; faults: {data row: BAD_INT | BAD_FLOAT | SHORT}"""
    lines = [b"i,u,f"] if has_header else []
    for r in range(rows):
        i, u, f = b"%d" % (r * 7 - 1000), b"w%d" % r, b"%d.5" % r
        kind = faults.get(r)
        if kind == BAD_INT:
            i = b"12x"
        if kind == BAD_FLOAT:
            f = b"1.5.5"
        lines.append(b",".join((i, u) if kind == SHORT else (i, u, f)))
    return b"\n".join(lines) + b"\n"


def read_error(ctx, data, has_header=True, batch_size=1_000_000, against_oracle=True):
    """the device reader's error with the schema given (inference would look at the first rows); the status also against the oracle
    wherever its own inference does not see the fault"""
    with pytest.raises(ErrorCode) as e:
        ctx.csv_read(data, DTYPES, has_header, ",", batch_size)
    assert e.value.status == Status.ArrowError
    if against_oracle:
        with pytest.raises(ErrorCode) as o:
            orc.csv_read(data, has_header=has_header, batch_size=batch_size)
        assert o.value.status == e.value.status
    return e.value.message


def names_record(message: str, kind: str, row: int, has_header=True):
    number = row + (1 if has_header else 0) + 1
    if kind == SHORT:
        assert re.search(rf"record {number} has a different number of fields", message), (message, number)
    else:
        assert re.search(rf"parsing a value at line {number}$", message), (message, number)


R0, R1, R2 = 100, 300, 520                              # one row in each workgroup of csv_fields_kernel
assert R0 // cu.FIELD_BLOCK == 0 and R1 // cu.FIELD_BLOCK == 1 and R2 // cu.FIELD_BLOCK == 2


@pytest.mark.parametrize("first,second", [(R0, R1), (R1, R2), (R0, R2)])
@pytest.mark.parametrize("kinds", [(BAD_INT, BAD_FLOAT), (BAD_FLOAT, BAD_INT)])
def test_two_unparsable_values_name_the_first(ctx, first, second, kinds):
    names_record(read_error(ctx, error_table({first: kinds[0], second: kinds[1]})), kinds[0], first)


@pytest.mark.parametrize("bad,short", [(R0, R1), (R1, R2), (R1, R0), (R2, R0)])
def test_a_short_row_is_named_by_its_own_number_whatever_else_fails_to_parse(ctx, bad, short):
    """the field-count message is the one the host prints first; it must carry the first record with THAT fault, also when a
    value fails to parse in an earlier record (one shared first-bad-row cell named the earlier one)"""
    names_record(read_error(ctx, error_table({bad: BAD_INT, short: SHORT})), SHORT, short)


def test_two_short_rows_name_the_first(ctx):
    names_record(read_error(ctx, error_table({R1: SHORT, R2: SHORT, R0: BAD_FLOAT})), SHORT, R1)


@pytest.mark.parametrize("kind", [BAD_INT, BAD_FLOAT, SHORT])
def test_a_fault_on_the_first_row_without_header_and_on_the_last_row(ctx, kind):
    # without a header the oracle infers its schema from the faulty row itself (a short first row is still an error for it)
    names_record(read_error(ctx, error_table({0: kind}, has_header=False), has_header=False, against_oracle=kind == SHORT), kind, 0, has_header=False)
    names_record(read_error(ctx, error_table({ROWS - 1: kind})), kind, ROWS - 1)
    names_record(read_error(ctx, error_table({ROWS - 1: kind}, has_header=False), has_header=False), kind, ROWS - 1, has_header=False)


@pytest.mark.parametrize("k", [1, cu.FIELD_BLOCK, cu.FIELD_BLOCK + 1])
def test_only_the_rows_of_the_first_batch_can_fail(ctx, k):
    for kind in (BAD_INT, SHORT):
        outside = error_table({k: kind})                # the first row that is not read
        t = ctx.csv_read(outside, DTYPES, True, ",", k)
        got = t.to_host()
        assert [c.length for c in got] == [k] * 3
        if k >= 3:                                      # (the oracle's inference reads three rows whatever the batch size)
            assert_columns_identical(got, orc.csv_read(outside, batch_size=k)[2], f"batch_size={k}, {kind} in row {k}")
        else:
            assert got[0].to_list() == [r * 7 - 1000 for r in range(k)] and got[1].to_list() == [f"w{r}" for r in range(k)]
        names_record(read_error(ctx, error_table({k - 1: kind}), batch_size=k, against_oracle=k - 1 >= 3 or kind == SHORT), kind, k - 1)
