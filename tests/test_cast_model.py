"""The Python model of tests/cast_util.py (quirk Q29) against pyarrow.compute.cast, on the CPU.  pyarrow has no NULL-on-failure cast: it
raises where this library's cast gives NULL.  So every row the model calls valid and pyarrow's grammar takes (cast_util's ARROW_ROWS)
goes through pyarrow and must agree bit for bit — checked integer / float options, with only allow_float_truncate set so that 1.5 -> 1
and 2^53+1 -> 2^53 are answers and not errors — and every other row is cast_util's HAND_ROWS, (input, expected) written by hand: the
expected NULLs, and the integer strings with a leading `+` (pyarrow's integer grammar is [-]digits; this library's is the CSV reader's
[+-]digits, as include/nqe.h states).

The share of rows checked only by the hand-written table is printed by test_the_share_of_rows_that_go_through_pyarrow (run with -s) and
was 93 of 684 rows (14 %) over all pairs when this was written, at most 29 % of one pair (Utf8 -> Int64 / UInt64); no pair, and no prefix
of a pair's rows, may be above 50 %, which the same test asserts."""
import numpy as np
import pyarrow as pa
import pyarrow.compute as pc
import pytest

from tests import cast_util as cu
from tests.cast_util import PAIRS, Val

PA = {"i64": pa.int64(), "u64": pa.uint64(), "f64": pa.float64(), "bool": pa.bool_(), "utf8": pa.binary()}

PYARROW_TAKES = {("utf8", "bool"): (b"1", b"0"), ("utf8", "i64"): (b"0x10",)}  # 1 / 0 as Booleans, hexadecimal integers: NULL here (include/nqe.h)


def arrow_cast(frm, to, values):
    target = pa.string() if to == "utf8" else PA[to]  # (pyarrow formats numbers as string, not binary)
    out = pc.cast(pa.array(values, type=PA[frm]), options=pc.CastOptions(target_type=target, allow_float_truncate=True)).to_pylist()
    return [x.encode() if to == "utf8" else x for x in out]


def same_value(kind, a, b):
    if kind == "f64":
        return (a != a and b != b) or (a == b and np.signbit(a) == np.signbit(b))
    return a == b and type(a) is type(b)


@pytest.mark.parametrize("frm,to", PAIRS)
def test_the_model_agrees_with_pyarrow_on_every_row_it_calls_valid(frm, to):
    rows = cu.arrow_rows(frm, to)
    expected = [cu.cast_one(frm, to, v) for v in rows]
    assert all(x is not None for x in expected), [v for v, x in zip(rows, expected) if x is None][:5]
    got = arrow_cast(frm, to, rows)
    bad = [(v, x, g) for v, x, g in zip(rows, expected, got) if not same_value(to, x, g)]
    assert not bad, bad[:5]
    # row by row as well: no row's answer depends on its neighbours
    assert all(same_value(to, x, arrow_cast(frm, to, [v])[0]) for v, x in list(zip(rows, expected))[:8])


@pytest.mark.parametrize("frm,to", sorted(cu.HAND_ROWS))
def test_the_model_gives_the_hand_written_answers(frm, to):
    for v, want in cu.HAND_ROWS[(frm, to)]:
        got = cu.cast_one(frm, to, v)
        assert (got is None) == (want is None) and (want is None or same_value(to, got, want)), (v, got, want)
        if want is None:  # pyarrow has no answer here: it raises (PYARROW_TAKES: the three strings its grammar takes and this library's does not)
            try:
                theirs = pc.cast(pa.array([v], type=PA[frm]), PA[to]).to_pylist()[0]
            except (pa.ArrowInvalid, pa.ArrowNotImplementedError):
                theirs = None
            assert theirs is None or v in PYARROW_TAKES.get((frm, to), ()), (v, theirs)


def test_only_the_fallible_pairs_have_expected_nulls():
    assert sorted(cu.HAND_ROWS) == sorted(p for p in PAIRS if cu.fallible(*p))
    for frm, to in cu.HAND_ROWS:
        assert any(x is None for _, x in cu.HAND_ROWS[(frm, to)])
    for frm in cu.KINDS:
        for to in cu.KINDS:
            expect = frm != to and (frm == "utf8" or {frm, to} == {"i64", "u64"} or (frm == "f64" and to in ("i64", "u64")))
            assert cu.fallible(frm, to) == expect


def test_the_share_of_rows_that_go_through_pyarrow():
    hand_total = rows_total = 0
    for frm, to in PAIRS:
        rows = cu.pair_rows(frm, to)
        hand = sum(1 for r in rows if not r[2])
        print(f"{frm:>4} -> {to:<4}: {len(rows):3d} rows, {hand:2d} by the hand-written table ({100 * hand / len(rows):.0f} %)")
        assert 2 * hand <= len(rows), (frm, to)
        for k in range(2, len(rows) + 1):  # and of every prefix: a short GPU column keeps the property
            assert 2 * sum(1 for r in rows[:k] if not r[2]) <= k, (frm, to, k)
        hand_total, rows_total = hand_total + hand, rows_total + len(rows)
    print(f"all pairs: {hand_total} of {rows_total} rows by the hand-written table ({100 * hand_total / rows_total:.0f} %)")
    assert 2 * hand_total <= rows_total


@pytest.mark.parametrize("frm,to", PAIRS)
def test_no_pair_has_a_constant_expected_column(frm, to):
    for nullable in (False, True):
        col = cu.pair_column(frm, to, 64, nullable)
        expected = cu.cast(col, to)
        cu.guard(frm, to, expected)
        assert expected.nullable == (cu.fallible(frm, to) or nullable)
        assert all(expected.values[i] == cu.zero_of(to) for i in range(64) if not expected.valid[i])  # zeros under a NULL
        assert not (expected.valid & ~col.valid).any()  # a NULL operand row is a NULL result row
    for n in (63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4096):  # the row counts of tests/test_gpu_cast.py that the guard covers
        for nullable in (False, True):
            cu.guard(frm, to, cu.cast(cu.pair_column(frm, to, n, nullable), to))
    rows = cu.pair_rows(frm, to)
    assert [cu.cast_one(frm, to, v) for v, _, _ in rows] == [x for _, x, _ in rows] or to == "f64"  # (NaN != NaN)


def test_the_same_dtype_cast_is_the_operand():
    for kind in cu.KINDS:
        v = Val(kind, [cu.zero_of(kind)] * 3, [True, False, True])
        assert cu.cast(v, kind) is v
