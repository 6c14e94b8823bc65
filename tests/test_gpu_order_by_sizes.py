"""ORDER BY on the device at the row counts where code starts to run that no smaller table reaches (csrc/order_by.hip over sort.hip).

  rows       what starts there
  262 144    the last row count at which the radix sort scans its tile counts (128 tiles of 2048 keys x 256 buckets = 8 chunks of 4096,
             in place) in ONE workgroup: label scan_single
  262 145    9 chunks: scan_chunk, the scan of the chunk sums, scan_add — per digit pass; and ob_max_len's grid, capped at num_cus * 4
             workgroups of 256, strides a second time on 256 CUs
  524 289    the grids of ob_encode / ob_encode_gather and ob_positions are capped at num_cus * 8 workgroups of 256 rows: a second trip
             of their stride loops on 256 CUs
  1 048 577  the same on any device of up to 512 CUs (the cap depends on the CU count, so no test asserts that a second trip was made)
The two label assertions at 262 144 / 262 145 pin the scan's threshold from the outside: if sort.hip's RT_TILE or SCAN_CHUNK changes they
fail, and the row counts here and in tests/test_gpu_window_sizes.py have to move with the constants.

The yardstick is order_by_util.sort_indices_np, the np.lexsort form of the model (tests/test_large_models_host.py holds it against the
row-at-a-time model), followed by the model's take; the comparison is value for value, Float64 bit for bit.  Every table carries its row
numbers, so stability shows."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import order_by_util as obu  # noqa: E402
from naive_query_engine_amd import Column, DType  # noqa: E402

pytestmark = pytest.mark.gpu
I64 = np.iinfo(np.int64)
SINGLE_MAX = 262_144  # the scan of the tile counts is one workgroup's up to here
SIZES = [SINGLE_MAX, SINGLE_MAX + 1, 524_289, 1_048_577]


@pytest.fixture(scope="module")
def ctx():
    from naive_query_engine_amd import capi

    return capi.default_context()


class Launches:
    """the kernel launches of the context while the block runs"""

    def __init__(self, ctx):
        self.ctx = ctx

    def __enter__(self):
        self.ctx.timing_enable(True)
        self.ctx.timing_reset()
        return self

    def count(self, name=""):
        return self.ctx.timing_query(name)[1]

    def __exit__(self, *exc):
        self.ctx.timing_enable(False)
        self.ctx.timing_reset()


def rownum(n):
    return Column.from_numpy(np.arange(n, dtype=np.int64))


def check(ctx, table, cols, keys, fetch=None, what=""):
    """device against the vectorised model; returns the device's columns and the launch counts of the sort's labels"""
    with Launches(ctx) as L:
        got = ctx.order_by(table, keys, fetch).to_host()
        counts = {s: L.count(s) for s in ("radix_scatter", "scan_single", "scan_chunk", "scan_add", "ob_encode_gather", "ob_max_len", "ob_positions")}
    obu.assert_same_rows(got, obu.take(cols, obu.sort_indices_np(cols, keys, fetch)), what=f"{what} keys {keys} fetch {fetch}")
    return got, counts


def assert_scan_form(n, counts, passes, what):
    """the digit passes that ran, and which form of the scan each of them took"""
    assert counts["radix_scatter"] == passes, (what, counts)
    if n <= SINGLE_MAX:
        assert (counts["scan_single"], counts["scan_chunk"], counts["scan_add"]) == (passes, 0, 0), (what, counts)
    else:
        # per pass: scan_chunk over the counts, scan_chunk again over the (single chunk of) chunk sums, scan_add
        assert (counts["scan_single"], counts["scan_chunk"], counts["scan_add"]) == (0, 2 * passes, passes), (what, counts)


# ----------------------------------------------------------------------------- digit passes: eight, one, three
@pytest.mark.parametrize("n", SIZES)
def test_int64_keys_of_eight_one_and_three_digit_passes(ctx, n):
    rng = np.random.default_rng(n)
    full = rng.integers(I64.min, I64.max, n, dtype=np.int64, endpoint=True)
    full[[0, 1, n // 2, n - 1]] = [I64.max, I64.min, I64.min, I64.max]
    cols = [Column.from_numpy(full), Column.from_numpy(rng.integers(0, 256, n).astype(np.int64)), Column.from_numpy(rng.integers(0, 2 ** 24, n).astype(np.int64)), rownum(n)]
    table = ctx.table_from_host(cols)
    for k, passes in ((0, 8), (1, 1), (2, 3)):  # an even count of ping-pong passes; one pass and no temporary buffers; an odd count
        for desc in (False, True):
            _, counts = check(ctx, table, cols, [(k, desc)], what=f"n={n}")
            assert_scan_form(n, counts, passes, f"n={n} column {k} desc={desc}")
            assert counts["ob_encode_gather"] == 0 and counts["ob_positions"] == 1


# ----------------------------------------------------------------------------- NULLs: the flag pass reads through the permutation
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("descending", [False, True])
@pytest.mark.parametrize("nulls_first", [False, True])
def test_nullable_full_range_int64_in_all_four_placements(ctx, n, descending, nulls_first):
    rng = np.random.default_rng(n + 1)
    mask = rng.random(n) > 0.1
    mask[:66] = True  # the first NULLs in input order are the planted ones, at a bitmap word's edges
    mask[[0, 63, 64, 65, n - 1]] = False
    full = rng.integers(I64.min, I64.max, n, dtype=np.int64, endpoint=True)  # no spare bit for the flag
    full[[1, 2]] = [I64.min, I64.max]
    cols = [Column.from_numpy(full, mask), rownum(n)]
    got, counts = check(ctx, ctx.table_from_host(cols), cols, [(0, descending, nulls_first)], what=f"n={n}")
    assert_scan_form(n, counts, 9, f"n={n}")  # eight value passes and the flag's one
    assert counts["ob_encode_gather"] == 1
    nulls = int((~mask).sum())
    r = got[1].to_numpy()
    r = r[:nulls] if nulls_first else r[n - nulls:]
    assert r[:4].tolist() == [0, 63, 64, 65] and r[-1] == n - 1 and (np.diff(r) > 0).all()  # NULLs tie among themselves: input order


@pytest.mark.parametrize("n", SIZES)
def test_nullable_float64_special_values_and_normals(ctx, n):
    rng = np.random.default_rng(n + 2)
    cols = [obu.random_column(rng, DType.FLOAT64, n, True), rownum(n)]
    table = ctx.table_from_host(cols)
    for desc, nf in ((False, True), (True, False), (True, True)):
        got, counts = check(ctx, table, cols, [(0, desc, nf)], what=f"n={n}")
        assert counts["ob_encode_gather"] == 1 and counts["scan_add"] == (0 if n <= SINGLE_MAX else counts["radix_scatter"])
        valid = got[0].to_numpy()[got[0].valid_mask()]
        assert np.isnan(valid[0 if desc else -1])  # NaN is greater than +inf


@pytest.mark.parametrize("n", SIZES)
def test_two_distinct_values_keep_the_input_order_inside_each(ctx, n):
    k = (np.random.default_rng(n + 3).random(n) < 0.5).astype(np.int64) * 7 - 3
    cols = [Column.from_numpy(k), rownum(n)]
    table = ctx.table_from_host(cols)
    for desc in (False, True):
        got, counts = check(ctx, table, cols, [(0, desc)], what=f"n={n}")
        assert counts["radix_scatter"] == 8  # -3 and 4 differ in every byte
        r, first = got[1].to_numpy(), int((k == (4 if desc else -3)).sum())
        assert (np.diff(r[:first]) > 0).all() and (np.diff(r[first:]) > 0).all()


# ----------------------------------------------------------------------------- three keys, Utf8 first
def test_three_keys_utf8_descending_float64_boolean(ctx):
    n = SINGLE_MAX + 1
    rng = np.random.default_rng(5)
    words = [w for w in obu.WORDS if b"\0" not in w and len(w) <= 17]
    assert max(len(w) for w in words) == 17  # three 8-byte chunk passes and the length's
    pick, ok = rng.integers(0, len(words), n).tolist(), (rng.random(n) > 0.2).tolist()
    cols = [obu.utf8_column([words[p] if o else None for p, o in zip(pick, ok)], null_bytes=b"zz"), obu.random_column(rng, DType.FLOAT64, n, True, 5),
            obu.random_column(rng, DType.BOOLEAN, n, False), rownum(n)]
    table = ctx.table_from_host(cols)
    _, counts = check(ctx, table, cols, [(0, True, False), (1, False, True), (2, False, True)], what="Utf8 desc, Float64, Boolean")
    assert counts["ob_max_len"] == 1 and counts["ob_encode_gather"] == 7  # behind Boolean's pass: Float64 and its flag, the length, 3 chunks, the flag
    assert counts["scan_add"] > 0
    check(ctx, table, cols, [(2, True), (1, True, False), 0], what="Boolean desc, Float64 desc, Utf8")


# ----------------------------------------------------------------------------- fetch
@pytest.mark.parametrize("fetch", [1, 524_288, 524_294])
def test_fetch_past_the_grid_cap_of_the_positions(ctx, fetch):
    n = 524_289
    rng = np.random.default_rng(41)
    cols = [obu.random_column(rng, DType.INT64, n, True, 17), Column.from_numpy(rng.normal(0, 1, n), rng.random(n) > 0.5), rownum(n)]
    table = ctx.table_from_host(cols)
    m = min(fetch, n)
    with Launches(ctx) as L:
        got = ctx.order_by(table, [(0, True, False)], fetch).to_host()
        assert L.count("ob_positions") == 1 and L.count(f"ob_positions:{m}") == 1  # the takes' row list holds min(fetch, n) rows
    assert got[0].length == m
    obu.assert_same_rows(got, obu.take(cols, obu.sort_indices_np(cols, [(0, True, False)], fetch)), what=f"fetch {fetch}")
