"""The vectorised models of the large-table GPU tests against the row-at-a-time models they stand in for (no device, no library call).

order_by_util.sort_indices_np (one stable np.lexsort) must give the list of order_by_util.sort_indices; window_util.window_np (cumulative
sums and running extremes over whole arrays) must give the columns of window_util.window under the comparator's own same_mask with bound
0: on window_np's domain — integers below 2^20 — every sum is exact in both.  The window cases are the partition layouts of
tests/test_gpu_window_sizes.py, scaled down to a tile of 4 rows and a carry chunk of 16, and once at the real constants."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import order_by_util as obu  # noqa: E402
import window_util as wu  # noqa: E402
from naive_query_engine_amd import Column, DType, WindowFrame as F, WindowFunc as W  # noqa: E402

I64 = np.iinfo(np.int64)
POOL = np.concatenate([obu.SPECIAL_F64.view(np.uint64), obu.NAN_BITS]).view(np.float64)
SIZES = [0, 1, 2, 257, 5000]
FETCHES = lambda n: [None, 0, 3, n, n + 1]


def rownum(n):
    return Column.from_numpy(np.arange(n, dtype=np.int64))


def same_order(cols, keys, fetches=(None,), what=""):
    for fetch in fetches:
        got = obu.sort_indices_np(cols, keys, fetch)
        assert got.dtype == np.int64
        assert got.tolist() == obu.sort_indices(cols, keys, fetch), f"{what} keys {keys} fetch {fetch}"


# ----------------------------------------------------------------------------- sort
def _without_nul(col):
    """a Utf8 column with every NUL byte replaced (sort_indices_np refuses them); everything else as it is"""
    if col.dtype != DType.UTF8:
        return col
    return obu.utf8_column([None if s is None else s.replace(b"\0", b"\x01") for s in obu.column_values(col)], null_bytes=b"zz")


@pytest.mark.parametrize("seed", range(30))
def test_sort_the_sweeps_seeded_tables(seed):
    cols, keys = obu.random_table(seed)
    cols = [_without_nul(c) for c in cols]
    n = cols[0].length
    same_order(cols, keys, FETCHES(n), what=f"seed {seed} n={n}")


@pytest.mark.parametrize("n", SIZES)
def test_sort_directed_cases(n):
    rng = np.random.default_rng(n)
    mask = rng.random(n) > 0.2
    full = rng.integers(I64.min, I64.max, n, dtype=np.int64, endpoint=True)
    if n >= 2:
        full[[0, n - 1]] = [I64.min, I64.max]
    two = (rng.random(n) < 0.5).astype(np.int64) * 7 - 3
    special = POOL[rng.integers(0, POOL.size, n)].copy()
    words = [w for w in obu.WORDS if b"\0" not in w]
    strs = [words[i] for i in rng.integers(0, len(words), n)]
    cols = [Column.from_numpy(np.full(n, 5, dtype=np.int64)), Column.from_numpy(two), Column.from_numpy(full, mask), Column.from_numpy(special),
            Column.from_numpy(special.copy(), mask), Column.from_numpy(rng.integers(0, 2 ** 64, n, dtype=np.uint64), mask), Column.from_numpy(two > 0, mask),
            obu.utf8_column([s if ok else None for s, ok in zip(strs, mask)], null_bytes=b"hidden"), obu.utf8_column(strs), rownum(n)]
    for k in range(len(cols) - 1):
        for desc in (False, True):
            for nf in (False, True):  # all keys equal, two values, the full range, the special pool, every dtype: all four placements
                same_order(cols, [(k, desc, nf)], FETCHES(n), what=f"n={n} column {k}")
    same_order(cols, [(1, True), (4, False, False), (7, True, True)], FETCHES(n), what=f"n={n} three keys")
    same_order(cols, [0, (6, True, False), (3, True)], FETCHES(n), what=f"n={n} a constant key first")
    if n == 0:
        same_order(cols, [], what="no rows, no keys")


def test_sort_np_strings_order_as_memcmp_and_nul_bytes_are_refused():
    col = obu.utf8_column([b"b", b"ab", "ÿz".encode(), b"a", b"", b"\x7f", "é".encode(), b"abcdefghijklmnopq", b"abcdefghijklmnop", None])
    assert obu.sort_indices_np([col], [0]).tolist() == [9, 4, 3, 1, 8, 7, 0, 5, 6, 2]  # NULL first, then bytes as UNSIGNED: 0x7f < 0xc3
    assert obu.sort_indices_np([col], [(0, True, False)]).tolist() == [2, 6, 5, 0, 7, 8, 1, 3, 4, 9]  # descending: the longer string first
    with pytest.raises(ValueError):
        obu.sort_indices_np([obu.utf8_column([b"a", b"a\0"])], [0])
    assert obu.sort_indices_np([obu.utf8_column([None, b"x"], null_bytes=b"\0\0")], [0]).tolist() == [0, 1]  # the bytes under a NULL are not looked at


# ----------------------------------------------------------------------------- window
EVERYTHING = [(W.RowNumber,), (W.Rank,), (W.DenseRank,)] + [(f, c, fr) for c in (2, 3) for fr in wu.FRAMES for f in wu.AGGREGATES]
WINDOW_SIZES = [0, 1, 2, 5, 257, 3000]
SCALES = [(4, 16, 3, 9), (4096, 256 * 4096, 5000, 10_000)]  # (tile, chunk, inside, longest): scaled down, and the real constants


def assert_same_window(cols, parts, order, funcs, what, **variant):
    """window_np against window, column for column, under the comparator's mask with bound 0; returns whether they agree"""
    fast, slow = wu.window_np(cols, parts, order, funcs, **variant), wu.window(cols, parts, order, funcs)
    assert fast.funcs == slow.funcs
    zero = np.zeros(cols[0].length if cols else 0)
    agree = True
    for i, (fn, c, frame) in enumerate(fast.funcs):
        g, e = fast.cols[i], slow.cols[i]
        assert g.dtype == e.dtype and g.shape == e.shape, f"{what}: function {i} is {g.dtype}{g.shape}, the row model's {e.dtype}{e.shape}"
        same = wu.same_mask(fn, g, e, zero)
        if not same.all():
            if not variant:
                bad = np.nonzero(~same)[0][:4]
                raise AssertionError(f"{what}: {fn.name} column {c} {frame.name}: rows {bad}: {g[bad]} vs {e[bad]}")
            agree = False
        if fn == W.Sum:
            assert (fast.tols[i] == 0).all()  # derived: integers below 2^53 add exactly in every order
        elif fn == W.Avg:
            with np.errstate(invalid="ignore"):
                assert (fast.tols[i] == np.where(np.isfinite(g), np.spacing(np.abs(np.where(np.isfinite(g), g, 0.0))), 0.0)).all()  # one ulp of the quotient
        else:
            assert fast.tols[i] is None
    return agree


def _shuffled(cols, seed):
    n = cols[0].length
    return obu.take(cols, np.random.default_rng(seed).permutation(n)) if n else cols


@pytest.mark.parametrize("scale", SCALES, ids=["scaled_down", "real_constants"])
@pytest.mark.parametrize("layout", wu.LAYOUTS)
@pytest.mark.parametrize("n", WINDOW_SIZES)
def test_window_layouts(n, layout, scale):
    tile, chunk, inside, longest = scale
    for peers, poisoned in ((False, 0), (True, 1), (True, None)):  # the poisoned partition: the first, the second, none
        rng = np.random.default_rng(n * 7 + wu.LAYOUTS.index(layout))
        lengths = wu.layout_lengths(layout, n, tile, chunk, rng, inside, longest)
        cols, parts, order = wu.layout_table(lengths, rng, peers, poisoned)
        cols = _shuffled(cols, 3)
        assert_same_window(cols, parts, order, EVERYTHING, f"n={n} {layout} tile {tile} peers {peers} poisoned {poisoned}")
        if layout == "one_partition":
            assert_same_window(cols, [], order, EVERYTHING, f"n={n} no partition key")


@pytest.mark.parametrize("n", WINDOW_SIZES)
def test_window_keys_of_every_type_with_nulls_and_nullable_float_values(n):
    rng = np.random.default_rng(n + 40)
    v = rng.integers(-9, 9, n).astype(np.float64)
    if n:
        v[rng.integers(0, n, n // 5)] = POOL[[2, 3, 11]][rng.integers(0, 3, n // 5)]  # +inf, -inf, a NaN
    words = [w for w in obu.WORDS if b"\0" not in w][:5]
    cols = [obu.random_column(rng, DType.INT64, n, True, 5), obu.random_column(rng, DType.FLOAT64, n, True, 5), obu.random_column(rng, DType.BOOLEAN, n, True),
            obu.utf8_column([words[i] if ok else None for i, ok in zip(rng.integers(0, 5, n), rng.random(n) > 0.2)]), Column.from_numpy(v, rng.random(n) > 0.3),
            Column.from_numpy(rng.integers(0, 2 ** 20, n).astype(np.uint64))]
    funcs = [(W.RowNumber,), (W.Rank,), (W.DenseRank,)] + [(f, c, fr) for c in (4, 5) for fr in wu.FRAMES for f in wu.AGGREGATES]
    for parts, order in (([0], [(1, True, False)]), ([1], [3]), ([2, 3], [(0, False, False), (1, True, True)]), ([], [(3, True), 2]), ([3], []), ([], [])):
        assert_same_window(cols, parts, order, funcs, f"n={n} partition by {parts} order by {order}")


def test_window_np_refuses_values_outside_its_domain():
    key = Column.from_numpy(np.zeros(3, dtype=np.int64))
    for bad in (np.array([1.5, 0.0, 0.0]), np.array([2.0 ** 20, 0.0, 0.0])):
        with pytest.raises(ValueError):
            wu.window_np([key, Column.from_numpy(bad)], [0], [], [(W.Sum, 1, F.Rows)])
    wu.window_np([key, Column.from_numpy(np.array([1.5, np.inf, np.nan]), np.array([False, True, True]))], [0], [], [(W.Sum, 1, F.Rows)])  # under a NULL: anything


def test_witness_a_running_min_without_the_partition_offset_is_told_apart():
    """the comparison can fail: the deliberately wrong window_np — ONE running min / max over the whole sorted order — differs from the
    row model as soon as a later partition's values do not beat an earlier partition's"""
    cols = [Column.from_numpy(np.array([0, 0, 1, 1], dtype=np.int64)), Column.from_numpy(np.arange(4, dtype=np.int64)), Column.from_numpy(np.array([-5, 7, 1, 2], dtype=np.int64))]
    funcs = [(W.Min, 2, F.Rows), (W.Max, 2, F.Rows), (W.Sum, 2, F.Rows), (W.Count, 2, F.Rows)]
    assert assert_same_window(cols, [0], [1], funcs, "witness, the right model")
    assert not assert_same_window(cols, [0], [1], funcs, "witness, the wrong model", _partition_offset=False)
    wrong = wu.window_np(cols, [0], [1], funcs, _partition_offset=False)
    assert wrong.cols[0].tolist() == [-5, -5, -5, -5] and wrong.cols[1].tolist() == [-5, 7, 7, 7]  # partition 1 should give 1, 1 and 1, 2
    assert wu.window(cols, [0], [1], funcs).cols[0].tolist() == [-5, -5, 1, 1]
    # and through the GPU tests' own comparator
    right = wu.window_np(cols, [0], [1], funcs)
    got = [Column.from_numpy(c) for c in right.cols]
    wu.assert_matches_window(got, right)
    with pytest.raises(AssertionError):
        wu.assert_matches_window(got, wrong)


# ----------------------------------------------------------------------------- the layouts do what the GPU tests say they do
def test_the_layouts_put_their_starts_where_the_large_gpu_tests_need_them():
    import re

    plan = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "naive_query_engine_amd", "csrc", "window_plan.hpp")).read()
    T = int(re.search(r"constexpr int64_t WIN_TILE = (\d+);", plan).group(1))
    C = T * int(re.search(r"constexpr int WIN_THREADS = (\d+);", plan).group(1))
    n = 2 * C + T + 1  # three carry chunks; the last tile holds one row
    starts = lambda name: np.concatenate([[0], np.cumsum(wu.layout_lengths(name, n, T, C, np.random.default_rng(0)))[:-1]])
    assert starts("one_partition").tolist() == [0]
    assert starts("tile_edges").tolist() == [0, C - 1, C]  # the last row of the first chunk's last tile, the first row of the tile behind it
    s = starts("flagless_chunk")
    assert s[1] == C - 5000 and not ((s >= C) & (s < 2 * C)).any() and (s >= 2 * C).sum() >= 2 and s[-1] < n - 1  # no start in the middle chunk;
    assert (starts("every_row_its_own") == np.arange(n)).all()                                                     # the last partition crosses into the last tile
    assert np.diff(starts("random_lengths")).max() <= 10_000 and len(starts("random_lengths")) > n // 10_000
    for name in wu.LAYOUTS:  # at every size of the GPU tests the lengths cover the table exactly
        for rows in (262_145, C, C + 1, n):
            assert sum(wu.layout_lengths(name, rows, T, C, np.random.default_rng(1))) == rows
    assert starts("tile_edges")[1] == C - 1 and wu.layout_lengths("tile_edges", C, T, C) == [C - 1, 1]  # exactly one chunk: the start on its last row
