"""Window functions on the device past the first trip of every loop that only the row count reaches (csrc/window_kernels.hpp, sort.hip).

  rows                       what starts there
  262 145                    the window's sort: the radix sort's in-place scan of its tile counts leaves the one-workgroup scan for
                             scan_chunk + scan_add (sort.hip: scan_impl; tests/test_gpu_order_by_sizes.py pins that threshold)
  THREADS * T = C            exactly THREADS tiles: the last row count at which the one-workgroup carry scans make ONE trip
  C + 1                      win_pos_carry and win_scan_carry<OPS> make a second trip: frun / brun / run are no longer the identity, and
                             the backward index spans two chunks.  Also more rows than num_cus * 8 workgroups of 256 cover on any device of
                             up to 512 CUs, so win_bounds, win_gather and win_emit (and the sort's ob_encode_gather) take a second trip of
                             their grid-stride loops — which is not asserted, the cap depends on the device
  2 C + T + 1                three chunks of THREADS, THREADS and 2 carries; the last tile holds one row
T and THREADS are read from csrc/window_plan.hpp, so a changed constant moves the cases with it.

The yardstick at these sizes is window_util.window_np, the vectorised form of the row-at-a-time model (tests/test_large_models_host.py holds
the two against each other).  Its values are integers below 2^20, so every sum is exact whatever the order of the additions: the bound of
sum is 0, that of avg one ulp of the quotient, everything else is equality.

The second half runs every instantiation of the segmented scan (one per non-empty subset of sum / count / min / max) and every function
alone, at 4 T + 8 rows against the row-at-a-time model."""
import itertools
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import agg_value_util as avu  # noqa: E402
import order_by_util as obu  # noqa: E402
import window_util as wu  # noqa: E402
from naive_query_engine_amd import Column, WindowFrame as F, WindowFunc as W  # noqa: E402

pytestmark = pytest.mark.gpu
_PLAN = open(os.path.join(ROOT, "naive_query_engine_amd", "csrc", "window_plan.hpp")).read()
T = int(re.search(r"constexpr int64_t WIN_TILE = (\d+);", _PLAN).group(1))
THREADS = int(re.search(r"constexpr int WIN_THREADS = (\d+);", _PLAN).group(1))
C = T * THREADS             # the rows one trip of the carry scans covers
N_SORT = 262_145            # sort.hip's threshold (see above): not a constant of the window
RANKS = [(W.RowNumber,), (W.Rank,), (W.DenseRank,)]


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


def shuffled(cols, seed):
    return obu.take(cols, np.random.default_rng(seed).permutation(cols[0].length))


# ----------------------------------------------------------------------------- row counts past the carry loops' first trip
# one call takes at most 16 functions: (first function, one past the last, distinct value columns) of each call
FUNCS = RANKS + wu.ALL_AGGS(2, F.Rows) + wu.ALL_AGGS(2, F.Range) + wu.ALL_AGGS(2, F.Partition) + [(f, 3, fr) for fr in (F.Rows, F.Partition) for f in (W.Sum, W.Max, W.Min)]
CALLS = [(0, 13, 1), (13, 24, 2)]
assert len(FUNCS) == 24

# (rows, layout, order key in peer groups of three)
LARGE = [(n, layout, True) for n in (N_SORT, C, C + 1, 2 * C + T + 1) for layout in wu.LAYOUTS[:3]]
LARGE += [(2 * C + T + 1, "one_partition", False), (C + 1, "every_row_its_own", False), (C + 1, "random_lengths", True), (C + 1, "random_lengths", False)]


@pytest.mark.parametrize("n,layout,peers", LARGE, ids=[f"{n}-{layout}-{'peers3' if p else 'distinct'}" for n, layout, p in LARGE])
def test_row_counts_past_the_first_chunk_of_the_carry_scans(ctx, n, layout, peers):
    rng = np.random.default_rng(n % 1000 + len(layout))
    lengths = wu.layout_lengths(layout, n, T, C, rng)
    # the poisoned partition is the first: it lies in the first chunk, the partitions checked behind it in the later ones
    cols, parts, order = wu.layout_table(lengths, rng, peers, poisoned=None if len(lengths) == 1 else 0)
    cols = shuffled(cols, 11)
    model = wu.window_np(cols, parts, order, FUNCS)
    table = ctx.table_from_host(cols)
    for lo, hi, value_cols in CALLS:
        with Launches(ctx) as L:
            got = ctx.window(table, parts, order, FUNCS[lo:hi]).to_host()
            assert L.count("win_pos_carry") == 1 and L.count("win_scan_carry") == value_cols  # ONE workgroup each, however many chunks
            assert L.count("win_pos_reduce") == 1 and L.count("win_scan_reduce") == value_cols and L.count("win_emit") == 1
            assert L.count("radix_scatter") > 0
            if n >= N_SORT:
                assert L.count("scan_chunk") > 0 and L.count("scan_add") > 0  # the sort's chunked scan ran under the window
        wu.assert_matches_window(got, wu.split_model(model, lo, hi), what=f"n={n} {layout} functions {lo}..{hi - 1}")
        if lo and len(lengths) > 1:  # the trap, directly: nothing of the poisoned partition reaches a later one
            later = cols[0].to_numpy() > 0
            for f, g in zip(FUNCS[lo:hi], got):
                if f[1] == 3:
                    assert np.isfinite(g.to_numpy()[later]).all(), f


# ----------------------------------------------------------------------------- every instantiation of the scan, every function alone
# the scan operators a function asks for (csrc/window_plan.hpp: win_ops_of, pinned by tests/cpp/test_window_plan.cpp)
OP_BITS = {W.Sum: 1, W.Count: 2, W.Min: 4, W.Max: 8, W.Avg: 1 | 2}
SUBSETS = [s for k in range(1, 5) for s in itertools.combinations((W.Count, W.Sum, W.Min, W.Max), k)]
# subset i's j-th function takes frame (i + j) mod 3
SUBSET_FUNCS = [[(f, 2, wu.FRAMES[(i + j) % 3]) for j, f in enumerate(s)] for i, s in enumerate(SUBSETS)]
ALONE = RANKS + [(f, 2, fr) for f in wu.AGGREGATES for fr in wu.FRAMES]


def _bits(funcs):
    b = 0
    for f in funcs:
        b |= OP_BITS[f[0]]
    return b


def test_the_subsets_are_the_fifteen_instantiations_and_every_frame_meets_every_function():
    assert sorted(_bits(fs) for fs in SUBSET_FUNCS) == list(range(1, 16))
    assert {(f, fr) for fs in SUBSET_FUNCS for f, _, fr in fs} == {(f, fr) for f in (W.Count, W.Sum, W.Min, W.Max) for fr in wu.FRAMES}


@pytest.fixture(scope="module")
def small_table():
    """4 T + 8 rows in the partitions of test_gpu_window.py's `lengths` layout: starts on a tile's last and first row, and a partition whose
    middle tile has no start; column 2: nullable Float64 with Q10's special values"""
    lengths = [T - 1, 1, 2 * T + 3, T, 5]
    n = sum(lengths)
    rng = np.random.default_rng(77)
    v, mask = avu.gen_values("f64_special", rng, n, True)
    cols = [Column.from_numpy(np.repeat(np.arange(len(lengths), dtype=np.int64), lengths)), Column.from_numpy(np.arange(n, dtype=np.int64) // 3), Column.from_numpy(v, mask)]
    return shuffled(cols, 3)


def _check_small(ctx, cols, funcs, what):
    model = wu.window(cols, [0], [1], funcs)
    with Launches(ctx) as L:
        got = ctx.window(ctx.table_from_host(cols), [0], [1], funcs).to_host()
        counts = {s: L.count(s) for s in ("win_gather", "win_scan_reduce", "win_scan_carry", "win_scan_apply", "win_pos_reduce", "win_pos_carry", "win_pos_apply", "win_emit")}
    wu.assert_matches_window(got, model, what=what)
    return counts


@pytest.mark.parametrize("i", range(15), ids=["+".join(f.name for f in s) for s in SUBSETS])
def test_every_instantiation_of_the_segmented_scan(ctx, small_table, i):
    funcs = SUBSET_FUNCS[i]
    counts = _check_small(ctx, small_table, funcs, what=f"scan operators {_bits(funcs)}")
    assert [counts[s] for s in ("win_gather", "win_scan_reduce", "win_scan_carry", "win_scan_apply", "win_emit")] == [1, 1, 1, 1, 1]  # one column, one scan


@pytest.mark.parametrize("func", ALONE, ids=["-".join([f[0].name] + ([f[2].name] if len(f) > 1 else [])) for f in ALONE])
def test_every_function_alone_asks_for_its_position_arrays_only(ctx, small_table, func):
    counts = _check_small(ctx, small_table, [func], what=f"{func} alone")
    needs_positions = len(func) == 1 or func[2] != F.Rows  # an aggregate over ROWS reads the state at the row itself: no position array
    assert [counts[s] for s in ("win_pos_reduce", "win_pos_carry", "win_pos_apply")] == ([1, 1, 1] if needs_positions else [0, 0, 0])
    assert counts["win_scan_apply"] == (0 if len(func) == 1 else 1) and counts["win_emit"] == 1
