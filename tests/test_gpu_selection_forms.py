"""Every keep-mask kernel and every compaction form of csrc/selection.hip, and the Utf8 copy kernels of take_utf8 (csrc/context.hip), at
the shapes where such code goes wrong, against the numpy model of tests/selection_util.py (which tests/test_selection_model_oracle.py
holds to the CPU oracle).  Every comparison is exact — values bit for bit (NaN = NaN), validity, row count, row order — and every table
carries a row-id column of distinct values (row * odd constant), so a row in another row's place is a wrong value.

  A  compact_staged_kernel<0|1|2> (>= 64 tiles, plain words) over tiles that keep 0, 1, 2, 15 … 4095, 4096 rows with every count at
     every output alignment (base mod 16), kept rows at random / packed at the front / packed at the back of the tile, a ragged last
     tile; and the same pattern cut to 63 tiles and 63 tiles + 1 row, either side of the strided / staged switch
  B  the general compact_kernel past 64 tiles: nullable and Boolean sources, a nullable predicate's NULL rows (Q4), Boolean output
  C  the mask kernels at every edge of their 64 / 512 / 1024 / 4096-row chunks, last row kept and last row dropped
  D  the 2^20-row switch of a chain predicate from keep_from_simple to the expression machine + keep_from_pred
  E  nqe_filter with a predicate column shorter and longer than the table, across tiles (Q3)
  F  Utf8 through selection, take and slice with the output's mean length in each of take_utf8's five bands

The run-time specialised kernels are switched off (NQE_NO_JIT, read per call), so the per-expression kernels run whatever the row
count; the forms are told apart by their timing labels where the labels differ."""
import numpy as np
import pytest

from naive_query_engine_amd import Column
from tests import selection_util as su
from tests.helpers import assert_batches_equal, assert_column_equal

pytestmark = pytest.mark.gpu

MASK_LABELS = {"keep_from_simple", "keep_from_conj", "keep_from_pred"}
JIT_LABELS = {"proj_jit", "select_project_jit"}


@pytest.fixture(scope="module")
def ctx():
    from naive_query_engine_amd import capi

    c = capi.Context(0)
    yield c
    c.close()


@pytest.fixture(autouse=True)
def no_jit(monkeypatch):
    monkeypatch.setenv("NQE_NO_JIT", "1")


def run(ctx, fn):
    """(the table fn() returns, the labels of what it launched)"""
    ctx.timing_enable(True)
    ctx.timing_reset()
    try:
        out = fn()
    finally:
        ctx.timing_enable(False)
    labels = set(ctx.timing_report())
    assert not labels & JIT_LABELS, labels
    return out, labels


def select(ctx, dev, table, pred, exprs=None):
    ncols = len(table)
    if exprs is None:
        return run(ctx, lambda: ctx.selection(dev, su.nodes(pred, ncols)))
    return run(ctx, lambda: ctx.selection_projection(dev, su.nodes(pred, ncols), [su.nodes(e, ncols) for e in exprs]))


def assert_table(got, model, what):
    assert got.num_rows == (len(model[0][0]) if model else 0), what
    assert_batches_equal(got.to_host(), su.to_columns(model), what=what)


class Case:
    """a model table, its device copy and the model's selection of it (computed once, shared, never written)"""

    def __init__(self, ctx, table, pred):
        self.table, self.pred = table, pred
        self.dev = ctx.table_from_host(su.to_columns(table))
        self.selected = su.model_selection(table, pred)

    def check_selection(self, ctx, label="compact_column"):
        got, labels = select(ctx, self.dev, self.table, self.pred)
        assert_table(got, self.selected, "selection")
        assert label in labels, labels
        return labels

    def check_projection(self, ctx, exprs, what):
        got, labels = select(ctx, self.dev, self.table, self.pred, exprs)
        assert_table(got, su.model_projection(self.selected, exprs), what)
        return labels


# ------------------------------------------------------------------------------------------------------------------ A
@pytest.fixture(scope="module", params=su.PLACEMENTS)
def pattern(request):
    return request.param, su.tile_pattern(16, request.param)          # asserts its coverage before anything reaches the device


@pytest.fixture(scope="module")
def staged(ctx, pattern):
    placement, m = pattern
    case = Case(ctx, su.staged_table(m), su.STAGED_PRED)
    assert len(m) == 240 * su.TILE + su.RAGGED and len(case.selected[0][0]) == 16 * sum(su.TILE_COUNTS) + su.RAGGED_KEPT
    for v, edges in ((case.selected[2][0], su.U64_EDGES), (case.selected[3][0].view(np.uint64), su.F64_EDGES.view(np.uint64))):
        assert np.isin(edges, v).all(), "every edge value is among the kept rows"
    return case


def test_staged_selection(ctx, staged):
    """compact_staged_kernel<0> over every column"""
    labels = staged.check_selection(ctx)
    assert "keep_from_simple" in labels and "compact_expr" not in labels


@pytest.mark.parametrize("which", range(len(su.STAGED_PROJECTIONS)))
def test_staged_projection(ctx, staged, which):
    """<2> for + - * by a literal over Int64 / UInt64 (both sides, wrapping), <1> for Float64 steps, % and /, <0> for bare columns"""
    exprs = su.STAGED_PROJECTIONS[which]
    labels = staged.check_projection(ctx, exprs, f"projection list {which}")
    assert ("compact_column" if which == len(su.STAGED_PROJECTIONS) - 1 else "compact_expr") in labels, labels


@pytest.mark.parametrize("n", [63 * su.TILE, 63 * su.TILE + 1])
def test_strided_and_staged_on_either_side_of_64_tiles(ctx, pattern, n):
    placement, m = pattern
    case = Case(ctx, su.cut(su.staged_table(m), 0, n), su.STAGED_PRED)
    case.check_selection(ctx)
    for which, exprs in enumerate(su.STAGED_PROJECTIONS):
        case.check_projection(ctx, exprs, f"n={n} projection list {which}")


# ------------------------------------------------------------------------------------------------------------------ B
@pytest.fixture(scope="module")
def general_table():
    return su.cut(su.general_table(su.tile_pattern(16, "random")), 0, 65 * su.TILE)


@pytest.fixture(scope="module", params=["plain", "nullable"])
def general(ctx, general_table, request):
    case = Case(ctx, general_table, su.GENERAL_PRED if request.param == "plain" else su.GENERAL_PRED_NULLABLE)
    null_rows = ~case.selected[0][1] if case.selected[0][1] is not None else np.zeros(0, bool)
    if request.param == "nullable":
        nul = ~general_table[2][1]
        assert int(null_rows.sum()) == int(nul.sum()) > 1000                       # every NULL of the predicate is an emitted NULL row
        assert int(nul[general_table[1][0] == 0].sum()) > 1000                       # most of them where the row would have been dropped
    else:
        assert case.selected[0][1] is None
    return case


def test_general_selection(ctx, general):
    """nullable Int64 / Float64 / Boolean sources and a plain Boolean one through compact_kernel; with the nullable predicate every
    column goes through it and the NULL rows' count and positions are the model's"""
    labels = general.check_selection(ctx)
    assert "keep_from_simple" in labels


@pytest.mark.parametrize("which", range(len(su.GENERAL_PROJECTIONS)))
def test_general_projection(ctx, general, which):
    labels = general.check_projection(ctx, su.GENERAL_PROJECTIONS[which], f"projection list {which}")
    assert "compact_expr" in labels, labels


# ------------------------------------------------------------------------------------------------------------------ C
def leave_stale_ones(ctx, n):
    """Best effort against masks that rely on zeroed memory: tables of all-ones words with the byte sizes the mask buffers of an n-row
    selection are about to request (keep and validity words, tile counts, tile offsets) are uploaded and released, so that the block
    pool hands those blocks back full of ones.  Nothing guarantees that the pool does; when it does not, the test checks no less than
    without this step."""
    nwords, ntiles = (n + 63) // 64, (n + su.TILE - 1) // su.TILE
    for nbytes in (nwords * 8 + 8, (ntiles + 1) * 4, (ntiles + 1) * 8, n * 8, n + 8):
        ones = np.full((nbytes + 7) // 8, ~np.uint64(0), dtype=np.uint64)
        tables = [ctx.table_from_host([Column.from_numpy(ones)]) for _ in range(3)]
        for t in tables:
            t.release()


@pytest.mark.parametrize("n", su.MASK_SIZES)
def test_mask_kernels_at_chunk_edges(ctx, n):
    for last_kept in (True, False):
        table = su.mask_table(n, seed=n, last_kept=last_kept)
        su.check_mask_table(table, last_kept)
        leave_stale_ones(ctx, n)
        dev = ctx.table_from_host(su.to_columns(table))
        for name, pred, label in su.MASK_PREDICATES:
            what = f"{name} n={n} last_kept={last_kept}"
            model = su.model_selection(table, pred)
            assert (len(model[0][0]) > 0 and model[0][0][-1] == table[0][0][-1]) == last_kept, what
            got, labels = select(ctx, dev, table, pred)
            assert_table(got, model, what)
            assert labels & MASK_LABELS == {label}, (what, labels)


# ------------------------------------------------------------------------------------------------------------------ D
@pytest.mark.parametrize("n", [(1 << 20) - 1, 1 << 20, (1 << 20) + 4097])
def test_chain_predicate_on_either_side_of_2p20_rows(ctx, n):
    rng = np.random.default_rng(n)
    table = [(su.row_ids(n), None), (rng.integers(-50, 51, n).astype(np.int64), None)]
    dev = ctx.table_from_host(su.to_columns(table))
    got, labels = select(ctx, dev, table, su.CHAIN_PRED)
    assert_table(got, su.model_selection(table, su.CHAIN_PRED), f"n={n}")
    assert labels & MASK_LABELS == {"keep_from_simple" if n < (1 << 20) else "keep_from_pred"}, labels


# ------------------------------------------------------------------------------------------------------------------ E
@pytest.fixture(scope="module")
def filter_case(ctx):
    table = su.filter_table()
    return table, ctx.table_from_host(su.to_columns(table))


@pytest.mark.parametrize("nullable", [False, True])
@pytest.mark.parametrize("length", su.FILTER_PRED_LENGTHS)
def test_filter_with_a_predicate_of_another_length(ctx, filter_case, length, nullable):
    table, dev = filter_case
    pred = su.filter_pred(length, nullable)
    pdev = ctx.table_from_host([su.to_column(pred)])
    got, labels = run(ctx, lambda: ctx.filter(dev, pdev, 0))
    model = su.model_selection(table, pred)
    assert len(model[0][0]) <= min(length, su.FILTER_ROWS)
    assert_table(got, model, f"length {length} nullable={nullable}")
    assert labels & MASK_LABELS == {"keep_from_pred"}, labels


# ------------------------------------------------------------------------------------------------------------------ F
@pytest.fixture(scope="module", params=range(len(su.UTF8_BANDS)))
def utf8(ctx, request):
    band = request.param
    table = su.utf8_table(su.UTF8_BANDS[band][0])
    return band, table, ctx.table_from_host(su.to_columns(table))


def in_band(model, band):
    assert su.band_of(su.utf8_mean_bytes(model[1])) == band, (su.utf8_mean_bytes(model[1]), su.UTF8_BANDS[band])


@pytest.mark.parametrize("nullable_predicate", [False, True])
def test_utf8_selection(ctx, utf8, nullable_predicate):
    band, table, dev = utf8
    pred = su.UTF8_PRED_NULLABLE if nullable_predicate else su.UTF8_PRED
    model = su.model_selection(table, pred)
    in_band(model, band)
    got, labels = select(ctx, dev, table, pred)
    assert_table(got, model, f"band {band}")
    assert {"kept_rows", "utf8_take_copy"} <= labels, labels


def test_utf8_take_with_repeated_indices(ctx, utf8):
    band, table, dev = utf8
    idx = su.utf8_take_indices()
    model = su.take_rows(table, idx)
    in_band(model, band)
    got, labels = run(ctx, lambda: ctx.take(dev, ctx.table_from_host([Column.from_numpy(idx)]), 0))
    assert_table(got, model, f"band {band}")
    assert "utf8_take_copy" in labels, labels


@pytest.mark.parametrize("offset", su.UTF8_SLICE_OFFSETS)
def test_utf8_slice(ctx, utf8, offset):
    band, table, dev = utf8
    length = su.UTF8_ROWS - offset - 7
    model = su.cut(table, offset, offset + length)
    in_band(model, band)
    got, labels = run(ctx, lambda: ctx.slice(dev, offset, length))
    assert_table(got, model, f"band {band} offset {offset}")
    assert "utf8_take_copy" in labels, labels
