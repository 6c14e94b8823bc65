"""The CPU oracle against the independent numpy model of selection and selection + projection (tests/selection_util.py) on reduced
versions — at most 20 000 rows — of every case family of tests/test_gpu_selection_forms.py: the tile pattern in its three placements
with the one-step projections (wrapping Int64 / UInt64, Float64 edge values, division and modulus by a literal), nullable sources and
a nullable predicate (quirk Q4), every mask predicate at every chunk-edge row count, a Boolean column as the predicate, and Utf8 columns
of every length band.  The generators' own coverage assertions run here too, before any device sees their output."""
import numpy as np
import pytest

from oracle import oracle as orc
from tests import selection_util as su
from tests.helpers import assert_batches_equal

REDUCED = (9 * su.TILE + 2000, 9 * su.TILE + 22_000)       # tiles that keep 65 (in part), 511, 512, 513 and 4095 (in part) rows


def oracle_selection(table, pred, exprs=None):
    batches = [su.to_columns(table)]
    out = orc.selection(batches, su.nodes(pred, len(table)))
    if exprs is not None:
        out = orc.projection(out, [su.nodes(e, len(table)) for e in exprs])
    assert len(out) == 1
    return out[0]


def check(table, pred, exprs=None, what=""):
    got = oracle_selection(table, pred, exprs)
    model = su.model_selection(table, pred) if exprs is None else su.model_selection_projection(table, pred, exprs)
    assert_batches_equal(got, su.to_columns(model), what=what)
    return model


@pytest.mark.parametrize("placement", su.PLACEMENTS)
def test_tile_pattern_covers_every_count_at_every_alignment(placement):
    m = su.tile_pattern(16, placement)                      # asserts its coverage itself
    assert len(m) == 984_274
    if placement != "random":
        assert int(m[-1]) == int(placement == "back") and int(m[-su.RAGGED]) == int(placement == "front")
    one = su.tile_pattern(1, placement)
    assert len(one) == 15 * su.TILE + su.RAGGED and int(one.sum()) == sum(su.TILE_COUNTS) + su.RAGGED_KEPT


@pytest.mark.parametrize("placement", su.PLACEMENTS)
def test_staged_family(placement):
    table = su.cut(su.staged_table(su.tile_pattern(1, placement)), *REDUCED)
    model = check(table, su.STAGED_PRED, what=f"{placement} selection")
    assert 5000 < len(model[0][0]) < 20_000
    for i, exprs in enumerate(su.STAGED_PROJECTIONS):
        check(table, su.STAGED_PRED, exprs, what=f"{placement} projection list {i}")


def test_general_family():
    table = su.cut(su.general_table(su.tile_pattern(1, "random")), *REDUCED)
    for pred, name in ((su.GENERAL_PRED, "plain predicate"), (su.GENERAL_PRED_NULLABLE, "nullable predicate")):
        model = check(table, pred, what=name)
        if pred is su.GENERAL_PRED_NULLABLE:
            assert (~model[0][1]).sum() > 50, "NULL rows are emitted"
        for i, exprs in enumerate(su.GENERAL_PROJECTIONS):
            check(table, pred, exprs, what=f"{name}, projection list {i}")


@pytest.mark.parametrize("n", su.MASK_SIZES + [20_000])
def test_mask_family(n):
    for last_kept in (True, False):
        table = su.mask_table(n, seed=n, last_kept=last_kept)
        su.check_mask_table(table, last_kept)
        for name, pred, _ in su.MASK_PREDICATES:
            check(table, pred, what=f"{name} n={n} last_kept={last_kept}")


@pytest.mark.parametrize("nullable", [False, True])
def test_boolean_column_as_the_predicate(nullable):
    """nqe_filter's predicate is a Boolean column; the oracle takes it as a column of the table (same length only)"""
    table = su.filter_table()
    pred = su.filter_pred(su.FILTER_ROWS, nullable)
    model = su.model_selection(table, pred)
    got = orc.selection([su.to_columns(table + [pred])], su.nodes(su.C(len(table)), len(table) + 1))[0]
    assert_batches_equal(got[:len(table)], su.to_columns(model), what=f"nullable={nullable}")
    # the model's Q3: a shorter or longer predicate column is the same selection over the first min(len, rows) rows
    for length in su.FILTER_PRED_LENGTHS:
        p = su.filter_pred(length, nullable)
        k = min(length, su.FILTER_ROWS)
        a = su.model_selection(table, p)
        b = su.model_selection(su.cut(table, 0, k), (p[0][:k], None if p[1] is None else p[1][:k]))
        assert_batches_equal(su.to_columns(a), su.to_columns(b), what=f"length {length}")
        assert len(a[0][0]) <= k


@pytest.mark.parametrize("mean", [b[0] for b in su.UTF8_BANDS])
def test_utf8_family(mean):
    full = su.utf8_table(mean)
    assert su.band_of(su.utf8_mean_bytes(full[1])) == su.band_of(mean)
    table = su.cut(full, 0, min(su.UTF8_ROWS, 20_000_00 // (mean * 10) + 100))
    for pred in (su.UTF8_PRED, su.UTF8_PRED_NULLABLE):
        check(table, pred, what=f"mean {mean}")
    for off in su.UTF8_SLICE_OFFSETS:
        length = len(table[0][0]) - off - 7
        got = orc.limit(orc.offset([su.to_columns(table)], off), length)
        assert len(got) == 1
        assert_batches_equal(got[0],su.to_columns(su.cut(table, off, off + length)), what=f"slice at {off}")
