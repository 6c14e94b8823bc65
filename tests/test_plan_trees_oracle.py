"""The reference side of tests/test_gpu_plan_trees.py is not taken on trust: the oracle's multi-batch operators (Selection with
quirks Q3 / Q4, Limit, Offset, the un-grouped aggregate executed k times, Q9) against numpy / Python models of a few lines each, at
the batch-length edges the device tests use; and the random-tree generator run through the oracle alone, so that the device fuzz
compares results and not mostly error codes.  No GPU."""
import numpy as np
import pytest

from naive_query_engine_amd import AggregateFunc as A, Column, DType, Operator
from naive_query_engine_amd.expression import binop, col, lit_i64
from oracle import oracle as orc
from tests.helpers import assert_column_equal
from tests.plan_tree_util import EDGES, RTOL, assert_same_batches, batch_lengths, make_batches, np_take, random_tree, schema, to_oracle

FLD = schema()
LENGTH_SETS = [[20000, 4097, 0, 8193, 63], [4096, 4096, 4096], [1000, 4095, 257, 20000, 65], [64, 127, 255, 1, 8193], [0, 65, 64]]
NULLS = [0.2, 0.0, 0.3, 0.0, 0.5]


def np_selection(batches, pvals, pvalid):
    """Q3: batch 0's predicate zipped against every batch and cut to the shorter side; Q4: a NULL predicate row emits a NULL row"""
    out = []
    for b in batches:
        n = min(pvals.size, b[0].length)
        rows = np.nonzero(~pvalid[:n] | pvals[:n])[0]
        out.append([np_take(c, rows, pvalid[rows]) for c in b])
    return out


def np_window(batches, lo, hi, keep):
    """rows [lo, hi) of the concatenated table, batch by batch; keep(start, end) says whether a batch that spans global rows
    [start, end) is emitted at all"""
    out, start = [], 0
    for b in batches:
        end = start + b[0].length
        if keep(start, end):
            out.append([np_take(c, np.arange(max(start, lo), min(end, hi)) - start) for c in b])
        start = end
    return out


def np_offset(batches, n):
    # a batch is skipped while rows remain to be dropped and it has no more than those; a zero-row batch passes once none remain
    return np_window(batches, n, 1 << 62, lambda s, e: n <= s or n < e)


def np_limit(batches, n):
    # the loop stops at the first batch that starts at or past the limit; a zero-row batch before that point is passed on
    return np_window(batches, 0, n, lambda s, e: s < n)


@pytest.fixture(scope="module", params=range(len(LENGTH_SETS)), ids=lambda i: "x".join(map(str, LENGTH_SETS[i])))
def batches(request):
    lengths = LENGTH_SETS[request.param]
    return make_batches(50 + request.param, lengths, NULLS[: len(lengths)], nan_frac=0.01)


def test_length_sets_cover_every_edge():
    assert {n for s in LENGTH_SETS for n in s} >= set(EDGES)


def test_oracle_multi_batch_selection_q3_q4(batches):
    k0, b0 = batches[0][1], batches[0][4]
    for what, pred, pvals, pvalid in [("k < 10", binop(col("k"), Operator.Lt, lit_i64(10)), k0.to_numpy() < 10, k0.valid_mask()),
                                      ("b", col("b"), b0.to_numpy(), b0.valid_mask())]:
        assert_same_batches(orc.selection(batches, pred.flatten(FLD)), np_selection(batches, pvals, pvalid), what)


def test_oracle_offset_and_limit_over_batch_boundaries(batches):
    lengths = [b[0].length for b in batches]
    total, first = sum(lengths), lengths[0]
    for n in sorted({0, 1, max(first - 1, 0), first, first + 1, first + 63, first + 64, first + 65, max(total - 1, 0), total, total + 5}):
        assert_same_batches(orc.offset(batches, n), np_offset(batches, n), f"offset {n} of {lengths}")
        assert_same_batches(orc.limit(batches, n), np_limit(batches, n), f"limit {n} of {lengths}")
    off = orc.offset(batches, first + 1, raw=True)
    assert_same_batches(orc.limit(off, 70), np_limit(np_offset(batches, first + 1), 70), "limit 70 over offset (chained handles)")


def test_oracle_ungrouped_aggregate_keeps_state_q9(batches):
    aggs = [(A.Count, 2), (A.Sum, 2), (A.Avg, 2), (A.Min, 2), (A.Max, 2), (A.Count, 5), (A.Count, 4)]
    v = np.concatenate([b[2].to_numpy()[b[2].valid_mask()] for b in batches])
    finite = v[~np.isnan(v)]
    for k in (1, 2, 3):
        got = orc.aggregate(batches, aggs, executions=k)
        assert batch_lengths(orc.aggregate(batches, aggs, executions=k, raw=True)) == [1]
        row = [c.to_numpy()[0] for c in got[0]]
        assert row[0] == k * v.size and row[5] == k * sum(int(b[5].valid_mask().sum()) for b in batches)
        assert row[6] == k * sum(int(b[4].valid_mask().sum()) for b in batches)
        # NaN in the input: the sum is NaN, max is NaN (OrderedFloat: NaN above everything), min ignores it
        assert row[3] == finite.min()
        if finite.size < v.size:
            assert np.isnan(row[1]) and np.isnan(row[2]) and np.isnan(row[4])
    clean = [[c if i != 2 else Column.from_numpy(np.nan_to_num(c.to_numpy(), nan=7.0), c.valid_mask()) for i, c in enumerate(b)] for b in batches]
    v = np.concatenate([b[2].to_numpy()[b[2].valid_mask()] for b in clean])
    for k in (1, 2, 3):
        row = [c.to_numpy()[0] for c in orc.aggregate(clean, aggs, executions=k)[0]]
        assert row[0] == k * v.size and row[3] == v.min() and row[4] == v.max()
        assert np.isclose(row[1], k * np.sum(v, dtype=np.longdouble), rtol=RTOL, atol=0)
        assert np.isclose(row[2], np.sum(v, dtype=np.longdouble) / v.size, rtol=RTOL, atol=0)


def test_oracle_aggregate_above_selection_is_selection_then_aggregate(batches):
    """the two ways the device tests feed the oracle a filtered aggregate agree: its own Aggregate(Selection(..)) and chained handles"""
    pred = binop(col("k"), Operator.Lt, lit_i64(10)).flatten(FLD)
    aggs = [(A.Count, 2), (A.Min, 2), (A.Max, 2), (A.Count, 5)]
    a = orc.aggregate(batches, aggs, pred_nodes=pred)
    b = orc.aggregate(orc.selection(batches, pred, raw=True), aggs)
    for x, y in zip(a[0], b[0]):
        assert_column_equal(x, y)


def test_fuzz_generator_mostly_yields_results():
    """the 16 default seeds of the device fuzz through the oracle chain alone: at most a quarter may end in an error, the trees
    stay within depth 4, and between them they use every operator"""
    errors, ops = 0, set()
    for seed in range(16):
        host, tree, status = random_tree(seed)
        assert tree.depth() <= 4, f"seed {seed}: {tree!r}"
        assert tree.ops().count("join") <= 1 and "agg" not in tree.ops()[1:], f"seed {seed}: {tree!r}"
        ops |= set(tree.ops())
        try:
            to_oracle(tree, host).to_python()
            assert status is None, f"seed {seed}: grown with status {status}, chain ran: {tree!r}"
        except orc.ErrorCode as e:
            assert status == e.status, f"seed {seed}: {tree!r}"
            errors += 1
    assert errors <= 4, f"{errors} of 16 seeds end in an error"
    assert ops >= {"scan", "sel", "proj", "off", "lim", "join", "agg"}, ops
