"""The model of the nqe_window_execute_ex tests (tests/window_ex_util.py) against three independent statements of the same thing:
sqlite3's window functions (ROWS BETWEEN frames, lag / lead with and without default, first_value / last_value, ntile) on small seeded
tables; window_util.window for the functions and frames of the old entry; and the whole-array numpy form against the row-at-a-time form.
SQLite gives NULL for an aggregate over a frame without a valid row where Q10 gives the start values, so sum / min / max / avg are
compared where the frame holds a valid row (count everywhere).  The row index is SQLite's last ORDER BY key: that is what the stable
sort means."""
import os
import sqlite3
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import agg_value_util as avu  # noqa: E402
import window_ex_util as wx  # noqa: E402
import window_util as wu  # noqa: E402
from naive_query_engine_amd import Column, DType, WindowFrame as F, WindowFrameEx as FX, WindowFunc as W, WindowFuncEx as WX  # noqa: E402

SQL_AGG = {WX.Count: "count(v)", WX.Sum: "sum(v)", WX.Min: "min(v)", WX.Max: "max(v)", WX.Avg: "avg(v)"}
FRAMES = [(-2, 0), (0, 2), (-1, 1), (-3, -1), (1, 3), (None, 2), (-2, None), (None, -1), (1, None), (None, None), (0, 0), (-300, 300), (5, 9)]


def _bound(x, following):
    if x is None:
        return "unbounded following" if following else "unbounded preceding"
    return "current row" if x == 0 else f"{-x} preceding" if x < 0 else f"{x} following"


def _sql_frame(start, end):
    return f"rows between {_bound(start, False)} and {_bound(end, True)}"


def _table(seed, n):
    rng = np.random.default_rng(seed)
    p = [None if rng.random() < 0.1 else int(x) for x in rng.integers(0, 4, n)]
    o = [None if rng.random() < 0.1 else int(x) for x in rng.integers(-3, 4, n)]
    v = [None if rng.random() < 0.25 else int(x) for x in rng.integers(-(1 << 40), 1 << 40, n)]
    cols = [Column.from_list(p, DType.INT64), Column.from_list(o, DType.INT64), Column.from_list(v, DType.INT64)]
    for c in cols:
        if c.validity is None:
            c.validity = np.packbits(np.ones(n, dtype=bool), bitorder="little")
    db = sqlite3.connect(":memory:")
    db.execute("create table t (idx integer, p integer, o integer, v integer)")
    db.executemany("insert into t values (?, ?, ?, ?)", [(i, p[i], o[i], v[i]) for i in range(n)])
    return db, cols


def _value_list(m, i):
    signed = m.cols[i].view(np.int64)
    return [int(x) if ok else None for x, ok in zip(signed.tolist(), m.valids[i].tolist())]


@pytest.mark.parametrize("seed", range(4))
def test_model_agrees_with_sqlite(seed):
    assert sqlite3.sqlite_version_info >= (3, 28)  # frames that exclude the current row, lag / lead, ntile
    n = 150
    db, cols = _table(seed, n)
    for parts, over in (([0], "partition by p order by o, idx"), ([], "order by o, idx")):
        query = lambda expr, frame="": [r[0] for r in db.execute(f"select {expr} over ({over} {frame}) from t order by idx")]
        for start, end in FRAMES:
            funcs = wx.all_aggs(2, start, end) + [wx.first(2, start, end), wx.last(2, start, end)]
            m = wx.window_ex(cols, parts, [1], funcs)
            what = f"seed {seed} partition by {parts} frame ({start}, {end})"
            keep = m.cols[0] > 0
            for i, f in enumerate(m.funcs[:5]):
                got = query(SQL_AGG[f["func"]], _sql_frame(start, end))
                if f["func"] == WX.Count:
                    assert got == m.cols[i].tolist(), what
                    continue
                assert all(g is None for g, k in zip(got, keep) if not k), what
                g = np.array([0.0 if x is None else float(x) for x in got])
                same = wu.same_mask(wx._AS_OLD[f["func"]], g, m.cols[i].astype(np.float64), m.tols[i])
                assert same[keep].all(), f"{what} {f['func'].name}: rows {np.nonzero(~same & keep)[0][:5]}"
                if f["func"] == WX.Sum:
                    assert (g[keep] == m.cols[i][keep]).all(), what  # integers below 2^53: exact
            assert query("first_value(v)", _sql_frame(start, end)) == _value_list(m, 5), what + " first_value"
            assert query("last_value(v)", _sql_frame(start, end)) == _value_list(m, 6), what + " last_value"
        for k in (0, 1, 2, 7, n):
            m = wx.window_ex(cols, parts, [1], [wx.lag(2, k), wx.lead(2, k), wx.lag(2, k, -77), wx.lead(2, k, 99)])
            for i, expr in enumerate((f"lag(v, {k})", f"lead(v, {k})", f"lag(v, {k}, -77)", f"lead(v, {k}, 99)")):
                assert query(expr) == _value_list(m, i), f"seed {seed} {parts} {expr}"
        for b in (1, 2, 3, 7, n, n + 1, 1000):
            m = wx.window_ex(cols, parts, [1], [wx.ntile(b)])
            assert query(f"ntile({b})") == m.cols[0].tolist(), f"seed {seed} {parts} ntile({b})"
        # the old frames of first_value / last_value: ROWS and PARTITION as SQLite spells them (RANGE needs peers: no idx in the order)
        m = wx.window_ex(cols, parts, [1], [wx.first(2, frame=FX.Rows), wx.last(2, frame=FX.Rows), wx.first(2, frame=FX.Partition), wx.last(2, frame=FX.Partition)])
        assert query("first_value(v)", _sql_frame(None, 0)) == _value_list(m, 0) and query("last_value(v)", _sql_frame(None, 0)) == _value_list(m, 1)
        assert query("first_value(v)", _sql_frame(None, None)) == _value_list(m, 2) and query("last_value(v)", _sql_frame(None, None)) == _value_list(m, 3)
        over_peers = over.replace(", idx", "")
        got = [r[0] for r in db.execute(f"select last_value(v) over ({over_peers} range between unbounded preceding and current row) from t order by idx")]
        m = wx.window_ex(cols, parts, [1], [wx.agg(WX.Count, 2, None, None), wx.last(2, frame=FX.Range)])
        # the last peer in the stable order is the peer with the largest row index; SQLite's choice among peers is its own, so compare
        # where the peer group is one row
        lay = wu.Layout(cols, parts, [1])
        alone = np.zeros(n, dtype=bool)
        for i in range(n):
            alone[lay.order[i]] = lay.peer_first[i] == lay.peer_last[i]
        assert [g for g, a in zip(got, alone) if a] == [g for g, a in zip(_value_list(m, 1), alone) if a]


def test_empty_frames_and_frames_of_nulls_give_the_start_values():
    v = Column.from_numpy(np.array([1.5, 2.5, 4.0, 8.0, 16.0]), np.array([True, True, False, False, True]))
    m = wx.window_ex([v], [], [], wx.all_aggs(0, -2, -1) + [wx.first(0, -2, -1), wx.last(0, 3, 9), wx.agg(WX.Sum, 0, 1, 1)])
    # row 0: the frame is empty; row 4: the frame is rows 2 and 3, both NULL
    for row in (0, 4):
        assert m.cols[0][row] == 0 and m.cols[1][row] == 0.0 and m.cols[2][row] == avu.F64_MAX and m.cols[3][row] == -avu.F64_MAX and np.isnan(m.cols[4][row])
    assert m.cols[1].tolist() == [0.0, 1.5, 4.0, 2.5, 0.0] and m.cols[7].tolist() == [2.5, 0.0, 0.0, 16.0, 0.0]
    assert m.valids[5].tolist() == [False, True, True, True, False] and m.cols[5][1:4].view(np.float64).tolist() == [1.5, 1.5, 2.5]
    assert m.valids[6].tolist() == [True, True, False, False, False] and m.cols[6][:2].view(np.float64).tolist() == [16.0, 16.0]


def test_ntile_by_hand():
    m = wx.window_ex([Column.from_numpy(np.arange(7, dtype=np.int64))], [], [0], [wx.ntile(3), wx.ntile(7), wx.ntile(8), wx.ntile(1), wx.ntile(2)])
    assert m.cols[0].tolist() == [1, 1, 1, 2, 2, 3, 3] and m.cols[1].tolist() == [1, 2, 3, 4, 5, 6, 7] and m.cols[2].tolist() == [1, 2, 3, 4, 5, 6, 7]
    assert m.cols[3].tolist() == [1] * 7 and m.cols[4].tolist() == [1, 1, 1, 1, 2, 2, 2]


def _random_table(seed, n, special):
    rng = np.random.default_rng(seed)
    x = rng.integers(-1000, 1000, n).astype(np.float64)
    if special:
        x[rng.integers(0, n, n // 9)] = np.inf
        x[rng.integers(0, n, n // 9)] = -np.inf
        x[rng.integers(0, n, n // 9)] = np.nan
    return [Column.from_numpy(rng.integers(0, 5, n).astype(np.int64)), Column.from_numpy(rng.integers(0, 12, n).astype(np.int64), rng.random(n) > 0.1),
            Column.from_numpy(rng.integers(-1000, 1000, n).astype(np.int64), rng.random(n) > 0.2), Column.from_numpy(x, rng.random(n) > 0.1)]


@pytest.mark.parametrize("seed", range(3))
def test_old_functions_and_frames_are_window_utils(seed):
    cols = _random_table(seed, 300, True)
    old = [(W.RowNumber,), (W.Rank,), (W.DenseRank,)] + [(fn, c, fr) for c in (2, 3) for fr in wu.FRAMES for fn in wu.AGGREGATES]
    m_old = wu.window(cols, [0], [(1, True, False)], old)
    m = wx.window_ex(cols, [0], [(1, True, False)], [wx.old(*f) for f in old])
    for i in range(len(old)):
        assert m.cols[i].dtype == m_old.cols[i].dtype and (m.cols[i].view(np.uint64) == m_old.cols[i].view(np.uint64)).all(), old[i]
    # ROWS is (UNBOUNDED, 0) and PARTITION is (UNBOUNDED, UNBOUNDED): the frame walk gives window_util's running state
    between = wx.window_ex(cols, [0], [(1, True, False)], wx.all_aggs(3, None, 0) + wx.all_aggs(3, None, None))
    same = wx.window_ex(cols, [0], [(1, True, False)], [wx.old(fn, 3, F.Rows) for fn in wu.AGGREGATES] + [wx.old(fn, 3, F.Partition) for fn in wu.AGGREGATES])
    for i, f in enumerate(between.funcs):
        assert wu.same_mask(wx._AS_OLD[f["func"]], between.cols[i], same.cols[i], same.tols[i]).all(), wx.describe(f)


@pytest.mark.parametrize("seed", range(3))
def test_numpy_form_agrees_with_the_row_at_a_time_form(seed):
    n = 257
    cols = _random_table(10 + seed, n, True)
    frames = FRAMES + [(-n, n), (-n - 1, n + 1), (-(2 ** 63) + 1, 2 ** 63 - 2), (2 ** 63 - 2, 2 ** 63 - 2), (16, 16), (-40, -8)]
    funcs = []
    for c in (2, 3):
        for start, end in frames:
            funcs += wx.all_aggs(c, start, end) + [wx.first(c, start, end), wx.last(c, start, end)]
    funcs += [wx.lag(3, k, d) for k in (0, 1, 5, n, 10 * n) for d in (None, 2.5)] + [wx.lead(2, k, d) for k in (0, 1, 5, n, 10 * n) for d in (None, -3)]
    funcs += [wx.ntile(b) for b in (1, 2, 3, 50, n, 1000)] + [wx.first(3, frame=fr) for fr in (FX.Rows, FX.Range, FX.Partition)] + [wx.last(2, frame=fr) for fr in (FX.Rows, FX.Range, FX.Partition)]
    funcs += [wx.old(W.Rank), wx.old(W.Sum, 2, F.Range)]
    for parts, order in (([0], [1]), ([], [(1, True, False)]), ([0], [])):
        a, b = wx.window_ex(cols, parts, order, funcs), wx.window_ex_np(cols, parts, order, funcs)
        for i, f in enumerate(a.funcs):
            w = f"{parts} {order} {wx.describe(f)}"
            assert a.dtypes[i] == b.dtypes[i] and a.cols[i].dtype == b.cols[i].dtype, w
            if f["func"] in wx.VALUES:
                assert (a.valids[i] == b.valids[i]).all() and (a.cols[i][a.valids[i]] == b.cols[i][a.valids[i]]).all(), w
            else:
                # integer values: every sum is exact in both forms, so the numpy form's bound (0, one ulp for avg) holds for the other form's value
                assert wu.same_mask(wx._AS_OLD[f["func"]], a.cols[i], b.cols[i], b.tols[i]).all(), w
