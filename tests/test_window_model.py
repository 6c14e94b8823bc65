"""CPU-only: the window-function model of tests/window_util.py (quirk Q23) on hand-written cases, its incremental state against
agg_value_util's per-group state (every frame one group), and against sqlite3 where the two definitions coincide: Int64 and Utf8
keys with NULLs ascending (NULLs first in both) or descending with NULLs last, integer values below 2^53 with NULLs, the three frames
written out, all eight functions.  ROW_NUMBER and ROWS get the row index as SQLite's last ORDER BY key (that is what stability
means); RANK, DENSE_RANK, RANGE and PARTITION do not.  Only frames with a valid row are compared: for an empty frame SQLite gives NULL
and Q10 the start values."""
import math
import os
import sqlite3
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import agg_value_util as avu  # noqa: E402
import order_by_util as obu  # noqa: E402
import window_util as wu  # noqa: E402
from naive_query_engine_amd import AggregateFunc, Column, DType, WindowFrame as F, WindowFunc as W  # noqa: E402

NAN, INF, MAX = math.nan, math.inf, avu.F64_MAX


def _vals(m, i):
    return [None if isinstance(v, float) and math.isnan(v) else v for v in m.cols[i].tolist()]


# ----------------------------------------------------------------------------- by hand
def test_ranking_functions_by_hand():
    part = Column.from_numpy(np.array([2, 1, 2, 1, 2, 2, 1], dtype=np.int64))
    key = Column.from_numpy(np.array([5, 7, 5, 7, 3, 9, 1], dtype=np.int64))
    m = wu.window([part, key], [0], [1], [W.RowNumber, W.Rank, W.DenseRank])
    # partition 1 in order: rows 6 (1), 1 (7), 3 (7); partition 2: rows 4 (3), 0 (5), 2 (5), 5 (9)
    assert m.cols[0].tolist() == [2, 2, 3, 3, 1, 4, 1]
    assert m.cols[1].tolist() == [2, 2, 2, 2, 1, 4, 1]
    assert m.cols[2].tolist() == [2, 2, 2, 2, 1, 3, 1]
    d = wu.window([part, key], [0], [(1, True)], [W.RowNumber, W.Rank, W.DenseRank])  # descending: 9, 5, 5, 3 and 7, 7, 1
    assert d.cols[0].tolist() == [2, 1, 3, 2, 4, 1, 3] and d.cols[1].tolist() == [2, 1, 2, 1, 4, 1, 3] and d.cols[2].tolist() == [2, 1, 2, 1, 3, 1, 2]
    none = wu.window([part, key], [0], [], [W.RowNumber, W.Rank, W.DenseRank])  # no order keys: all peers, input order
    assert none.cols[0].tolist() == [1, 1, 2, 2, 3, 4, 3] and none.cols[1].tolist() == [1] * 7 and none.cols[2].tolist() == [1] * 7
    one = wu.window([part, key], [], [], [W.RowNumber, W.Rank])  # no keys at all: one partition
    assert one.cols[0].tolist() == [1, 2, 3, 4, 5, 6, 7] and one.cols[1].tolist() == [1] * 7


def test_frames_by_hand():
    part = Column.from_numpy(np.array([0, 0, 0, 0, 1], dtype=np.int64))
    key = Column.from_numpy(np.array([1, 2, 2, 3, 0], dtype=np.int64))
    v = Column.from_list([10, None, 5, 1, None], DType.INT64)
    m = wu.window([part, key, v], [0], [1], [(W.Sum, 2, F.Rows), (W.Sum, 2, F.Range), (W.Sum, 2, F.Partition), (W.Count, 2, F.Rows), (W.Count, 2, F.Range),
                                              (W.Avg, 2, F.Range), (W.Min, 2, F.Rows), (W.Max, 2, F.Partition), (W.Avg, 2, F.Partition)])
    assert m.cols[0].tolist() == [10.0, 10.0, 15.0, 16.0, 0.0]  # ROWS: the NULL adds nothing
    assert m.cols[1].tolist() == [10.0, 15.0, 15.0, 16.0, 0.0]  # RANGE: rows 1 and 2 are peers, both see the 5
    assert m.cols[2].tolist() == [16.0, 16.0, 16.0, 16.0, 0.0]
    assert m.cols[3].tolist() == [1, 1, 2, 3, 0] and m.cols[4].tolist() == [1, 2, 2, 3, 0]
    assert _vals(m, 5) == [10.0, 7.5, 7.5, 16.0 / 3.0, None]     # a frame without valid rows: avg NaN
    assert m.cols[6].tolist() == [10.0, 10.0, 5.0, 1.0, MAX]      # … min f64::MAX
    assert m.cols[7].tolist() == [10.0, 10.0, 10.0, 10.0, -MAX]   # … max f64::MIN
    assert m.tols[0].tolist() == [1 * 2.0 ** -52 * 10, 1 * 2.0 ** -52 * 10, 2 * 2.0 ** -52 * 15, 3 * 2.0 ** -52 * 16, 0.0]  # n_frame * 2^-52 * sum|x|


def test_q10_specials_by_hand():
    v = Column.from_numpy(np.array([1.0, NAN, INF, 2.0, -INF, -0.0, INF, INF]))
    part = Column.from_numpy(np.array([0, 0, 0, 0, 0, 1, 2, 2], dtype=np.int64))
    m = wu.window([part, v], [0], [], [(W.Sum, 1, F.Rows), (W.Min, 1, F.Rows), (W.Max, 1, F.Rows), (W.Sum, 1, F.Partition), (W.Min, 1, F.Partition)])
    assert _vals(m, 0) == [1.0, None, None, None, None, 0.0, INF, INF]
    assert m.cols[1].tolist() == [1.0, 1.0, 1.0, 1.0, -INF, 0.0, MAX, MAX]  # min ignores NaN; a frame of nothing but +inf keeps f64::MAX
    assert _vals(m, 2) == [1.0, None, None, None, None, 0.0, INF, INF]     # max becomes NaN and stays NaN
    assert _vals(m, 3) == [None] * 5 + [0.0, INF, INF]
    assert m.cols[4].tolist() == [-INF] * 5 + [0.0, MAX, MAX]


def test_key_ties_by_hand():
    f = Column.from_numpy(np.array([0.0, -0.0, NAN, -NAN, 1.0]))  # the zeros tie, the NaNs tie
    assert wu.window([f], [0], [], [W.RowNumber]).cols[0].tolist() == [1, 2, 1, 2, 1]
    k = Column.from_list([None, 3, None, 3], DType.INT64)            # NULLs form one partition
    assert wu.window([k], [0], [], [W.RowNumber]).cols[0].tolist() == [1, 1, 2, 2]
    for desc in (False, True):
        for nf in (False, True):                                     # NULL order keys are peers wherever they are placed
            m = wu.window([k], [], [(0, desc, nf)], [W.Rank, W.DenseRank])
            assert m.cols[0].tolist() == ([1, 3, 1, 3] if nf else [3, 1, 3, 1]) and m.cols[1].tolist() == ([1, 2, 1, 2] if nf else [2, 1, 2, 1])
    s = obu.utf8_column([b"a", b"a\0", b"a", None, None], null_bytes=b"zz")
    assert wu.window([s], [0], [], [W.RowNumber]).cols[0].tolist() == [1, 1, 2, 1, 2]


# ----------------------------------------------------------------------------- the incremental state against agg_value_util's
@pytest.mark.parametrize("domain,nullable", avu.VARIANTS, ids=avu.VARIANT_IDS)
def test_running_state_equals_the_per_group_state_of_every_frame(domain, nullable):
    rng = np.random.default_rng(avu.DOMAINS.index(domain) * 2 + nullable)
    n = 150
    v, mask = avu.gen_values(domain, rng, n, nullable)
    cols = [Column.from_numpy(rng.integers(0, 4, n).astype(np.int64)), Column.from_numpy(rng.integers(0, 6, n).astype(np.int64)), Column.from_numpy(v, mask)]
    lay = wu.Layout(cols, [0], [1])
    running = wu.position_states(cols[2], lay)
    for frame in wu.FRAMES:
        by_groups = wu.frame_states_by_groups(cols[2], lay, frame)
        for i in range(n):
            a, b = running[lay.frame_end(i, frame)], by_groups[i]
            assert a[0] == b[0], (frame, i)
            for x, y in zip(a[1:4], b[1:4]):  # sum (exact: fsum on both sides), min, max
                assert (math.isnan(x) and math.isnan(y)) or x == y, (frame, i, a, b)
            assert a[4] == pytest.approx(b[4], rel=1e-12), (frame, i)  # the bound: sum|x| added up in another order


def test_partition_frame_equals_the_grouped_aggregate_model():
    rng = np.random.default_rng(5)
    n = 400
    v, mask = avu.gen_values("f64_special", rng, n, True)
    key = rng.integers(0, 7, n).astype(np.int64)
    m = wu.window([Column.from_numpy(key), Column.from_numpy(v, mask)], [0], [], wu.ALL_AGGS(1, F.Partition))
    agg = avu.model_aggregate([(key, None), (v, mask)], [(AggregateFunc.Count, 1), (AggregateFunc.Sum, 1), (AggregateFunc.Min, 1), (AggregateFunc.Max, 1), (AggregateFunc.Avg, 1)], key=key)
    groups = np.unique(key)
    for j in range(5):
        per_group = dict(zip(groups.tolist(), agg.cols[j].tolist()))
        for i in range(n):
            x, y = float(m.cols[j][i]), float(per_group[int(key[i])])
            assert (math.isnan(x) and math.isnan(y)) or x == y, (j, i)


# ----------------------------------------------------------------------------- against SQLite
SQL_WORDS = ["", "a", "ab", "b", "abc", "Z", "é"]
SQL_FUNCS = {W.RowNumber: "row_number()", W.Rank: "rank()", W.DenseRank: "dense_rank()", W.Count: "count(v)", W.Sum: "sum(v)", W.Min: "min(v)", W.Max: "max(v)",
             W.Avg: "avg(v)"}
SQL_FRAMES = {F.Partition: "rows between unbounded preceding and unbounded following", F.Rows: "rows between unbounded preceding and current row",
              F.Range: "range between unbounded preceding and current row"}


def _sqlite_table(seed, n):
    rng = np.random.default_rng(seed)
    p = [None if rng.random() < 0.15 else int(x) for x in rng.integers(0, 4, n)]
    s = [None if rng.random() < 0.15 else SQL_WORDS[int(x)] for x in rng.integers(0, len(SQL_WORDS), n)]
    o = [None if rng.random() < 0.15 else int(x) for x in rng.integers(-3, 4, n)]
    v = [None if rng.random() < 0.2 else int(x) for x in rng.integers(-(1 << 40), 1 << 40, n)]
    cols = [Column.from_list(p, DType.INT64), obu.utf8_column(s), Column.from_list(o, DType.INT64), Column.from_list(v, DType.INT64)]
    db = sqlite3.connect(":memory:")
    db.execute("create table t (idx integer, p integer, s text, o integer, v integer)")
    db.executemany("insert into t values (?, ?, ?, ?, ?)", [(i, p[i], s[i], o[i], v[i]) for i in range(n)])
    return db, cols


@pytest.mark.parametrize("seed", range(6))
def test_model_agrees_with_sqlite(seed):
    assert sqlite3.sqlite_version_info >= (3, 25)  # window functions
    n = 220
    db, cols = _sqlite_table(seed, n)
    names = ["p", "s", "o", "v"]
    # (partition columns, order columns, descending): ascending puts NULLs first in both; descending puts them last in SQLite
    windows = [([0], [2], False), ([1], [2], False), ([0, 1], [2], False), ([], [2, 1], False), ([0], [], False), ([], [], False), ([1], [0, 2], False), ([0], [2], True)]
    for parts, orders, desc in windows:
        order_keys = [(c, desc, not desc) for c in orders]
        funcs = [(W.RowNumber,), (W.Rank,), (W.DenseRank,)] + [(fn, 3, fr) for fr in wu.FRAMES for fn in wu.AGGREGATES]
        m = wu.window(cols, parts, order_keys, funcs)
        counts = {fr: wu.window(cols, parts, order_keys, [(W.Count, 3, fr)]).cols[0] for fr in wu.FRAMES}
        for i, (fn, c, fr) in enumerate(m.funcs):
            stable = fn == W.RowNumber or (fn in wu.AGGREGATES and fr == F.Rows)
            order_sql = [names[c] + (" desc" if desc else "") for c in orders] + (["idx"] if stable else [])
            over = (("partition by " + ", ".join(names[c] for c in parts) + " ") if parts else "") + (("order by " + ", ".join(order_sql) + " ") if order_sql else "")
            if fn in wu.AGGREGATES:
                if fr == F.Range and not order_sql:
                    over += SQL_FRAMES[F.Partition]  # RANGE without ORDER BY: all rows are peers (SQLite wants an ORDER BY for the words)
                else:
                    over += SQL_FRAMES[fr]
            got = [r[0] for r in db.execute(f"select {SQL_FUNCS[fn]} over ({over}) from t order by idx")]
            what = f"seed {seed} window {parts} {orders} desc={desc} {fn.name} {fr.name}"
            if fn in wu.AGGREGATES and fn != W.Count:
                keep = counts[fr] > 0
                assert all(g is None for g, k in zip(got, keep) if not k), what  # SQLite: NULL over an empty frame
                g = np.array([0.0 if x is None else float(x) for x in got])
                tol = m.tols[i] if m.tols[i] is not None else None
                same = wu.same_mask(fn, g, m.cols[i].astype(np.float64), tol)
                assert same[keep].all(), f"{what}: rows {np.nonzero(~same & keep)[0][:5]}"
                if fn == W.Sum:
                    assert (g[keep] == m.cols[i][keep]).all(), what  # integers below 2^53: exact
            else:
                assert got == m.cols[i].tolist(), what
