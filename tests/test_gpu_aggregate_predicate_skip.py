"""The streaming aggregate's key-only loop (NQE_PRED_SKIP, aggregate_fast_kernel.hpp): a wave that meets a tile none of whose rows
pass a range predicate reads only the tested words until a tile with a passing row comes up.  Every limit around the tile and wave
boundaries, every comparison operator, Int64 and UInt64 keys, the key shapes, one or two value columns, a predicate on another
column, and poisoned values in the filtered-out rows — against float64 numpy over the same host columns: counts, min and max
exact, sums and averages within 1e-9 relative."""
import numpy as np
import pytest

from naive_query_engine_amd import AggregateFunc, Column, Operator
from naive_query_engine_amd.expression import binop, col, lit_i64, lit_u64
from tests.helpers import fields

pytestmark = pytest.mark.gpu

RTOL = 1e-9
N = 1 << 24
SIZES = [N, N + 13]
OPS = {Operator.Lt: np.less, Operator.LtEq: np.less_equal, Operator.Gt: np.greater, Operator.GtEq: np.greater_equal,
       Operator.Eq: np.equal, Operator.NotEq: np.not_equal}
ALL = lambda c: [(AggregateFunc.Count, c), (AggregateFunc.Sum, c), (AggregateFunc.Avg, c), (AggregateFunc.Min, c), (AggregateFunc.Max, c)]


@pytest.fixture(scope="module")
def ctx():
    from naive_query_engine_amd import capi

    c = capi.Context(0)
    yield c
    c.close()


def limits(n):
    return sorted({0, 1, 63, 64, 65, 4095, 4096, 4097, n // 2, n - 1, n})


class Groups:
    """the group structure of one key column, computed once: expected() then costs a few passes per predicate"""

    def __init__(self, keys):
        self.uk, self.inv = np.unique(keys, return_inverse=True)
        self.order = np.argsort(self.inv, kind="stable")
        self.starts = np.searchsorted(self.inv[self.order], np.arange(len(self.uk)))
        self.sorted = {}  # id(value column) -> (column, its float64 image in group order)

    def expected(self, mask, vals):
        """{key: [(count, sum, min, max) per value column]} over the passing rows, float64"""
        g = len(self.uk)
        cnt = np.bincount(self.inv, weights=mask, minlength=g).astype(np.int64)
        ms = mask[self.order]
        per = []
        for v in vals:
            x = v.astype(np.float64)
            s = np.bincount(self.inv, weights=np.where(mask, x, 0.0), minlength=g)
            if id(v) not in self.sorted:
                self.sorted[id(v)] = (v, x[self.order])
            xs = self.sorted[id(v)][1]
            mn = np.minimum.reduceat(np.where(ms, xs, np.inf), self.starts)
            mx = np.maximum.reduceat(np.where(ms, xs, -np.inf), self.starts)
            per.append((s, mn, mx))
        return {int(self.uk[i]): [(int(cnt[i]), p[0][i], p[1][i], p[2][i]) for p in per] for i in np.nonzero(cnt)[0]}


def check(ctx, t, nv, key_node, pred_node, exp, what):
    aggs = [a for j in range(nv) for a in ALL(1 + j)]
    out, keys = ctx.aggregate(t, aggs, group_nodes=key_node, pred_nodes=pred_node, with_keys=True)
    cols = [c.to_numpy() for c in out.to_host()]
    got_keys = keys.to_host()[0].to_numpy() if keys is not None else np.zeros(0, np.int64)
    assert len(got_keys) == len(exp), f"{what}: {len(got_keys)} groups, expected {len(exp)}"
    for r, key in enumerate(got_keys.tolist()):
        assert key in exp, f"{what}: unexpected group {key}"
        for j in range(nv):
            cnt, s, mn, mx = exp[key][j]
            c = cols[5 * j:5 * j + 5]
            assert int(c[0][r]) == cnt, f"{what}: count of group {key}, column {j}"
            assert np.isclose(c[1][r], s, rtol=RTOL, atol=0), f"{what}: sum of group {key}, column {j}: {c[1][r]} vs {s}"
            assert np.isclose(c[2][r], s / cnt, rtol=RTOL, atol=0), f"{what}: avg of group {key}, column {j}"
            assert c[3][r] == mn and c[4][r] == mx, f"{what}: min / max of group {key}, column {j}"


def lit_for(unsigned, k):
    return lit_u64(k) if unsigned else lit_i64(k)


@pytest.mark.timeout(900)
@pytest.mark.parametrize("unsigned", [False, True])
@pytest.mark.parametrize("n", SIZES)
def test_row_number_ids_every_limit_and_operator(ctx, n, unsigned):
    """`select … where id OP K group by id % 1024` over ids = row numbers: the headline's shape, K at every boundary"""
    rng = np.random.default_rng(n + unsigned)
    ids = np.arange(n, dtype=np.uint64 if unsigned else np.int64)
    v = rng.random(n) * 100.0
    t = ctx.table_from_host([Column.from_numpy(ids), Column.from_numpy(v)])
    f = fields("id", "v")
    key = binop(col(0), Operator.Modulos, lit_for(unsigned, 1024)).flatten(f)
    grp = Groups((ids % 1024).astype(np.int64))
    for k in limits(n):
        for op, fn in OPS.items():
            mask = fn(ids, ids.dtype.type(k))
            check(ctx, t, 1, key, binop(col(0), op, lit_for(unsigned, k)).flatten(f), grp.expected(mask, [v]), f"id {op} {k}, n={n}")


@pytest.mark.timeout(900)
@pytest.mark.parametrize("n", SIZES)
def test_key_and_value_shapes(ctx, n):
    """a plain key column in direct-mapped range, a hashed key, Int64 values, two value columns"""
    rng = np.random.default_rng(n)
    ids = np.arange(n, dtype=np.int64)
    small = rng.integers(-300, 300, n).astype(np.int64)
    wide = rng.integers(0, 1 << 40, n).astype(np.int64) % 3000 * 1000003
    v = rng.random(n) * 200.0 - 100.0
    iv = rng.integers(-(1 << 40), 1 << 40, n).astype(np.int64)
    f = fields("id", "v", "w")
    gid, gsmall, gwide = Groups(ids % 1024), Groups(small), Groups(wide)
    for lim, op in ((n // 3, Operator.Lt), (n - n // 5, Operator.GtEq), (4097, Operator.LtEq)):
        mask = OPS[op](ids, lim)
        pred = binop(col(0), op, lit_i64(lim)).flatten(f)
        # key = id % 1024 with Int64 values; two value columns
        t = ctx.table_from_host([Column.from_numpy(ids), Column.from_numpy(iv), Column.from_numpy(v)])
        key = binop(col(0), Operator.Modulos, lit_i64(1024)).flatten(f)
        check(ctx, t, 1, key, pred, gid.expected(mask, [iv]), f"Int64 values, id {op} {lim}")
        check(ctx, t, 2, key, pred, gid.expected(mask, [iv, v]), f"two value columns, id {op} {lim}")
        # the key is another column: the predicate goes on the id column (PRED 2), plain key in direct range / hashed
        for kc, grp, what in ((small, gsmall, "direct key"), (wide, gwide, "hashed key")):
            t = ctx.table_from_host([Column.from_numpy(ids), Column.from_numpy(v), Column.from_numpy(kc)])
            check(ctx, t, 1, col(2).flatten(f), pred, grp.expected(mask, [v]), f"{what}, id {op} {lim}")


@pytest.mark.timeout(900)
@pytest.mark.parametrize("n", SIZES)
def test_random_ids_nothing_skipped(ctx, n):
    rng = np.random.default_rng(n + 7)
    ids = rng.permutation(n).astype(np.int64)
    v = rng.random(n) * 100.0
    t = ctx.table_from_host([Column.from_numpy(ids), Column.from_numpy(v)])
    f = fields("id", "v")
    key = binop(col(0), Operator.Modulos, lit_i64(1024)).flatten(f)
    grp = Groups(ids % 1024)
    for lim in (1, 4096, n // 2, n):
        mask = ids < lim
        check(ctx, t, 1, key, binop(col(0), Operator.Lt, lit_i64(lim)).flatten(f), grp.expected(mask, [v]), f"random ids < {lim}")


@pytest.mark.timeout(900)
@pytest.mark.parametrize("n", SIZES)
def test_poison_in_filtered_out_rows(ctx, n):
    """NaN, ±inf and ±DBL_MAX in every row the predicate rejects: they must not reach any statistic"""
    rng = np.random.default_rng(n + 11)
    ids = np.arange(n, dtype=np.int64)
    v = rng.random(n) * 100.0
    poison = np.array([np.nan, np.inf, -np.inf, np.finfo(np.float64).max, -np.finfo(np.float64).max])
    f = fields("id", "v")
    key = binop(col(0), Operator.Modulos, lit_i64(1024)).flatten(f)
    grp = Groups(ids % 1024)
    for lim, op in ((n // 2, Operator.Lt), (n // 2, Operator.GtEq), (65, Operator.Lt), (n - 1, Operator.GtEq)):
        mask = OPS[op](ids, lim)
        vp = v.copy()
        vp[~mask] = poison[rng.integers(0, len(poison), int((~mask).sum()))]
        t = ctx.table_from_host([Column.from_numpy(ids), Column.from_numpy(vp)])
        check(ctx, t, 1, key, binop(col(0), op, lit_i64(lim)).flatten(f), grp.expected(mask, [v]), f"poisoned, id {op} {lim}")
