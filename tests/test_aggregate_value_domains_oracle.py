"""The CPU oracle against the independent model of the aggregate functions' numerics (tests/agg_value_util.py) on the value
domains the device suite uses: Int64 over its whole range, Int64 sums that pass 2^63, UInt64 beyond 2^63, Float64 with NaN, +-inf,
+-0, subnormals and groups of nothing but +inf / -inf / NaN / NULL — 20 000 rows, 1 / 7 / 3000 groups and un-grouped, one and two value
columns.  Two things are checked: the oracle stays inside the model's derived sum bound, and its Q10 edge semantics are the model's
(count.rs, sum.rs, avg.rs, min.rs, max.rs; aggregate/mod.rs:113-222)."""
import numpy as np
import pytest

from naive_query_engine_amd import Column
from naive_query_engine_amd.expression import col
from oracle import oracle as orc
from tests.agg_value_util import ALL_AGGS, DOMAINS, VARIANT_IDS, VARIANTS, assert_matches_model, gen_values, interior_keys, model_aggregate, plant_only_groups
from tests.helpers import fields

N = 20_000
FLD = fields("k", "a", "b")


def build(domain, nullable, groups, seed):
    rng = np.random.default_rng(seed)
    key = rng.integers(0, groups, N).astype(np.int64) * 1_000_003 - 7 * groups
    key_mask = (rng.random(N) >= 0.05) if nullable else None     # NULL keys are dropped
    a, am = gen_values(domain, rng, N, nullable)
    other = DOMAINS[(DOMAINS.index(domain) + 1) % len(DOMAINS)]
    b, bm = gen_values(other, rng, N, nullable)
    if groups >= 6:
        for v, m, d in ((a, am, domain), (b, bm, other)):
            if d == "f64_special":
                plant_only_groups(v, m, key, *interior_keys(key))
    return key, key_mask, [(key, key_mask), (a, am), (b, bm)]


@pytest.mark.parametrize("two_columns", [False, True])
@pytest.mark.parametrize("groups", [0, 1, 7, 3000])          # 0: un-grouped
@pytest.mark.parametrize("domain,nullable", VARIANTS, ids=VARIANT_IDS)
def test_oracle_agrees_with_the_model(domain, nullable, groups, two_columns):
    key, key_mask, table = build(domain, nullable, max(groups, 1), 1000 * groups + 10 * DOMAINS.index(domain) + int(nullable))
    cols = [Column.from_numpy(v, m) for v, m in table]
    aggs = ALL_AGGS(1) + (ALL_AGGS(2) if two_columns else [])
    if groups:
        got = orc.aggregate([cols], aggs, group_nodes=col(0).flatten(FLD))[0]
        model = model_aggregate(table, aggs, key=key, key_mask=key_mask)
    else:
        got = orc.aggregate([cols], aggs)[0]
        model = model_aggregate(table, aggs)
    assert_matches_model(got, model, what=f"oracle, {domain} nullable={nullable} groups={groups}")


def test_model_states_the_edges():
    """the model itself on hand-written rows: what Q10 means for 2^63 + 1, for a sum that mixes +inf and NaN, for the "only" groups"""
    from naive_query_engine_amd import AggregateFunc as A

    fmax = np.finfo(np.float64).max
    u = np.array([(1 << 63) + 1, (1 << 64) - 1, (1 << 53) + 1], dtype=np.uint64)
    m = model_aggregate([(u, None)], ALL_AGGS(0))
    assert m.cols[0][0] == 3 and m.cols[3][0] == 2.0 ** 53 and m.cols[4][0] == 2.0 ** 64      # 2^53 + 1 rounds to even, 2^64 - 1 up
    assert m.cols[1][0] == 2.0 ** 63 + 2.0 ** 64 + 2.0 ** 53
    i = np.array([(1 << 62), (1 << 62), (1 << 62)], dtype=np.int64)                           # 3 x 2^62 wraps in int64, not in f64
    assert model_aggregate([(i, None)], [(A.Sum, 0)]).cols[0][0] == 3 * 2.0 ** 62
    k = np.array([0, 0, 1, 1, 2, 3, 4, 4], dtype=np.int64)
    v = np.array([np.inf, np.nan, np.inf, -np.inf, np.inf, -np.inf, 1.0, 2.0])
    mask = np.array([1, 1, 1, 1, 1, 1, 0, 0], dtype=bool)
    m = model_aggregate([(k, None), (v, mask)], ALL_AGGS(1), key=k)
    cnt, s, avg, mn, mx = m.cols
    assert cnt.tolist() == [2, 2, 1, 1, 0]
    assert np.isnan(s[0]) and np.isnan(s[1]) and s[2] == np.inf and s[3] == -np.inf and s[4] == 0.0
    assert np.isnan(avg[4]) and avg[2] == np.inf
    assert mn.tolist() == [fmax, -np.inf, fmax, -np.inf, fmax]                               # NaN ignored; +inf alone keeps f64::MAX
    assert np.isnan(mx[0]) and mx[1:].tolist() == [np.inf, np.inf, -fmax, -fmax]             # -inf alone keeps f64::MIN
