"""Wide integers and special floats through every kernel tier of the aggregate, against the independent model of its numerics
(tests/agg_value_util.py): count exact, min / max bit for bit, sum / avg within the derived summation bound.

Every case builds its table, runs the aggregate twice (three times where the tier is only taken from the second remembered execution
on) — the later executions start from the plan hint —, compares every result with the model and asserts from the timing report that
the tier's kernels ran.  Value domains: Int64 over its whole range, Int64 in [2^61, 2^62) (sums pass 2^63), UInt64 in [2^63, 2^64),
Float64 with NaN, +-inf, +-0, subnormals, +-1e300 and groups of nothing but +inf / -inf / NaN (/ NULL, nullable variant: a column without a
validity bitmap has no NULL) whose keys lie mid-range.  `f64_special_filtered`: the Float64 domain under a range predicate on the key
column that rejects about half the rows (the shape NQE_PRED_SKIP's key-only loop takes).

Tier x domain cells that cannot be reached, and what the case asserts instead of dropping them:
  * nullable value columns.  Only the streaming kernel's VNULL instances, the un-grouped kernels, the general kernel and the merges read
    validity bitmaps (aggregate.hip, shape_pass: `vnull && partition_mode` -> not `plain`; tier_streaming: the register kernel, the
    specialised kernel, wide direct tables, direct key subsets and the single-load instance all ask `!vnull`; begin_attempt: `dense`
    asks `!any_val_nullable`).  A nullable column over the key shape of one of those tiers is served by `agg_grouped_fast` (register,
    specialised and direct-subset shapes) or by the general kernel `agg_grouped` (every partitioned shape): the nullable cases of
    those tiers run all the same and assert THAT label — the value domains reach the VNULL and general kernels at those group counts.
  * a range test on the key column drops the groups it rejects, and under a predicate no key sample is taken: the streaming attempt must
    overflow a workgroup table before the measured range picks the tier.  The filtered case of `subsets_direct` and `partitioned_range`
    therefore has a key column of its own (FILTERED_TIERS: twice the keys, 3 million rows) and IS asserted in its tier.  That of `two_levels`
    (2.6 -> 1.3 million groups, at most 1.5 million kept rows: 512 partitions are never overfull) runs in one partition level — asserted as such.
  * the value column being the key column has no domain of its own: its two cases take wide Int64 and UInt64 keys instead.  `val_shares_key`
    has no label and no other observable: the cases pin the tier and that every group's min, max and avg is its converted key.
  * labels are per launch site, not per kernel instance: `subsets_hashed` shows what `one_table_hashed` shows, the 12- and 16-byte tuple forms
    and both block-scatter forms show `agg_partition_scatter` alone.  The key shapes are those of the tests that introduced the forms; which
    instance ran is not observable here.
  * groups of nothing but +inf / -inf / NaN / NULL need six groups or more to sit mid-range; tiers of four groups or fewer (the register
    kernel, `id % 2`) carry the all -inf group alone, one group none.
aggregate/mod.rs:113-222, count.rs, sum.rs, avg.rs, min.rs, max.rs"""
import dataclasses
import functools

import numpy as np
import pytest

from naive_query_engine_amd import AggregateFunc, Column, DType, Operator
from naive_query_engine_amd.expression import binop, col, lit_i64, lit_u64
from tests.agg_value_util import (ALL_AGGS, DOMAINS, VARIANT_IDS, VARIANTS, assert_matches_model, gen_values, interior_keys, model_aggregate,
                                  plant_only_groups)
from tests.helpers import fields

pytestmark = pytest.mark.gpu

FLD = fields("k", "a", "b", "c")
X, O = binop, Operator
CASES = VARIANTS + [("f64_special", "filtered")]
CASE_IDS = VARIANT_IDS + ["f64_special_filtered"]


@pytest.fixture(scope="module")
def ctx():
    from naive_query_engine_amd import capi

    c = capi.Context(0)
    yield c
    c.close()


@dataclasses.dataclass
class Shape:
    """one tier's key shape"""
    kcol: np.ndarray                    # the key source column
    key_expr: object                    # the key expression over it
    key_np: np.ndarray                  # the same expression in numpy: the group key of every row
    want: dict                          # label -> launches the timing report must show: `agg_grouped_fast` exactly that many (an abandoned
                                        # attempt and its redo are two), the partitioned path's kernels at least (its two-level and fall-back
                                        # forms scatter twice by design)
    forbid: tuple = ()                  # labels it must not show
    want_null: dict = None              # the same two for the nullable variants (default: `want`, nothing forbidden)
    forbid_null: tuple = ()
    want_filt: dict = None              # labels of the filtered case where the filter moves the query to another tier
    filt: tuple = None                  # the filtered case's (predicate, rows it keeps)
    pred: tuple = None                  # a predicate of every case
    env: dict = dataclasses.field(default_factory=dict)
    reps: int = 2                       # executions
    check_from: int = 1                 # the first execution whose labels are asserted
    jit: bool = False                   # wait for the specialised kernel after the first execution
    one_pass: bool = True               # False: one streaming pass per value column, so `agg_grouped_fast` runs at least `want` times

    def __post_init__(self):
        if self.want_null is None:
            self.want_null = self.want


def _median_filter(k, lit=lit_i64):
    """`k < median`: a range test on the key column itself, about half the rows"""
    c = int(np.sort(k)[len(k) // 2])
    return X(col(0), O.Lt, lit(c)), k < k.dtype.type(c)


def _mod(k, m):
    return np.fmod(k, np.int64(m)) if k.dtype == np.int64 else k % np.uint64(m)


# --------------------------------------------------------------------------- the tiers
def _tiny(m):
    def make():
        rng = np.random.default_rng(100 + m)
        n = (1 << 20) + 777                                       # the register kernel is taken from 2^20 rows on
        ids = rng.integers(0, 1 << 40, n).astype(np.int64)
        return Shape(ids, X(col(0), O.Modulos, lit_i64(m)), _mod(ids, m), {"agg_grouped_tiny": 1}, want_null={"agg_grouped_fast": 1}, forbid_null=("agg_grouped_tiny",),
                     filt=(X(col(0), O.Lt, lit_i64(1 << 39)), ids < (1 << 39)), check_from=0)
    return make


def _replicated(m):
    def make():
        n = 300_007
        ids = (np.arange(n, dtype=np.int64) - n // 3) * (1 if m % 2 else 3)
        c = int(ids[n // 2])
        return Shape(ids, X(col(0), O.Modulos, lit_i64(m)), _mod(ids, m), {"agg_grouped_fast": 1}, forbid=("agg_partition_scatter", "agg_grouped"), forbid_null=("agg_partition_scatter",),
                     filt=(X(col(0), O.Lt, lit_i64(c)), ids < c), check_from=0)
    return make


def _plain(n, draw, want, forbid=(), unsigned=False, key_mod=None, **shape_args):
    def make():
        rng = np.random.default_rng(n % 9973 + len(want))
        k = draw(rng, n)
        k = k.astype(np.uint64) if unsigned else k.astype(np.int64)
        lit = lit_u64 if unsigned else lit_i64
        key_expr, key_np = (col(0), k) if key_mod is None else (X(col(0), O.Modulos, lit(key_mod)), _mod(k, key_mod))
        return Shape(k, key_expr, key_np, want, forbid, filt=_median_filter(k, lit), **shape_args)
    return make


GENERAL_NULL = {"agg_grouped": 1}        # the general kernel: what a nullable column over a partitioned key shape is served by
NO_PART = ("agg_partition_scatter",)
PART = {"agg_partition_scatter": 1}
ONE_TABLE = {"agg_grouped_fast": 1}
RANGE_PART = {"agg_partition_scatter": 1, "agg_segments_direct": 1}


def _jit():
    n = 70_001
    ids = np.arange(n, dtype=np.int64) - n // 3
    # (key `(id + 1) % 1000`: an interpreted chain key takes the specialised kernel whatever the predicate — none, or the filtered case's range test)
    key = X(X(col(0), O.Plus, lit_i64(1)), O.Modulos, lit_i64(1000))
    return Shape(ids, key, _mod(ids + 1, 1000), {"agg_grouped_jit": 1}, forbid=("agg_grouped_fast", "agg_grouped"), want_null={"agg_grouped_fast": 1}, forbid_null=("agg_grouped_jit",),
                 filt=(X(col(0), O.Lt, lit_i64(n // 2 - n // 3)), ids < n // 2 - n // 3), env={"NQE_JIT_MIN_ROWS": "1000"}, jit=True)


def _general():
    rng = np.random.default_rng(50)
    n = 50_000
    ids = rng.permutation(n).astype(np.int64) + 1
    # a literal-on-the-left division can fault: the general kernel.  (C division of positive operands: floor)
    key = X(X(lit_i64(1_000_000), O.Divide, col(0)), O.Modulos, lit_i64(7))
    c = n // 2
    return Shape(ids, key, (1_000_000 // ids) % 7, {"agg_grouped": 1}, forbid=("agg_grouped_fast",), filt=(X(col(0), O.Lt, lit_i64(c)), ids < c), check_from=0)


TIERS = {
    "register_m1": _tiny(1), "register_m3": _tiny(3), "register_m4": _tiny(4),
    "replicated_m2": _replicated(2), "replicated_m512": _replicated(512), "replicated_m2047": _replicated(2047),
    # one workgroup table: addressed by key - min (dense_4096) and hashed (sparse_3000)
    "one_table_direct": _plain(400_000, lambda r, n: r.integers(100, 4196, n), {"agg_grouped_fast": 1}, NO_PART, forbid_null=NO_PART),
    "one_table_hashed": _plain(400_000, lambda r, n: r.integers(0, 3000, n) * 1_000_003 - 5, {"agg_grouped_fast": 1}, NO_PART, forbid_null=NO_PART),
    # hashed partitions whose densely written table is ranked by key - min
    "dense_rank_tail": _plain(600_000, lambda r, n: r.integers(0, 70_000, n) * 5 - 1234, {"agg_partition_scatter": 1, "agg_segments": 1, "agg_dense_rank_emit": 1},
                              want_null=GENERAL_NULL, env={"NQE_NO_RANGE_PARTITION": "1"}, check_from=0),
    # two key subsets: the halves of a measured range (dense_6000), hashed (5000 groups no table addresses directly)
    "subsets_direct": _plain(1_000_000, lambda r, n: r.integers(-2000, 4000, n), {"agg_grouped_fast": 1, "agg_fold_partials": 1, "agg_range_emit": 1}, NO_PART,
                             want_null=GENERAL_NULL, reps=3, check_from=2, want_filt=ONE_TABLE),
    "subsets_hashed": _plain(700_000, lambda r, n: r.integers(0, 5000, n) * 1_000_033 - 77, {"agg_grouped_fast": 1}, NO_PART, want_null=GENERAL_NULL),
    "partitioned_hashed": _plain(700_000, lambda r, n: r.integers(0, 20_000, n) * 1_000_033 - 77, {"agg_partition_scatter": 1, "agg_segments": 1}, ("agg_segments_direct",),
                                 want_null=GENERAL_NULL, check_from=0),
    "partitioned_range": _plain(700_000, lambda r, n: r.integers(0, 6000, n) * 7 + 11, RANGE_PART, want_null=GENERAL_NULL, reps=3, check_from=1),
    "tuples12_small": _plain(600_000, lambda r, n: r.integers(0, 70_000, n), PART, want_null=GENERAL_NULL, env={"NQE_NO_RANGE_PARTITION": "1"}, check_from=0),
    "tuples16_one_wide": _plain(600_000, lambda r, n: np.concatenate([r.integers(0, 70_000, n - 1), [1 << 31]]), PART, want_null=GENERAL_NULL, env={"NQE_NO_RANGE_PARTITION": "1"},
                                reps=3, check_from=0),
    "two_levels": _plain(3_000_000, lambda r, n: r.integers(0, 2_600_000, n) * 3 - 2_600_000, {"agg_partition_scatter": 1, "agg_subpartition": 1, "agg_segments": 1}, want_null=GENERAL_NULL,
                         check_from=0, want_filt={"agg_partition_scatter": 1, "agg_segments": 1}),
    "block_scatter_range": _plain(3_000_000, lambda r, n: r.integers(0, 2_000_000, n) + 7_000_000_000, PART, want_null=GENERAL_NULL, check_from=0),
    "block_scatter_mod_key": _plain(900_000, lambda r, n: r.integers(-(1 << 40), 1 << 40, n), PART, want_null=GENERAL_NULL, check_from=0, key_mod=70_001),
    "specialised_streaming": _jit,
    "general": _general,
}


# the filtered case of a tier whose own key column the range test would move into the tier below: a key column of its own, twice the keys
FILTERED_TIERS = {
    # 8000 consecutive keys under `k < median`, 3 million rows: every workgroup meets more than 3072 of the 4000 kept keys in its hashed table and
    # gives up; the measured range (8000 values, at most two tables' worth) goes to two key subsets addressed by key - min
    "subsets_direct": _plain(3_000_000, lambda r, n: r.integers(-3000, 5000, n), {"agg_grouped_fast": 1, "agg_fold_partials": 1, "agg_range_emit": 1}, NO_PART, reps=3, check_from=2),
    # 12 000 keys x 7 under `k < median`, 3 million rows: every workgroup of the streaming attempt meets some 3700 of the 6000 kept keys, more than
    # three quarters of its 4096 slots, and gives up; the measured range (84 000 values) then goes to the range tier in that execution already
    "partitioned_range": _plain(3_000_000, lambda r, n: r.integers(0, 12_000, n) * 7 + 11, RANGE_PART, check_from=0),
}


@functools.lru_cache(maxsize=2)
def shape_of(tier, filtered=False):
    return (FILTERED_TIERS.get(tier, TIERS[tier]) if filtered else TIERS[tier])()


def plant(v, mask, domain, key, keep):
    if domain != "f64_special":
        return
    groups = len(np.unique(key if keep is None else key[keep]))
    if groups >= 6:
        plant_only_groups(v, mask, key, *interior_keys(key, keep))
    elif groups >= 2:
        v[key == interior_keys(key, keep)[0]] = -np.inf


def run(ctx, monkeypatch, shape, table, aggs, nullable, filtered, what):
    """the executions of one case: each against the model, the labels from `check_from` on"""
    for name, value in shape.env.items():
        monkeypatch.setenv(name, value)
    pred, keep = shape.filt if filtered else (shape.pred if shape.pred is not None else (None, None))
    model = model_aggregate(table, aggs, key=shape.key_np, keep=keep)
    t = ctx.table_from_host([Column.from_numpy(v, m) for v, m in table])
    kn = shape.key_expr.flatten(FLD)
    pn = pred.flatten(FLD) if pred is not None else None
    want, forbid = (shape.want_null, shape.forbid_null) if nullable else (shape.want, shape.forbid)
    if filtered and shape.want_filt is not None:
        want, forbid = shape.want_filt, ()
    for rep in range(shape.reps):
        ctx.timing_enable(True)
        ctx.timing_reset()
        got = ctx.aggregate(t, aggs, group_nodes=kn, pred_nodes=pn).to_host()
        ctx.timing_enable(False)
        names = ctx.timing_report()
        assert_matches_model(got, model, what=f"{what} execution {rep}")
        if shape.jit and rep == 0:
            ctx.jit_wait()
        if rep >= shape.check_from:
            for label, count in want.items():
                ran = names.get(label, (0, 0))[1]
                exact = label == "agg_grouped_fast" and (shape.one_pass or not nullable)
                assert ran == count if exact else ran >= count, f"{what} execution {rep}: {label} ran {ran} times, expected {count}: {sorted(names)}"
            for label in forbid:
                assert label not in names, f"{what} execution {rep}: {label} ran: {sorted(names)}"
    return model


@pytest.mark.parametrize("domain,variant", CASES, ids=CASE_IDS)
@pytest.mark.parametrize("tier", list(TIERS))
def test_value_domains_one_value_column(ctx, monkeypatch, tier, domain, variant):
    nullable, filtered = variant is True, variant == "filtered"
    shape = shape_of(tier, filtered)
    rng = np.random.default_rng(len(tier) * 131 + CASES.index((domain, variant)))
    v, mask = gen_values(domain, rng, len(shape.kcol), nullable)
    keep = shape.filt[1] if filtered else (shape.pred[1] if shape.pred is not None else None)
    plant(v, mask, domain, shape.key_np, keep)
    run(ctx, monkeypatch, shape, [(shape.kcol, None), (v, mask)], ALL_AGGS(1), nullable, filtered, f"{tier} {domain} {variant}")


# --------------------------------------------------------------------------- two and three value columns in one pass
@pytest.mark.parametrize("domain,nullable", VARIANTS, ids=VARIANT_IDS)
@pytest.mark.parametrize("ncols", [2, 3])
def test_value_domains_two_and_three_value_columns_in_one_pass(ctx, monkeypatch, ncols, domain, nullable):
    """one column from each of three different domains (the case's own first): two columns with all five aggregates each, three in the
    three-column instance's shape — count, sum, and sum / avg / min / max of the last.  700 groups, one launch; nullable columns go one per pass"""
    rng = np.random.default_rng(4242 + ncols + 10 * VARIANTS.index((domain, nullable)))
    n, groups = 300_011, 700
    k = rng.integers(-(groups // 2), groups - groups // 2, n).astype(np.int64)
    doms = [DOMAINS[(DOMAINS.index(domain) + j) % len(DOMAINS)] for j in range(ncols)]
    table = [(k, None)]
    for d in doms:
        v, mask = gen_values(d, rng, n, nullable)
        plant(v, mask, d, k, None)
        table.append((v, mask))
    if ncols == 2:
        aggs = ALL_AGGS(1) + ALL_AGGS(2)
    else:
        A = AggregateFunc
        aggs = [(A.Count, 1), (A.Sum, 1), (A.Sum, 2), (A.Avg, 2), (A.Sum, 3), (A.Avg, 3), (A.Max, 3), (A.Min, 3), (A.Count, 3)]
    shape = Shape(k, col(0), k, {"agg_grouped_fast": 1}, NO_PART, forbid_null=NO_PART, one_pass=False)
    for rep_pred in (None, _median_filter(k)):
        shape.pred = rep_pred
        run(ctx, monkeypatch, shape, table, aggs, nullable, False, f"{ncols} columns {doms} nullable={nullable} pred={rep_pred is not None}")


# --------------------------------------------------------------------------- un-grouped
@pytest.mark.parametrize("domain,variant", CASES, ids=CASE_IDS)
@pytest.mark.parametrize("kernel", ["agg_ungrouped_fast", "agg_ungrouped"])
def test_value_domains_ungrouped(ctx, kernel, domain, variant):
    """`agg_ungrouped_fast` (no predicate; filtered case: the range test `w < 0`) and the general `agg_ungrouped`, which only runs under a
    predicate the fast kernel does not take: the chain `w % 7 >= 2` in every case, so its filtered case is one more draw of the Float64 domain
    under the same predicate (a conjunction with a range test is evaluated into a bitmap that the fast kernel takes).  Both behind
    `agg_ungrouped_fold`; two value columns in one pass"""
    nullable, filtered = variant is True, variant == "filtered"
    rng = np.random.default_rng(8 + CASES.index((domain, variant)))
    n = 300_000
    w = rng.integers(-50, 50, n).astype(np.int64)
    v, mask = gen_values(domain, rng, n, nullable)
    other = DOMAINS[(DOMAINS.index(domain) + 2) % len(DOMAINS)]
    v2, mask2 = gen_values(other, rng, n, nullable)
    table = [(w, None), (v, mask), (v2, mask2)]
    if kernel == "agg_ungrouped":
        pred, keep = X(X(col(0), O.Modulos, lit_i64(7)), O.GtEq, lit_i64(2)), np.fmod(w, 7) >= 2
    elif filtered:
        pred, keep = X(col(0), O.Lt, lit_i64(0)), w < 0
    else:
        pred, keep = None, None
    aggs = ALL_AGGS(1) + ALL_AGGS(2)
    model = model_aggregate(table, aggs, keep=keep)
    t = ctx.table_from_host([Column.from_numpy(a, m) for a, m in table])
    pn = pred.flatten(FLD) if pred is not None else None
    for rep in range(2):
        ctx.timing_enable(True)
        ctx.timing_reset()
        got = ctx.aggregate(t, aggs, pred_nodes=pn).to_host()
        ctx.timing_enable(False)
        names = ctx.timing_report()
        assert_matches_model(got, model, what=f"un-grouped {kernel} {domain} {variant} execution {rep}")
        assert kernel in names and "agg_ungrouped_fold" in names, sorted(names)


# --------------------------------------------------------------------------- partial states and their merges
@pytest.mark.parametrize("domain,variant", CASES, ids=CASE_IDS)
@pytest.mark.parametrize("grouped", [True, False])
def test_value_domains_partial_states_merged(ctx, grouped, domain, variant):
    """three unequal parts -> nqe_aggregate_partial each (`agg_fold_partials` behind the direct-mapped table of `id % 100`) -> merged by
    nqe_aggregate_merge (`agg_merge_states`) and, packed into one buffer as the exchange ships them, by nqe_aggregate_merge_packed
    (`agg_merge_packed`): both equal the model over all the rows"""
    nullable, filtered = variant is True, variant == "filtered"
    rng = np.random.default_rng(99 + CASES.index((domain, variant)))
    n = 40_000
    ids = rng.permutation(n).astype(np.int64) - n // 4
    v, mask = gen_values(domain, rng, n, nullable)
    key_np = _mod(ids, 100)
    pred, keep = (X(col(0), O.Lt, lit_i64(n // 4)), ids < n // 4) if filtered else (None, None)
    plant(v, mask, domain, key_np, keep)
    table = [(ids, None), (v, mask)]
    aggs = ALL_AGGS(1)
    kn = X(col(0), O.Modulos, lit_i64(100)).flatten(FLD) if grouped else None
    pn = pred.flatten(FLD) if pred is not None else None
    model = model_aggregate(table, aggs, key=key_np if grouped else None, keep=keep)
    states, keys = [], []
    ctx.timing_enable(True)
    ctx.timing_reset()
    for lo, hi in [(0, 13_000), (13_000, 13_001), (13_001, n)]:
        sub = [Column.from_numpy(a[lo:hi], None if m is None else m[lo:hi]) for a, m in table]
        st, sk = ctx.aggregate_partial(ctx.table_from_host(sub), aggs, group_nodes=kn, pred_nodes=pn)
        states.append(st), keys.append(sk)
    merged, _ = ctx.aggregate_merge(states, keys if grouped else None, aggs)
    ctx.timing_enable(False)
    names = ctx.timing_report()
    assert "agg_merge_states" in names, sorted(names)
    if grouped and not nullable:
        assert "agg_fold_partials" in names, sorted(names)
    assert_matches_model(merged.to_host(), model, what=f"merged partial states, {domain} {variant} grouped={grouped}")
    # the same parts as the exchange ships them: [key column] + {count, sum, min, max}, `stride` words per column, + the row count
    ncols = (1 if grouped else 0) + 4
    stride = max(s.num_rows for s in states) + 3
    buf = ctx.device_alloc(len(states) * (ncols * stride + 1) * 8)
    try:
        for p, (st, sk) in enumerate(zip(states, keys)):
            ctx.pack_words(([sk] if grouped else []) + [st], stride, buf + p * (ncols * stride + 1) * 8)
        ctx.timing_enable(True)
        ctx.timing_reset()
        out = ctx.aggregate_merge_packed(buf, len(states), stride, grouped, DType.INT64, aggs)
        ctx.timing_enable(False)
        assert out is not None and "agg_merge_packed" in ctx.timing_report(), sorted(ctx.timing_report())
        assert_matches_model(out[0].to_host(), model, what=f"packed partial states, {domain} {variant} grouped={grouped}")
    finally:
        ctx.synchronize()
        ctx.device_free(buf)


# --------------------------------------------------------------------------- the value column is the key column
@pytest.mark.parametrize("tier", ["one_table_hashed", "partitioned_hashed"])
@pytest.mark.parametrize("keys", ["i64_wide", "u64_high"])
def test_value_domains_value_column_is_the_key_column(ctx, monkeypatch, keys, tier):
    """`count(k), sum(k), avg(k), min(k), max(k) … group by k` over wide keys (val_shares_key: the key word is the value word; nothing reports that it engaged): 3000 distinct
    keys in one hashed workgroup table, 20 000 in hashed partitions — every group's min, max and avg is its key converted as Q10 says"""
    rng = np.random.default_rng(len(keys) + len(tier))
    n, distinct = (400_000, 3000) if tier == "one_table_hashed" else (700_000, 20_000)
    base, _ = gen_values(keys, rng, 4 * distinct, False)
    base = np.unique(base)[:distinct]
    k = base[rng.integers(0, len(base), n)]
    k[:len(base)] = base
    if tier == "one_table_hashed":
        shape = Shape(k, col(0), k, {"agg_grouped_fast": 1}, NO_PART)
    else:
        shape = Shape(k, col(0), k, {"agg_partition_scatter": 1, "agg_segments": 1}, check_from=0)
    model = run(ctx, monkeypatch, shape, [(k, None)], ALL_AGGS(0), False, False, f"value is key, {keys}, {tier}")
    assert model.rows == len(base)
    assert (np.sort(model.cols[3]) == np.sort(base.astype(np.float64))).all()
