"""Pins the aggregate's dispatch: for a key shape of every kernel tier (plain, with a nullable value column, under a filter) and for the
query shapes that take a path of their own, the kernels launched — every label of the context's timing report with its launch count —
by each of THREE executions (two cases: by the second and third), and every execution's result against the model of tests/agg_value_util.py.  Three executions show the
ladder (an abandoned attempt launches its kernels too), the start the context recalls for the query shape, and that the recall is stable.
The expected launches are data: tests/golden/aggregate_paths.json, recorded once (python -m tests.test_gpu_aggregate_paths --record,
which refuses to overwrite an existing file) from the library as it was before the aggregate's host code was split into named steps
around one plan memo; the test only ever reads it.

Every case runs in a context of its own: what a context remembers of a query shape is keyed by buffer address, and its block pool
hands addresses out again, so cases sharing one context would see each other.  The value columns are Int64 of small integers (every
sum is exact) under all five aggregates unless the case says otherwise."""
import contextlib
import dataclasses
import json
import os
import sys

import numpy as np
import pytest

from naive_query_engine_amd import AggregateFunc, Column, DType, Operator
from naive_query_engine_amd.expression import binop, col, lit_i64
from tests.agg_value_util import ALL_AGGS, assert_matches_model, model_aggregate
from tests.test_gpu_aggregate_value_domains import FILTERED_TIERS, FLD, TIERS, shape_of

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "aggregate_paths.json")
SWITCHES = ("NQE_NO_PLAN_HINTS", "NQE_NO_KEY_SAMPLE", "NQE_NO_RANGE_PARTITION", "NQE_NO_RANGE_TAIL", "NQE_NO_AGG_JIT", "NQE_NO_WIDE_DIRECT",
            "NQE_TEST_SLAB_OOM", "NQE_JIT_MIN_ROWS", "NQE_TINY_UNPACK_TILES", "NQE_DEBUG")
EXECUTIONS = 3
X, O, A = binop, Operator, AggregateFunc


@dataclasses.dataclass
class Case:
    table: list                         # [(values, validity mask or None)]: the whole table, as the model indexes it
    aggs: list
    key: object = None                  # the key expression (None: un-grouped) …
    key_np: np.ndarray = None           # … and the group key of every row
    pred: object = None                 # the predicate …
    keep: np.ndarray = None             # … and the rows it keeps
    env: dict = dataclasses.field(default_factory=dict)
    jit: bool = False                   # wait for the specialised kernel after the first execution
    device_cols: dict = dataclasses.field(default_factory=dict)  # column index -> the Column uploaded instead of table[index] (a Utf8 key)


def small_ints(rng, n):
    return rng.integers(-50, 50, n).astype(np.int64)


# --------------------------------------------------------------------------- every tier: plain, nullable value column, filtered
def tier_case(tier, variant):
    def make(rng):
        filtered = variant == "filtered"
        s = shape_of(tier, filtered)
        n = len(s.kcol)
        mask = (rng.random(n) >= 0.1) if variant == "nullable" else None
        pred, keep = s.filt if filtered else (None, None)
        return Case([(s.kcol, None), (small_ints(rng, n), mask)], ALL_AGGS(1), s.key_expr, s.key_np, pred, keep, dict(s.env), s.jit)
    return make


assert set(FILTERED_TIERS) <= set(TIERS)
CASES = {f"{tier}_{variant}": tier_case(tier, variant) for tier in TIERS for variant in ("plain", "nullable", "filtered")}
# The FIRST execution of these two is not reproducible on the recorded library itself: whether it already takes the run-time specialised kernel
# depends on what an earlier process left in the specialised kernels' disk cache (expr_jit.hpp).  It is run and checked against the model, but its
# launches are not pinned (null in the fixture); after jit_wait() the second and third executions take `agg_grouped_jit` and are.
FIRST_EXECUTION_NOT_PINNED = ("specialised_streaming_plain", "specialised_streaming_filtered")


# --------------------------------------------------------------------------- shapes with a path of their own
def c_three_value_columns(rng, plain_key=False, env=None):
    n = 300_011
    if plain_key:  # 3000 consecutive keys, more than the three-column instance's 2048-slot table holds: the key sample sees that and starts partitioned;
        # without the sample the instance overflows and the redo runs in passes of one and two, which overflow in turn
        k = rng.integers(-1000, 2000, n).astype(np.int64)
        key, key_np = col(0), k
    else:
        k = rng.integers(0, 1 << 40, n).astype(np.int64)
        key, key_np = X(col(0), O.Modulos, lit_i64(700)), k % 700
    aggs = [(A.Count, 1), (A.Sum, 1), (A.Sum, 2), (A.Avg, 2), (A.Sum, 3), (A.Avg, 3), (A.Count, 3)]
    return Case([(k, None)] + [(small_ints(rng, n), None) for _ in range(3)], aggs, key, key_np, env=env or {})


def c_two_value_columns(rng):
    n = 300_011
    k = rng.integers(-400, 600, n).astype(np.int64)
    return Case([(k, None), (small_ints(rng, n), None), (small_ints(rng, n), None)], ALL_AGGS(1) + ALL_AGGS(2), col(0), k)


def c_utf8_key(rng):
    n = 300_011
    ids = rng.integers(0, 500, n).astype(np.int64)
    names = [f"key-{i:04d}" + ("é" if i % 7 == 0 else "") for i in range(500)]
    strings = Column.from_list([names[i] for i in ids.tolist()], DType.UTF8)
    return Case([(ids, None), (small_ints(rng, n), None)], ALL_AGGS(1), col(0), ids, device_cols={0: strings})


def _keyed(rng, n=300_011, groups=1000):
    k = rng.integers(0, groups, n).astype(np.int64)
    return k, [(k, None), (small_ints(rng, n), None), (small_ints(rng, n), None)]


def c_pred_and_list_of_range_tests(rng):
    k, table = _keyed(rng)
    v = table[1][0]
    pred = X(X(col(0), O.GtEq, lit_i64(100)), O.And, X(col(1), O.Lt, lit_i64(20)))
    return Case(table, ALL_AGGS(1), col(0), k, pred, (k >= 100) & (v < 20))


def c_pred_tree(rng):
    k, table = _keyed(rng)
    v = table[1][0]
    pred = X(X(col(1), O.Lt, lit_i64(20)), O.Or, X(X(col(0), O.Modulos, lit_i64(3)), O.Eq, lit_i64(0)))
    return Case(table, ALL_AGGS(1), col(0), k, pred, (v < 20) | (k % 3 == 0))


def c_pred_column_with_column(rng):
    # column-with-column compares over FOUR columns, one more than the in-kernel stack machine reads: a materialised Boolean column
    k, table = _keyed(rng)
    table.append((small_ints(rng, len(k)), None))
    a, b, c = table[1][0], table[2][0], table[3][0]
    pred = X(X(col(1), O.Lt, col(2)), O.Or, X(col(3), O.Lt, col(0)))
    return Case(table, ALL_AGGS(1), col(0), k, pred, (a < b) | (c < k))


def c_general_key_under_a_filter(rng):
    n = 50_000   # (the selection's output is a new table every time: nothing is recalled)
    ids = rng.permutation(n).astype(np.int64) + 1
    key = X(X(lit_i64(1_000_000), O.Divide, col(0)), O.Modulos, lit_i64(7))
    return Case([(ids, None), (small_ints(rng, n), None)], ALL_AGGS(1), key, (1_000_000 // ids) % 7, X(col(0), O.Lt, lit_i64(n // 2)), ids < n // 2)


def c_partitioned_hashed_under(env):
    def make(rng):
        s = shape_of("partitioned_hashed")
        return Case([(s.kcol, None), (small_ints(rng, len(s.kcol)), None)], ALL_AGGS(1), s.key_expr, s.key_np, env=dict(s.env, **env))
    return make


def c_ungrouped(rng, pred=False, n=300_000):
    w = rng.integers(-50, 50, n).astype(np.int64)
    p, keep = (X(X(col(0), O.Modulos, lit_i64(7)), O.GtEq, lit_i64(2)), np.fmod(w, 7) >= 2) if pred else (None, None)
    return Case([(w, None), (small_ints(rng, n), None)], ALL_AGGS(1), pred=p, keep=keep)


def c_grouped_zero_rows(rng):
    k = np.zeros(0, dtype=np.int64)
    return Case([(k, None), (k.copy(), None)], ALL_AGGS(1), col(0), k)


CASES.update({
    "three_value_columns_one_pass": c_three_value_columns,
    "three_value_columns_overflow_sampled": lambda rng: c_three_value_columns(rng, plain_key=True),
    "three_value_columns_overflow_without_key_sample": lambda rng: c_three_value_columns(rng, plain_key=True, env={"NQE_NO_KEY_SAMPLE": "1"}),
    "two_value_columns": c_two_value_columns,
    "utf8_key": c_utf8_key,
    "pred_and_list_of_range_tests": c_pred_and_list_of_range_tests,
    "pred_tree": c_pred_tree,
    "pred_column_with_column": c_pred_column_with_column,
    "general_key_under_a_filter": c_general_key_under_a_filter,
    "partitioned_hashed_slab_oom": c_partitioned_hashed_under({"NQE_TEST_SLAB_OOM": "1"}),
    "partitioned_hashed_no_plan_hints": c_partitioned_hashed_under({"NQE_NO_PLAN_HINTS": "1"}),
    "partitioned_hashed_no_key_sample": c_partitioned_hashed_under({"NQE_NO_KEY_SAMPLE": "1"}),
    "ungrouped": c_ungrouped,
    "ungrouped_chain_predicate": lambda rng: c_ungrouped(rng, pred=True),
    "ungrouped_zero_rows": lambda rng: c_ungrouped(rng, n=0),
    "grouped_zero_rows": c_grouped_zero_rows,
})


@contextlib.contextmanager
def switches(env):
    """the aggregate's environment switches are read per context or per call: exactly `env` is set while a case runs"""
    saved = {k: os.environ.pop(k, None) for k in SWITCHES}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def launches(ctx):
    return {name: cnt for name, (_, cnt) in sorted(ctx.timing_report().items())}


def run_case(name):
    """runs one case in a fresh context; returns the launches of each execution, every result checked against the model"""
    from naive_query_engine_amd import capi

    c = CASES[name](np.random.default_rng(sum(map(ord, name))))
    model = model_aggregate(c.table, c.aggs, key=c.key_np, keep=c.keep)
    kn = c.key.flatten(FLD) if c.key is not None else None
    pn = c.pred.flatten(FLD) if c.pred is not None else None
    runs = []
    with switches(c.env):
        ctx = capi.Context(0)
        try:
            t = ctx.table_from_host([c.device_cols[i] if i in c.device_cols else Column.from_numpy(v, m) for i, (v, m) in enumerate(c.table)])
            for rep in range(EXECUTIONS):
                ctx.timing_enable(True)
                ctx.timing_reset()
                got = ctx.aggregate(t, c.aggs, group_nodes=kn, pred_nodes=pn).to_host()
                ctx.timing_enable(False)
                runs.append(launches(ctx))
                assert_matches_model(got, model, what=f"{name}: execution {rep}")
                if c.jit and rep == 0:
                    ctx.jit_wait()
            del t
        finally:
            ctx.close()
    return runs


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as f:
        return json.load(f)


def test_the_fixture_covers_exactly_these_cases(recorded):
    assert sorted(recorded) == sorted(CASES)


@pytest.mark.parametrize("name", list(CASES))
def test_aggregate_path(recorded, name):
    got, exp = run_case(name), recorded[name]
    assert len(got) == len(exp) == EXECUTIONS
    assert [i for i, e in enumerate(exp) if e is None] == ([0] if name in FIRST_EXECUTION_NOT_PINNED else [])
    for i, (g, e) in enumerate(zip(got, exp)):
        print(name, i, g)
        assert e is None or g == e, f"{name}: launches of execution {i}"


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: python -m tests.test_gpu_aggregate_paths --record")
    if os.path.exists(FIXTURE):
        sys.exit(f"{FIXTURE} exists: the recorded dispatch is the reference and is not rewritten")
    rec = {}
    for case_name in CASES:
        rec[case_name] = run_case(case_name)
        if case_name in FIRST_EXECUTION_NOT_PINNED:
            rec[case_name][0] = None
        print(case_name, json.dumps(rec[case_name]), flush=True)
    with open(FIXTURE, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
