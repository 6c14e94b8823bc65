"""Pins the hash join's dispatch: for every build form and probe form, the kernels launched (every label of the context's
timing report with its launch count), which output columns share a buffer with a probe-table column or with another output
column, and the rows themselves against the oracle.  The expected launches and aliasing are data: tests/golden/hash_join_paths.json,
recorded once (python -m tests.test_gpu_hash_join_paths --record, which refuses to overwrite an existing file) from the library
as it was before the join's host code was split into per-form functions; the test only ever reads it.

Every case runs in a context of its own: a context remembers failed all-match probes by buffer address (join hints) and its
block pool hands addresses out again, so cases sharing one context would see each other."""
import contextlib
import json
import os
import sys

import numpy as np
import pytest

from naive_query_engine_amd import Column, DType
from oracle import oracle as orc
from tests.helpers import assert_batches_equal, random_utf8

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hash_join_paths.json")
SWITCHES = ("NQE_JOIN_NO_ASCENDING", "NQE_JOIN_PART_BUILD_MIN", "NQE_JOIN_PART_ONE_LEVEL", "NQE_JOIN_NO_SHARED_PROBE_COLUMNS",
            "NQE_TEST_PART_BUILD_OOM", "NQE_TEST_SORTED_COLS_OOM", "NQE_DEBUG")


def I64(a):
    return Column.from_numpy(np.asarray(a).astype(np.int64))


def U64(a):
    return Column.from_numpy(np.asarray(a).astype(np.uint64))


def F64(rng, n):
    return Column.from_numpy(rng.random(n))


def case(left, rights, lk=0, rk=0, env=None, split=False):
    """rights: the probe tables, probed one after the other; split: hash_join_build + hash_join_probe instead of hash_join"""
    return {"left": left, "rights": rights, "lk": lk, "rk": rk, "env": env or {}, "split": split or len(rights) > 1}


# ---- unique dense keys, plain payload (the key-ordered payload table)
def dense_unique(rng, nb=3000, gaps=False, lo=50):
    space = 2 * nb if gaps else nb
    keys = rng.permutation(space)[:nb].astype(np.int64) + lo
    return keys, [I64(keys), I64(rng.integers(0, 1000, nb)), F64(rng, nb)]


def c_dense_full_all_match(rng):
    keys, left = dense_unique(rng)
    return case(left, [[I64(rng.choice(keys, 5000)), F64(rng, 5000)]])


def c_dense_full_one_miss_probed_twice(rng):
    keys, left = dense_unique(rng)
    rk = rng.choice(keys, 5000)
    rk[1234] = keys.max() + 1
    right = [I64(rk), F64(rng, 5000)]
    return case(left, [right, "again"])


def c_dense_gaps_presence_in_lds(rng):
    keys, left = dense_unique(rng, gaps=True)
    return case(left, [[I64(rng.integers(47, 50 + 6003, 5000)), F64(rng, 5000)]])


def c_dense_gaps_presence_bitmap_beyond_128k(rng):
    # a key range of more than 2^20 (the bitmap of the probe exceeds 128 KiB) that is still dense: range <= 4 x rows
    nb, span = 270_000, 1_060_000
    keys = rng.permutation(span)[:nb].astype(np.int64)
    keys[:2] = [0, span - 1]
    return case([I64(keys), I64(rng.integers(0, 1000, nb))], [[I64(rng.integers(-3, span + 3, 6000)), F64(rng, 6000)]])


def c_dense_gaps_every_probe_row_matches(rng):
    keys, left = dense_unique(rng, gaps=True)
    return case(left, [[I64(rng.choice(keys, 5000)), F64(rng, 5000)]])


def c_dense_payload_kinds_2_3_4(rng):
    nb = 3000
    keys = rng.permutation(2 * nb)[:nb].astype(np.int64)
    wide = rng.integers(0, 1 << 30, nb)
    wide[:2] = [0, (1 << 30) - 1]
    left = [I64(keys), F64(rng, nb), I64(wide - 5), U64(rng.integers(0, 500, nb)), U64(rng.integers(0, 1 << 60, nb))]
    return case(left, [[I64(rng.integers(-3, 2 * nb + 3, 5000)), F64(rng, 5000)]])


def c_dense_key_only_build_side(rng):
    keys = rng.permutation(6000)[:3000].astype(np.int64)
    return case([I64(keys)], [[I64(rng.integers(-3, 6003, 5000)), F64(rng, 5000)]])


# ---- build forms of the dense table
def sized_build(rng, nb, env=None, ascending=False):
    keys = rng.permutation(2 * nb)[:nb].astype(np.int64)
    if ascending:
        keys = np.sort(keys)
        keys[[100, 5000]] = keys[[5000, 100]]
    return case([I64(keys), I64(rng.integers(0, 1 << 20, nb))], [[I64(rng.integers(-3, 2 * nb + 3, 6000)), F64(rng, 6000)]], env=env)


PART = {"NQE_JOIN_PART_BUILD_MIN": "65536"}
BUILD_FORMS = {
    "build_scatter_finish_65536": lambda rng: sized_build(rng, 1 << 16),
    "build_one_kernel_65535": lambda rng: sized_build(rng, (1 << 16) - 1),
    "build_partitioned_two_level": lambda rng: sized_build(rng, 1 << 17, PART),
    "build_partitioned_one_level": lambda rng: sized_build(rng, 1 << 17, dict(PART, NQE_JOIN_PART_ONE_LEVEL="1")),
    "build_partitioned_oom_falls_back": lambda rng: sized_build(rng, 1 << 17, dict(PART, NQE_TEST_PART_BUILD_OOM="1")),
    "build_ascending_skips_partitioning": lambda rng: sized_build(rng, 1 << 17, PART, ascending=True),
}


# ---- unique sparse keys (hashed tables)
def sparse_keys(rng, nb, hi):
    keys = np.unique(rng.integers(1 << 20, hi, nb + 64).astype(np.uint64))[:nb]
    assert keys.size == nb
    return rng.permutation(keys)


def sparse_probe(rng, keys, n, hi):
    return U64(rng.permutation(np.concatenate([rng.choice(keys, n - n // 4), rng.integers(0, hi, n // 4).astype(np.uint64)])))


def c_sparse_packed_pairs(rng):
    keys = sparse_keys(rng, 3000, 1 << 40)
    return case([U64(keys), I64(rng.integers(-500, 500, 3000))], [[sparse_probe(rng, keys, 6000, 1 << 40), F64(rng, 6000)]])


def c_sparse_pairs_of_16_bytes(rng):
    keys = sparse_keys(rng, 3000, 1 << 62)
    return case([U64(keys), I64(rng.integers(0, 1 << 50, 3000))], [[sparse_probe(rng, keys, 6000, 1 << 62), F64(rng, 6000)]])


def c_sparse_keys_0_to_max_check_form(rng):
    keys = sparse_keys(rng, 3000, 1 << 62)
    keys[:2] = [0, (1 << 64) - 1]
    return case([U64(keys), I64(rng.integers(0, 1 << 50, 3000))], [[sparse_probe(rng, keys, 6000, 1 << 62), F64(rng, 6000)]])


def c_sparse_pairs_every_probe_row_matches(rng):
    keys = sparse_keys(rng, 3000, 1 << 62)
    return case([U64(keys), I64(rng.integers(0, 1 << 50, 3000))], [[U64(rng.choice(keys, 6000)), F64(rng, 6000)]])


def c_sparse_two_payloads_coop_probe(rng):
    keys = sparse_keys(rng, 3000, 1 << 40)
    return case([U64(keys), I64(rng.integers(0, 99, 3000)), F64(rng, 3000)], [[sparse_probe(rng, keys, 6000, 1 << 40), F64(rng, 6000)]])


def c_sparse_nullable_and_utf8_payload(rng):
    keys = sparse_keys(rng, 3000, 1 << 40)
    left = [U64(keys), Column.from_numpy(rng.integers(0, 99, 3000).astype(np.int64), rng.random(3000) > 0.2), random_utf8(rng, 3000, 0.1)]
    return case(left, [[sparse_probe(rng, keys, 6000, 1 << 40), F64(rng, 6000)]])


def c_dense_unique_nullable_payload_lookup_probe(rng):
    keys = rng.permutation(6000)[:3000].astype(np.int64)
    left = [I64(keys), Column.from_numpy(rng.random(3000), rng.random(3000) > 0.2)]
    return case(left, [[I64(rng.integers(-3, 6003, 5000)), F64(rng, 5000)]])


# ---- duplicate keys (the sort-based build)
def dup_case(rng, key_space=400, env=None, left_extra=None, right_extra=None, key=I64, lo=0):
    nb, n = 3000, 4000
    left = [key(rng.integers(lo, lo + key_space, nb)), I64(rng.integers(0, 1000, nb)), F64(rng, nb)] + (left_extra(nb) if left_extra else [])
    right = [key(rng.integers(lo, lo + key_space + 5, n)), F64(rng, n)] + (right_extra(n) if right_extra else [])
    return case(left, [right], env=env)


def nullable_key(rng, k):
    """a key column with NULL slots (their words are zero; key validity is ignored: a NULL key joins as the key 0)"""
    valid = rng.random(k.length) > 0.1
    return Column.from_numpy(np.where(valid, k.to_numpy(), 0), valid)


def c_dup_nullable_probe_key_not_shared(rng):
    c = dup_case(rng)
    rk = c["rights"][0][0]
    c["rights"][0][0] = nullable_key(rng, rk)
    return c


def c_dup_nullable_build_key_no_shortcut(rng):
    c = dup_case(rng)
    k = c["left"][0]
    c["left"][0] = nullable_key(rng, k)
    return c


def utf8_keys(rng, ids):
    return Column.from_list([f"key-{i:05d}" + ("é" if i % 7 == 0 else "") for i in ids], DType.UTF8)


def c_utf8_key_unique(rng):
    return case([utf8_keys(rng, rng.permutation(2000)), I64(rng.integers(0, 100, 2000))], [[F64(rng, 4000), utf8_keys(rng, rng.integers(-5, 2005, 4000))]], rk=1)


def c_utf8_key_duplicates(rng):
    return case([utf8_keys(rng, rng.integers(0, 300, 2000)), I64(rng.integers(0, 100, 2000))], [[F64(rng, 4000), utf8_keys(rng, rng.integers(-5, 305, 4000))]], rk=1)


# ---- degenerate shapes, and one table probed by two batches
def c_empty_build_side(rng):
    return case([I64([]), F64(rng, 0)], [[I64(rng.integers(0, 9, 100)), F64(rng, 100)]])


def c_empty_probe_side(rng):
    keys, left = dense_unique(rng)
    return case(left, [[I64([]), F64(rng, 0)]])


def c_build_once_probe_twice(rng):
    keys, left = dense_unique(rng, gaps=True)
    return case(left, [[I64(rng.integers(47, 6053, 5000)), F64(rng, 5000)], [I64(rng.choice(keys, 3000)), F64(rng, 3000)]])


CASES = {
    "dense_full_all_match": c_dense_full_all_match,
    "dense_full_one_miss_probed_twice": c_dense_full_one_miss_probed_twice,
    "dense_gaps_presence_in_lds": c_dense_gaps_presence_in_lds,
    "dense_gaps_presence_bitmap_beyond_128k": c_dense_gaps_presence_bitmap_beyond_128k,
    "dense_gaps_every_probe_row_matches": c_dense_gaps_every_probe_row_matches,
    "dense_payload_kinds_2_3_4": c_dense_payload_kinds_2_3_4,
    "dense_key_only_build_side": c_dense_key_only_build_side,
    **BUILD_FORMS,
    "sparse_packed_pairs": c_sparse_packed_pairs,
    "sparse_pairs_of_16_bytes": c_sparse_pairs_of_16_bytes,
    "sparse_keys_0_to_max_check_form": c_sparse_keys_0_to_max_check_form,
    "sparse_pairs_every_probe_row_matches": c_sparse_pairs_every_probe_row_matches,
    "sparse_two_payloads_coop_probe": c_sparse_two_payloads_coop_probe,
    "sparse_nullable_and_utf8_payload": c_sparse_nullable_and_utf8_payload,
    "dense_unique_nullable_payload_lookup_probe": c_dense_unique_nullable_payload_lookup_probe,
    "dup_plain_sorted_copies": lambda rng: dup_case(rng),
    "dup_plain_sorted_copies_oom": lambda rng: dup_case(rng, env={"NQE_TEST_SORTED_COLS_OOM": "1"}),
    "dup_sparse_key_range": lambda rng: dup_case(rng, key_space=700, lo=1 << 40, key=lambda a: I64(np.asarray(a) * 1_000_003)),
    "dup_utf8_payload_both_sides": lambda rng: dup_case(rng, left_extra=lambda n: [random_utf8(rng, n, 0.1)], right_extra=lambda n: [random_utf8(rng, n, 0.1)]),
    "dup_boolean_and_nullable_payload": lambda rng: dup_case(rng, left_extra=lambda n: [Column.from_numpy(rng.random(n) < 0.5), Column.from_numpy(rng.random(n), rng.random(n) > 0.2)]),
    "dup_uint64_keys": lambda rng: dup_case(rng, key=U64),
    "dup_nullable_probe_key_not_shared": c_dup_nullable_probe_key_not_shared,
    "dup_nullable_build_key_no_shortcut": c_dup_nullable_build_key_no_shortcut,
    "utf8_key_unique": c_utf8_key_unique,
    "utf8_key_duplicates": c_utf8_key_duplicates,
    "empty_build_side": c_empty_build_side,
    "empty_probe_side": c_empty_probe_side,
    "build_once_probe_twice": c_build_once_probe_twice,
}


@contextlib.contextmanager
def switches(env):
    """the join's environment switches are read per call: exactly `env` is set while a case runs"""
    saved = {k: os.environ.pop(k, None) for k in SWITCHES}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def aliasing(out, probe):
    """[[output column, probe-table column]] and [[output column, earlier output column]] holding the same values buffer"""
    optr = [out.column_info(i).values for i in range(out.num_columns)]
    pptr = [probe.column_info(j).values for j in range(probe.num_columns)]
    with_probe = [[i, j] for i, p in enumerate(optr) for j, q in enumerate(pptr) if p and p == q]
    with_out = [[i, k] for i, p in enumerate(optr) for k in range(i) if p and p == optr[k]]
    return {"probe": with_probe, "out": with_out}


def launches(ctx):
    return {name: cnt for name, (_, cnt) in sorted(ctx.timing_report().items())}


def run_case(name):
    """runs one case in a fresh context; returns its record: one entry per call (build / probe / join), oracle-checked"""
    from naive_query_engine_amd import capi

    c = CASES[name](np.random.default_rng(sum(map(ord, name))))
    left, lk, rk = c["left"], c["lk"], c["rk"]
    ctx = capi.Context(0)
    calls = []
    try:
        with switches(c["env"]):
            lt = ctx.table_from_host(left)
            ctx.timing_enable()
            jt = None
            if c["split"]:
                ctx.timing_reset()
                jt = ctx.hash_join_build(lt, lk)
                calls.append({"call": "build", "launches": launches(ctx)})
            right = rt = None
            for r in c["rights"]:
                if r != "again":  # "again": the same probe table object once more
                    right, rt = r, ctx.table_from_host(r)
                ctx.timing_reset()
                out = ctx.hash_join_probe(jt, rt, rk) if c["split"] else ctx.hash_join(lt, rt, lk, rk)
                calls.append({"call": "probe" if c["split"] else "join", "launches": launches(ctx), "aliases": aliasing(out, rt), "rows": out.num_rows})
                assert_batches_equal(out.to_host(), orc.hash_join([left], [right], lk, rk)[0], what=f"{name}: call {len(calls) - 1}")
                del out
            del jt, rt, lt
    finally:
        ctx.close()
    return calls


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as f:
        return json.load(f)


def test_the_fixture_covers_exactly_these_cases(recorded):
    assert sorted(recorded) == sorted(CASES)


@pytest.mark.parametrize("name", list(CASES))
def test_hash_join_path(recorded, name):
    got, exp = run_case(name), recorded[name]
    for i, (g, e) in enumerate(zip(got, exp)):
        print(name, i, g)
        assert g["call"] == e["call"]
        assert g["launches"] == e["launches"], f"{name}: launches of call {i} ({g['call']})"
        assert g.get("aliases") == e.get("aliases"), f"{name}: output aliasing of call {i}"
        assert g.get("rows") == e.get("rows")
    assert len(got) == len(exp)
    if name == "dense_full_one_miss_probed_twice":
        # the first probe tries the one-pass form and repeats the write; the second probe of the table goes to two passes at once
        assert got[1]["launches"]["join_fused_write"] == 2 and "join_probe_presence" in got[1]["launches"]
        assert got[2]["launches"]["join_fused_write"] == 1 and "join_probe_presence" in got[2]["launches"]


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: python -m tests.test_gpu_hash_join_paths --record")
    if os.path.exists(FIXTURE):
        sys.exit(f"{FIXTURE} exists: the recorded dispatch is the reference and is not rewritten")
    rec = {}
    for case_name in CASES:
        rec[case_name] = run_case(case_name)
        print(case_name, json.dumps(rec[case_name]))
    with open(FIXTURE, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
