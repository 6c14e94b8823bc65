"""The hash join on several keys on the device (nqe_hash_join_build_keys / _probe_keys / _execute_keys, csrc/join_keys.hip; quirk Q21:
HashJoin honouring every `on` pair, with the hash join's own match relation).

The yardstick is the tuple model of tests/join_keys_util.py (checked against pyarrow in tests/test_join_keys_host.py).  As a second,
independent check the model's dense tuple ids are handed to the unmodified oracle's single-key join: its rows are the inner join's, in
its order.  Every comparison is bit for bit: the operator only compares and copies.  Which path ran — packed or dictionary — is asserted
through nqe_ctx_timing_query on the kernels' names; integer cases run both plain and with NQE_JOIN_KEYS_FORCE_DICT=1."""
import contextlib
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import join_keys_util as jku  # noqa: E402
import outer_join_util as oju  # noqa: E402
from naive_query_engine_amd import Column, DType, ErrorCode, Field, RecordBatch, Status  # noqa: E402

pytestmark = pytest.mark.gpu
I64 = np.iinfo(np.int64)
U64_MAX = 2**64 - 1
LABELS = ("join_keys_pack_probe", "join_keys_lookup", "group_keys_ranges", "group_keys_pack", "group_keys_dict")


@pytest.fixture(scope="module")
def pp():
    from naive_query_engine_amd import physical_plan

    return physical_plan


@pytest.fixture(scope="module")
def ctx():
    from naive_query_engine_amd import capi

    c = capi.default_context()
    c.timing_enable(True)
    yield c
    c.timing_enable(False)


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle

    return oracle


@contextlib.contextmanager
def force_dict(on):
    old = os.environ.pop("NQE_JOIN_KEYS_FORCE_DICT", None)
    if on:
        os.environ["NQE_JOIN_KEYS_FORCE_DICT"] = "1"
    try:
        yield
    finally:
        os.environ.pop("NQE_JOIN_KEYS_FORCE_DICT", None)
        if old is not None:
            os.environ["NQE_JOIN_KEYS_FORCE_DICT"] = old


def i64(a):
    return Column.from_numpy(np.asarray(a, dtype=np.int64))


def u64(a):
    return Column.from_numpy(np.asarray(a, dtype=np.uint64))


def f64(a, mask=None):
    return Column.from_numpy(np.asarray(a, dtype=np.float64), mask)


def launches(ctx):
    return {name: ctx.timing_query(name)[1] for name in LABELS}


def build_path(ctx):
    """which path the build that just ran took: 'pack', 'dict' or 'none' (one pair, or an empty build side)"""
    n = launches(ctx)
    if n["group_keys_pack"]:
        assert n["group_keys_ranges"] == 1 and n["group_keys_pack"] == 1 and n["group_keys_dict"] == 0
        return "pack"
    if n["group_keys_dict"]:
        return "dict"
    return "none"


def check_table(t, exp, null_left, null_right, nleft, what, inner=False):
    got = t.to_host()
    ncols = len(exp)
    zero_rows = [null_left] * nleft + [null_right] * (ncols - nleft)
    oju.assert_same_columns(got, exp, what, zero_rows=zero_rows)  # (the column count: no code column in any output)
    assert t.num_columns == ncols
    for i, e in enumerate(jku.null_counts(exp)):
        nc = int(t.column_info(i).null_count)  # exact on the outer path (Q19); the inner probe's tiers may leave a gathered column's count unknown (-1)
        assert nc == e or (inner and nc == -1), f"{what} column {i}: null_count {nc}, expected {e}"
    return got


def run_join(ctx, left, lkeys, batches, rkeys, how, dict_forced=False, path=None, orc=None, what=""):
    """builds, probes every batch (marks for left / full, keep_probe for right / full), takes the final batch, and compares each output
    with the model; `path`: the expected build path; `orc`: also compare an inner join with the oracle through dense ids"""
    exp = jku.expected_batches(left, lkeys, batches, rkeys, how)
    nleft = len(left)
    with force_dict(dict_forced):
        lt = ctx.table_from_host(left)
        ctx.timing_reset()
        jt = ctx.hash_join_build_keys(lt, lkeys)
        taken = build_path(ctx)
        if path is not None and left[0].length > 0:
            assert taken == path, f"{what}: build path {taken}, expected {path}"
        marks = ctx.join_marks(jt) if how in ("left", "full") else None
        outs = []
        for bi, right in enumerate(batches):
            rt = ctx.table_from_host(right)
            ctx.timing_reset()
            t = ctx.hash_join_probe_keys(jt, rt, rkeys, keep_probe=how in ("right", "full"), marks=marks)
            n = launches(ctx)
            if len(lkeys) > 1 and right[0].length > 0:
                want = "join_keys_pack_probe" if taken == "pack" or (taken == "none" and not dict_forced and all(left[k].dtype != DType.UTF8 for k in lkeys)) else "join_keys_lookup"
                other = "join_keys_lookup" if want == "join_keys_pack_probe" else "join_keys_pack_probe"
                assert n[want] == 1 and n[other] == 0, f"{what} batch {bi}: launches {n}"
            cols, nl, nr = exp[bi]
            outs.append(check_table(t, cols, nl, nr, nleft, f"{what} [{how}{' dict' if dict_forced else ''}] batch {bi}", inner=how == "inner"))
        if marks is not None:
            cols, nl, nr = exp[-1]
            t = ctx.hash_join_unmatched_build(jt, marks, [c.dtype for c in batches[0]])
            check_table(t, cols, nl, nr, nleft, f"{what} [{how}{' dict' if dict_forced else ''}] final batch")
            assert t.num_columns == nleft + len(batches[0])
    if orc is not None and how == "inner":
        lid, rids = jku.dense_tuple_ids(left, lkeys, batches, rkeys)
        for bi, right in enumerate(batches):
            ref = orc.hash_join([list(left) + [i64(lid)]], [list(right) + [i64(rids[bi])]], nleft, len(right))
            if not ref:
                assert outs[bi][0].length == 0
                continue
            assert len(ref) == 1
            ref = ref[0][:nleft] + ref[0][nleft + 1:-1]
            oju.assert_same_columns(outs[bi], ref, f"{what} batch {bi} vs the oracle over dense ids", presence=False)
    return outs


def both_paths(ctx, left, lkeys, batches, rkeys, hows=("inner", "full"), path="pack", orc=None, what=""):
    for how in hows:
        run_join(ctx, left, lkeys, batches, rkeys, how, False, path, orc, what)
        run_join(ctx, left, lkeys, batches, rkeys, how, True, "dict", None, what)


def int_tables(rng, nb, npr, k, card=6, dup=True):
    """build: k key columns + a row id + a nullable Float64; probe: a row id, then k key columns, then a nullable Boolean.  Keys of
    `card` values each, so that one key alone matches many rows and the tuple few; about a fifth of the probe tuples lie outside."""
    lk = [rng.integers(-2, card - 2, nb).astype(np.int64) for _ in range(k)]
    if not dup and nb:
        flat = rng.permutation(card**k)[:nb] if card**k >= nb else None
        assert flat is not None
        lk = [((flat // card**i) % card - 2).astype(np.int64) for i in range(k)]
    rk = [rng.integers(-3, card - 1, npr).astype(np.int64) for _ in range(k)]
    left = [i64(a) for a in lk] + [i64(np.arange(nb)), f64(rng.integers(-9, 9, nb), rng.random(nb) > 0.3 if nb else None)]
    right = [i64(np.arange(npr) * 3)] + [i64(a) for a in rk] + [Column.from_numpy(rng.random(npr) < 0.5, rng.random(npr) > 0.2 if npr else None)]
    return left, list(range(k)), right, list(range(1, k + 1))


# ----------------------------------------------------------------------------- sizes
SIZES = [0, 1, 2, 3, 63, 64, 65, 4097]  # pairs and the odd tail of the pack kernels, wave edges, one past a probe tile


@pytest.mark.parametrize("nb", SIZES)
def test_build_and_probe_row_counts(ctx, orc, nb):
    rng = np.random.default_rng(300 + nb)
    for npr in SIZES:
        left, lkeys, right, rkeys = int_tables(rng, nb, npr, 2)
        hows = ("inner", "full") if npr in (0, 3, 65, 4097) else ("full",)
        both_paths(ctx, left, lkeys, [right], rkeys, hows=hows, orc=orc if nb <= 65 else None, what=f"build {nb} probe {npr}")


def test_second_pair_in_flight_and_the_scalar_tail(ctx):
    """join_keys_pack_probe with 16-byte loads: a lane takes pair p and pair p + stride per trip, stride = grid x 256 lanes, and
    grid = stream_grid(n / 2 pairs, 512 per block) = ceil(20000 / 512) = 40 blocks for n = 40001 (far below the cap of 8 blocks per
    CU).  stride = 10240: lanes 0 .. 9759 have their second pair inside the 20000 pairs, lanes 9760 .. 10239 do not, and row 40000 — the
    odd one — goes through the scalar tail.  The build side has the same size, so group_keys_pack runs the same shape."""
    n = 40001
    rng = np.random.default_rng(40001)
    left = [i64(rng.integers(0, 300, n)), i64(rng.integers(-100, 100, n)), i64(np.arange(n))]
    right = [i64(rng.integers(-1, 301, n)), i64(rng.integers(-101, 101, n)), f64(np.arange(n))]
    right[0].values[n - 1], right[1].values[n - 1] = left[0].values[5], left[1].values[5]  # the tail row matches
    out = run_join(ctx, left, [0, 1], [right], [0, 1], "inner", path="pack", what="40001 rows")
    assert out[0][0].length > 1000 and (out[0][5].to_numpy()[-1] == n - 1)
    run_join(ctx, left, [0, 1], [right], [0, 1], "right", dict_forced=True, path="dict", what="40001 rows")


def test_probe_columns_that_start_at_an_odd_word(ctx):
    """key columns 8-byte but not 16-byte aligned: the 8-byte form of the pack-probe kernel (the lookup kernel has one form)"""
    rng = np.random.default_rng(9)
    n = 1001
    left, lkeys, right, rkeys = int_tables(rng, 500, n + 1, 3)
    owner = ctx.table_from_host(right)
    word = [c for c in range(len(right)) if right[c].dtype != DType.BOOLEAN]
    tail = [Column.from_numpy(right[c].to_numpy()[1:].copy()) for c in word]  # rows 1 .. n of the word columns (no validity among them)
    exp = jku.expected_batches(left, lkeys, [tail], rkeys, "right")
    lt = ctx.table_from_host(left)
    for forced in (False, True):
        with force_dict(forced):
            jt = ctx.hash_join_build_keys(lt, lkeys)
            rt = ctx.table_from_device([(right[c].dtype, n, owner.column_info(c).values + 8, None) for c in word])
            assert all((owner.column_info(c).values + 8) % 16 == 8 for c in word)
            ctx.timing_reset()
            t = ctx.hash_join_probe_keys(jt, rt, rkeys, keep_probe=True)
            assert launches(ctx)["join_keys_lookup" if forced else "join_keys_pack_probe"] == 1
            check_table(t, exp[0][0], exp[0][1], exp[0][2], len(left), f"odd-word probe columns forced={forced}")
            del t, rt


@pytest.mark.parametrize("k", [2, 3, 8])
def test_key_counts(ctx, orc, k):
    rng = np.random.default_rng(400 + k)
    left, lkeys, right, rkeys = int_tables(rng, 700, 1500, k, card=3 if k == 8 else 5)
    both_paths(ctx, left, lkeys, [right], rkeys, orc=orc, what=f"{k} keys")


# ----------------------------------------------------------------------------- discrimination
def test_single_keys_match_many_rows_the_tuple_few(ctx, orc):
    n = 400
    x, y = np.arange(n) % 20, np.arange(n) // 20  # every (x, y) once
    left = [i64(x), i64(y), i64(np.arange(n))]
    right = [i64(np.arange(60)), i64(np.arange(60) % 20), i64((np.arange(60) * 7) % 25)]  # y up to 24: some tuples are absent
    out = run_join(ctx, left, [0, 1], [right], [1, 2], "inner", path="pack", orc=orc, what="x and y")
    on_x_only = ctx.hash_join(ctx.table_from_host(left), ctx.table_from_host(right), 0, 1).num_rows
    assert on_x_only == 60 * 20 and out[0][0].length == int(((np.arange(60) * 7) % 25 < 20).sum()) < 60  # a join on on[0] alone fails this
    both_paths(ctx, left, [0, 1], [right], [1, 2], hows=("left",), what="x and y")


def test_1_2_against_2_1(ctx, orc):
    left = [i64([1, 2, 1, 2]), i64([2, 1, 1, 2]), i64([10, 20, 30, 40])]
    right = [i64([2, 1, 3]), i64([1, 2, 3])]
    for forced in (False, True):
        out = run_join(ctx, left, [0, 1], [right], [0, 1], "inner", forced, orc=orc, what="(1,2) vs (2,1)")
        assert out[0][2].to_list() == [20, 10]
        out = run_join(ctx, left, [1, 0], [right], [0, 1], "inner", forced, what="swapped pairs")
        assert out[0][2].to_list() == [10, 20]


@pytest.mark.parametrize("dtype", ["int64", "uint64"])
def test_probe_keys_one_outside_the_build_range_in_each_position(ctx, dtype):
    mk = i64 if dtype == "int64" else u64
    lo, hi = (-5, 5) if dtype == "int64" else (2**63 - 3, 2**63 + 3)  # (the unsigned range straddles the sign bit)
    vals = list(range(lo, hi + 1))
    left = [mk(vals), mk(vals[::-1]), mk([hi] * len(vals)), i64(np.arange(len(vals)))]
    rows = []
    for pos in range(3):
        for v in (lo - 1, hi + 1, lo, hi):
            t = [vals[3], vals[-4], hi]
            t[pos] = v
            rows.append(t)
    rows.append([vals[3], vals[-4], hi])  # the one real match
    right = [mk([r[i] for r in rows]) for i in range(3)]
    for forced in (False, True):
        out = run_join(ctx, left, [0, 1, 2], [right], [0, 1, 2], "full", forced, "dict" if forced else "pack", what=f"{dtype} range edges")
        assert out[0][3].to_list().count(3) == 2  # the real match, and the row whose third key was "replaced" by the value it had


def test_extreme_values_and_the_dictionary_without_the_switch(ctx, orc):
    # one full-range key beside a small one: the spans' product overflows 2^62
    left = [i64([I64.min, I64.max, 0, I64.min]), i64([1, 2, 1, 2]), i64([0, 1, 2, 3])]
    right = [i64([I64.min, I64.max, I64.min, -1, 0]), i64([2, 2, 1, 1, 1])]
    run_join(ctx, left, [0, 1], [right], [0, 1], "full", path="dict", what="int64 extremes")
    run_join(ctx, left, [0, 1], [right], [0, 1], "inner", path="dict", orc=orc, what="int64 extremes")
    # two full-range keys
    left = [i64([I64.min, I64.max, I64.max]), u64([0, U64_MAX, 0]), i64([7, 8, 9])]
    right = [u64([U64_MAX, 0, U64_MAX, 0]), i64([I64.max, I64.max, I64.min, I64.min])]
    out = run_join(ctx, left, [0, 1], [right], [1, 0], "full", path="dict", what="two full-range keys")
    assert out[0][2].to_list() == [8, 9, None, 7]
    # the extremes inside ranges that still pack
    left = [i64([I64.max - 2, I64.max, I64.max - 1]), i64([I64.min, I64.min + 2, I64.min + 1]), u64([U64_MAX, U64_MAX - 1, U64_MAX])]
    right = [i64([I64.max, I64.max - 3, I64.max - 1, I64.min]), i64([I64.min + 2, I64.min, I64.min + 1, I64.min]), u64([U64_MAX - 1, U64_MAX, U64_MAX, 0])]
    both_paths(ctx, left, [0, 1, 2], [right], [0, 1, 2], orc=orc, what="extremes, packed")


def test_int64_and_uint64_pairs_in_one_join(ctx, orc):
    rng = np.random.default_rng(5)
    n, m = 300, 800
    left = [i64(rng.integers(-4, 4, n)), u64(rng.integers(2**63 - 2, 2**63 + 2, n, dtype=np.uint64)), i64(np.arange(n))]
    right = [u64(rng.integers(2**63 - 3, 2**63 + 3, m, dtype=np.uint64)), f64(np.arange(m)), i64(rng.integers(-5, 5, m))]
    both_paths(ctx, left, [0, 1], [right], [2, 0], orc=orc, what="Int64 + UInt64")


# ----------------------------------------------------------------------------- Utf8
def test_utf8_pairs(ctx, orc):
    names = ["", "a", "ab", "abc", "b", "a" * 40, "ab\x00"]  # the empty string; strings equal up to length
    rng = np.random.default_rng(6)
    n, m = 200, 500
    ls = [names[i] for i in rng.integers(0, len(names), n)]
    rs = [(names + ["absent", "abcd"])[i] for i in rng.integers(0, len(names) + 2, m)]  # strings the build side does not have
    left = [oju.utf8_column(ls), i64(rng.integers(0, 4, n)), i64(np.arange(n))]
    right = [i64(rng.integers(0, 5, m)), oju.utf8_column(rs), f64(np.arange(m), rng.random(m) > 0.5)]
    for how in ("inner", "full"):
        run_join(ctx, left, [0, 1], [right], [1, 0], how, path="dict", orc=orc, what="(Utf8, Int64)")
        run_join(ctx, left, [1, 0], [right], [0, 1], how, path="dict", what="(Int64, Utf8)")
    left2 = [oju.utf8_column(ls), oju.utf8_column(ls[::-1]), i64(np.arange(n))]
    right2 = [oju.utf8_column(rs), oju.utf8_column(rs[::-1])]
    for how in ("inner", "full"):
        run_join(ctx, left2, [0, 1], [right2], [0, 1], how, path="dict", orc=orc, what="(Utf8, Utf8)")
    # ("a", "bc") against ("ab", "c"): the tuple is not the concatenation
    out = run_join(ctx, [oju.utf8_column(["a", "ab"]), oju.utf8_column(["bc", "c"]), i64([1, 2])], [0, 1], [[oju.utf8_column(["ab", "a", "a"]), oju.utf8_column(["c", "bc", "b"])]],
                   [0, 1], "right", path="dict", what="tuple boundaries")
    assert out[0][2].to_list() == [2, 1, None]
    # an empty build side with a Utf8 pair: the empty dictionary
    run_join(ctx, [oju.utf8_column([]), i64([]), i64([])], [0, 1], [[oju.utf8_column(["a", ""]), i64([1, 2])]], [0, 1], "full", what="empty Utf8 build")


# ----------------------------------------------------------------------------- Q11
def test_null_key_slots_match_by_their_raw_slot(ctx):
    bmask = np.array([True, False, True, False])
    left = [Column.from_numpy(np.array([5, 7, 9, 7], dtype=np.int64), bmask), Column.from_numpy(np.array([1, 2, 3, 4], dtype=np.int64), ~bmask),
            f64([0.5, 1.5, 2.5, 3.5], np.array([True, True, False, True]))]
    right = [Column.from_numpy(np.array([7, 9, 5, 7], dtype=np.int64), np.array([False, True, False, True])), Column.from_numpy(np.array([2, 3, 9, 4], dtype=np.int64)),
             Column.from_numpy(np.array([True, False, True, True]), np.array([True, False, True, True]))]
    for forced in (False, True):
        out = run_join(ctx, left, [0, 1], [right], [0, 1], "full", forced, what="NULL key slots")
        assert out[0][2].to_list() == [1.5, None, None, 3.5]  # the NULLs' slots matched; the payload's own NULL survives
        assert out[0][0].to_list() == [None, 9, None, None] and out[0][3].to_list() == [None, 9, None, 7]  # key validity is copied, not read
    # Utf8: the bytes under a NULL
    ls = oju.utf8_column(["x", "y", "z"])
    ls.validity = oju.pack_bits(np.array([True, False, True]))
    rs = oju.utf8_column(["y", "q"])
    rs.validity = oju.pack_bits(np.array([False, True]))
    out = run_join(ctx, [ls, i64([1, 1, 1]), i64([10, 20, 30])], [0, 1], [[rs, i64([1, 1])]], [0, 1], "right", path="dict", what="NULL Utf8 slots")
    assert out[0][2].to_list() == [20, None]


# ----------------------------------------------------------------------------- build forms
def test_build_forms(ctx, orc):
    rng = np.random.default_rng(8)
    # unique tuples; every tuple four times (ascending build row within a probe row's matches)
    left, lkeys, right, rkeys = int_tables(rng, 600, 1300, 2, card=30, dup=False)
    both_paths(ctx, left, lkeys, [right], rkeys, orc=orc, what="unique tuples")
    four = [oju.take_null([c], np.tile(np.arange(150), 4))[0] for c in left[:2]] + [i64(np.arange(600)), left[3]]
    both_paths(ctx, four, lkeys, [right], rkeys, orc=orc, what="every tuple four times")
    # packed codes dense and gap-free (a 16 x 16 box, every tuple once, plain payload), probed with tuples outside the box: the all-match
    # probe of the dense build fails on the -1 code and the two-pass form takes over
    n = 256
    left = [i64(np.arange(n) // 16), i64(np.arange(n) % 16), i64(np.arange(n) * 10)]
    inside = [i64(rng.integers(0, 16, 500)), i64(rng.integers(0, 16, 500)), i64(np.arange(500))]
    outside = [i64(np.r_[rng.integers(0, 16, 499), 16]), i64(np.r_[rng.integers(0, 16, 499), 3]), i64(np.arange(500))]
    for batch in ([inside], [outside], [inside, outside, inside]):
        run_join(ctx, left, [0, 1], batch, [0, 1], "inner", path="pack", orc=orc, what="gap-free codes")
    # the route itself, by launch label: the all-match form is ONE join_fused_write and no presence pass; the batch that fails it runs
    # join_fused_write twice (the abandoned attempt, then the two-pass form's write) after one presence pass; from then on the table
    # goes to the two-pass form at once.  (A tuple table neither reads nor leaves a hint in the context, so a fresh table starts optimistic.)
    lt = ctx.table_from_host(left)
    jt = ctx.hash_join_build_keys(lt, [0, 1])
    for bi, (batch, fused, presence) in enumerate([(inside, 1, 0), (outside, 2, 1), (inside, 1, 1), (outside, 1, 1)]):
        ctx.timing_reset()
        t = ctx.hash_join_probe_keys(jt, ctx.table_from_host(batch), [0, 1])
        got = (ctx.timing_query("join_fused_write")[1], ctx.timing_query("join_probe_presence")[1])
        assert got == (fused, presence), f"gap-free codes, probe {bi}: (join_fused_write, join_probe_presence) launches {got}, expected {(fused, presence)}"
        assert t.num_rows == (500 if batch is inside else 499)
    jt_fresh = ctx.hash_join_build_keys(lt, [0, 1])  # the verdict stayed with the other table
    ctx.timing_reset()
    ctx.hash_join_probe_keys(jt_fresh, ctx.table_from_host(inside), [0, 1])
    assert (ctx.timing_query("join_fused_write")[1], ctx.timing_query("join_probe_presence")[1]) == (1, 0)
    run_join(ctx, left, [0, 1], [outside, inside], [0, 1], "full", path="pack", what="gap-free codes")
    run_join(ctx, left, [0, 1], [outside], [0, 1], "inner", dict_forced=True, path="dict", what="gap-free codes")


# ----------------------------------------------------------------------------- outer joins
@pytest.mark.parametrize("how", ["right", "left", "full"])
def test_outer_joins_over_two_probe_batches(ctx, how):
    rng = np.random.default_rng(11)
    left, lkeys, r1, rkeys = int_tables(rng, 301, 5000, 2, card=25)
    _, _, r2, _ = int_tables(rng, 1, 1025, 2, card=9)  # the second batch reaches fewer build rows: the marks of the two differ
    both_paths(ctx, left, lkeys, [r1, r2], rkeys, hows=(how,), what="two probe batches")
    sl, sk, s1, srk = [oju.utf8_column([f"s{v}" for v in left[0].to_numpy()])] + left[1:], lkeys, [r1[0], oju.utf8_column([f"s{v}" for v in r1[1].to_numpy()])] + r1[2:], rkeys
    run_join(ctx, sl, sk, [s1], srk, how, path="dict", what="two probe batches, Utf8")


def test_the_final_batch_has_no_code_column_and_all_null_right_columns(ctx):
    left = [i64([1, 1, 2]), i64([1, 2, 2]), oju.utf8_column(["a", None, "c"])]
    right = [i64([1, 5]), i64([2, 5]), Column.from_numpy(np.array([True, False])), oju.utf8_column(["p", "q"]), f64([1.0, 2.0])]
    for forced in (False, True):
        with force_dict(forced):
            jt = ctx.hash_join_build_keys(ctx.table_from_host(left), [0, 1])
            marks = ctx.join_marks(jt)
            ctx.hash_join_probe_keys(jt, ctx.table_from_host(right), [0, 1], marks=marks)
            t = ctx.hash_join_unmatched_build(jt, marks, [c.dtype for c in right])
            got = t.to_host()
            assert t.num_columns == 8 and t.num_rows == 2 and [c.dtype for c in got] == [c.dtype for c in left + right]
            assert got[0].to_list() == [1, 2] and got[1].to_list() == [1, 2] and got[2].to_list() == ["a", "c"]
            for i in range(3, 8):
                assert got[i].to_list() == [None, None] and int(t.column_info(i).null_count) == 2
            assert [int(t.column_info(i).null_count) for i in range(3)] == [0, 0, 0]


# ----------------------------------------------------------------------------- one pair
def test_one_pair_is_the_single_key_join(ctx):
    rng = np.random.default_rng(12)
    left, _, right, _ = int_tables(rng, 500, 3000, 2, card=40)
    lt, rt = ctx.table_from_host(left), ctx.table_from_host(right)
    ctx.timing_reset()
    jt, jt1 = ctx.hash_join_build_keys(lt, [1]), ctx.hash_join_build(lt, 1)
    oju.assert_same_columns(ctx.hash_join_probe_keys(jt, rt, [2]).to_host(), ctx.hash_join_probe(jt1, rt, 2).to_host(), "one pair, inner")
    oju.assert_same_columns(ctx.hash_join_keys(lt, rt, [1], [2]).to_host(), ctx.hash_join(lt, rt, 1, 2).to_host(), "one pair, execute")
    for keep in (False, True):
        m, m1 = ctx.join_marks(jt), ctx.join_marks(jt1)
        oju.assert_same_columns(ctx.hash_join_probe_keys(jt, rt, [2], keep_probe=keep, marks=m).to_host(),
                                ctx.hash_join_probe_outer(jt1, rt, 2, keep_probe=keep, marks=m1).to_host(), f"one pair, keep_probe={keep}")
        dts = [c.dtype for c in right]
        oju.assert_same_columns(ctx.hash_join_unmatched_build(jt, m, dts).to_host(), ctx.hash_join_unmatched_build(jt1, m1, dts).to_host(), "one pair, final batch")
    assert sum(launches(ctx).values()) == 0  # a single key keeps its own tiers: none of the tuple kernels ran
    # the tables are interchangeable: the single-key probe takes a one-pair table from build_keys
    oju.assert_same_columns(ctx.hash_join_probe(jt, rt, 2).to_host(), ctx.hash_join_probe(jt1, rt, 2).to_host(), "one pair, the other door")


# ----------------------------------------------------------------------------- errors
def _status(ctx, fn, *args):
    from naive_query_engine_amd import capi

    h = C.c_void_p()
    st = fn(ctx.handle, *args, C.byref(h))
    if st == 0 and h.value:
        capi.Table(ctx, h)  # released by its destructor
    return st


def _build_status(ctx, fn, *args):
    from naive_query_engine_amd import capi

    h = C.c_void_p()
    st = fn(ctx.handle, *args, C.byref(h))
    if st == 0 and h.value:
        capi.JoinTable(ctx, h)
    return st


def test_errors_are_decided_before_any_launch(ctx):
    from naive_query_engine_amd import capi

    L = capi.lib()
    ks = lambda *a: (C.c_int32 * max(1, len(a)))(*a)  # noqa: E731
    lt = ctx.table_from_host([i64([1, 2, 3]), i64([4, 5, 6]), f64([1, 2, 3]), u64([1, 2, 3]), oju.utf8_column(["a", "b", "c"])])
    rt = ctx.table_from_host([i64([1, 2]), i64([4, 5]), f64([1, 2]), u64([1, 2]), oju.utf8_column(["a", "b"])])
    jt2, jt1 = ctx.hash_join_build_keys(lt, [0, 1]), ctx.hash_join_build_keys(lt, [0])
    other = ctx.hash_join_build_keys(lt, [1, 0])
    marks_other = ctx.join_marks(other)
    ctx.synchronize()
    ctx.timing_reset()
    B, P, X = L.nqe_hash_join_build_keys, L.nqe_hash_join_probe_keys, L.nqe_hash_join_execute_keys
    # key counts
    assert _build_status(ctx, B, lt.handle, ks(0), 0) == Status.PlanError and _build_status(ctx, B, lt.handle, ks(0), -1) == Status.PlanError
    assert _build_status(ctx, B, lt.handle, ks(*[0] * 9), 9) == Status.NotSupported
    assert _status(ctx, P, jt2.handle, rt.handle, ks(0, 1), 0, 0, None) == Status.PlanError
    assert _status(ctx, P, jt2.handle, rt.handle, ks(*[0] * 9), 9, 0, None) == Status.NotSupported
    assert _status(ctx, X, lt.handle, rt.handle, ks(0), ks(0), 0) == Status.PlanError
    assert _status(ctx, X, lt.handle, rt.handle, ks(*[0] * 9), ks(*[0] * 9), 9) == Status.NotSupported
    # NULL index arrays and NULL out
    assert _build_status(ctx, B, lt.handle, None, 2) == Status.InvalidArgument
    assert _status(ctx, P, jt2.handle, rt.handle, None, 2, 0, None) == Status.InvalidArgument
    assert _status(ctx, X, lt.handle, rt.handle, None, ks(0, 1), 2) == Status.InvalidArgument and _status(ctx, X, lt.handle, rt.handle, ks(0, 1), None, 2) == Status.InvalidArgument
    assert B(ctx.handle, lt.handle, ks(0, 1), 2, None) == Status.InvalidArgument and P(ctx.handle, jt2.handle, rt.handle, ks(0, 1), 2, 0, None, None) == Status.InvalidArgument
    assert X(ctx.handle, lt.handle, rt.handle, ks(0, 1), ks(0, 1), 2, None) == Status.InvalidArgument
    # a key index out of range, in any position
    for bad in (ks(5, 0), ks(0, 5), ks(0, -1)):
        assert _build_status(ctx, B, lt.handle, bad, 2) == Status.LogicalError
        assert _status(ctx, P, jt2.handle, rt.handle, bad, 2, 0, None) == Status.LogicalError
        assert _status(ctx, X, lt.handle, rt.handle, bad, ks(0, 1), 2) == Status.LogicalError and _status(ctx, X, lt.handle, rt.handle, ks(0, 1), bad, 2) == Status.LogicalError
    # key types: check_key_types' errors for the first offending pair, in pair order
    assert _build_status(ctx, B, lt.handle, ks(0, 2), 2) == Status.NotImplemented  # a Float64 build key
    assert _status(ctx, P, jt2.handle, rt.handle, ks(0, 2), 2, 0, None) == Status.NotImplemented  # a Float64 probe key
    assert _status(ctx, P, jt2.handle, rt.handle, ks(0, 3), 2, 0, None) == Status.NotSupported  # Int64 against UInt64
    assert _status(ctx, P, jt2.handle, rt.handle, ks(4, 2), 2, 0, None) == Status.NotSupported  # the first pair decides (Int64 against Utf8)
    assert _status(ctx, P, jt2.handle, rt.handle, ks(2, 4), 2, 0, None) == Status.NotImplemented
    assert _status(ctx, X, lt.handle, rt.handle, ks(0, 1), ks(0, 3), 2) == Status.NotSupported and _status(ctx, X, lt.handle, rt.handle, ks(0, 2), ks(0, 1), 2) == Status.NotImplemented
    # num_keys against the build's; the single-key doors refuse a tuple table
    assert _status(ctx, P, jt2.handle, rt.handle, ks(0), 1, 0, None) == Status.InvalidArgument and _status(ctx, P, jt2.handle, rt.handle, ks(0, 1, 1), 3, 0, None) == Status.InvalidArgument
    assert _status(ctx, P, jt1.handle, rt.handle, ks(0, 1), 2, 0, None) == Status.InvalidArgument
    assert _status(ctx, L.nqe_hash_join_probe, jt2.handle, rt.handle, 0) == Status.InvalidArgument
    assert _status(ctx, L.nqe_hash_join_probe_outer, jt2.handle, rt.handle, 0, 1, None) == Status.InvalidArgument
    # flags and marks
    assert _status(ctx, P, jt2.handle, rt.handle, ks(0, 1), 2, 2, None) == Status.InvalidArgument
    assert _status(ctx, P, jt2.handle, rt.handle, ks(0, 1), 2, 1, marks_other.handle) == Status.InvalidArgument  # marks of another table
    assert _status(ctx, L.nqe_hash_join_unmatched_build, jt2.handle, marks_other.handle, ks(int(DType.INT64)), 1) == Status.InvalidArgument
    # the 32-column limit: the two hidden columns count — left + right = 31 is refused, 30 passes
    assert ctx.timing_query("")[1] == 0, "a refused call launched a kernel"
    w15, w16, w32 = (ctx.table_from_host([i64([1, 2])] * w) for w in (15, 16, 32))
    jw = ctx.hash_join_build_keys(w15, [0, 1])
    ctx.synchronize()
    ctx.timing_reset()
    assert _status(ctx, P, jw.handle, w16.handle, ks(0, 1), 2, 0, None) == Status.NotSupported
    assert _status(ctx, P, jw.handle, w16.handle, ks(0, 1), 2, 1, None) == Status.NotSupported
    assert _status(ctx, X, w15.handle, w16.handle, ks(0, 1), ks(0, 1), 2) == Status.NotSupported
    assert _build_status(ctx, B, w32.handle, ks(0, 1), 2) == Status.NotSupported
    assert ctx.timing_query("")[1] == 0, "a refused call launched a kernel"
    assert ctx.hash_join_probe_keys(jw, w15, [0, 1]).num_columns == 30 and ctx.hash_join_keys(w15, w15, [0, 1], [0, 1]).num_columns == 30
    # the sharded probe refuses a tuple table as the single-key probe does (one rank, a transport that must never be called: the
    # refusal comes before any exchange)
    class _NoTransport:
        def all_gather(self, *a):
            raise AssertionError("the refused probe reached the exchange")

        all_gather_v = all_gather

    comm = capi.Comm.custom(ctx, _NoTransport(), 0, 1)
    try:
        with pytest.raises(ErrorCode) as e:
            comm.sharded_hash_join_probe(jt2, rt, 0)
        assert e.value.status == Status.InvalidArgument
        assert comm.sharded_hash_join_probe(jt1, rt, 0).num_rows == 2  # (a one-pair table passes)
    finally:
        comm.close()
    # nothing above marked anything
    assert ctx.hash_join_unmatched_build(other, marks_other, []).num_rows == 3


# ----------------------------------------------------------------------------- mirrors
def _batches(cols, names, cuts):
    out, lo = [], 0
    for hi in cuts:
        out.append(RecordBatch([Field(nm, c.dtype, True) for nm, c in zip(names, cols)], oju.take_null(cols, np.arange(lo, hi))))
        lo = hi
    return out


@pytest.mark.parametrize("use_rewrite", [False, True])
def test_mirror_inner_left_right_over_multi_batch_children(ctx, pp, use_rewrite):
    from naive_query_engine_amd.rewrite import rewrite

    rng = np.random.default_rng(21)
    n, m = 150, 2600
    left = [i64(rng.integers(0, 9, n)), oju.utf8_column([f"n{v}" for v in rng.integers(0, 7, n)]), i64(np.arange(n))]
    right = [i64(np.arange(m)), oju.utf8_column([f"n{v}" for v in rng.integers(0, 8, m)]), i64(rng.integers(0, 10, m))]
    lnames, rnames = ["a", "s", "row"], ["rid", "s2", "a2"]
    lschema, rschema = [Field(nm, c.dtype) for nm, c in zip(lnames, left)], [Field(nm, c.dtype) for nm, c in zip(rnames, right)]
    lb, rb = _batches(left, lnames, [40, 150]), _batches(right, rnames, [1000, 2600])
    ls, rs = pp.ScanPlan.create(pp.MemTable.try_create(lschema, lb, ctx)), pp.ScanPlan.create(pp.MemTable.try_create(rschema, rb, ctx))
    on = [(pp.ColumnRef(None, "a"), pp.ColumnRef(None, "a2")), (pp.ColumnRef(None, "s"), pp.ColumnRef(None, "s2"))]
    rparts = [list(b.columns) for b in rb]
    for jtype, how in ((pp.JoinType.Inner, "inner"), (pp.JoinType.Left, "left"), (pp.JoinType.Right, "right")):
        plan = pp.MultiKeyHashJoin.create(ls, rs, on, jtype, lschema + rschema)
        if use_rewrite:
            plan = rewrite(plan)
            assert isinstance(plan, pp.MultiKeyHashJoin)
        exp = jku.expected_batches(left, [0, 1], rparts, [2, 1], how)
        for execution in range(2):  # nothing is kept between execute() calls
            out = plan.execute()
            assert len(out) == len(exp)
            for bi, (cols, _, _) in enumerate(exp):
                oju.assert_same_columns(out[bi].table.to_host(), cols, f"{how} execution {execution} batch {bi}")
                assert [f.name for f in out[bi].fields] == lnames + rnames
        # one pair: HashOuterJoin's batches
        one = pp.MultiKeyHashJoin.create(ls, rs, on[:1], jtype, lschema + rschema).execute()
        ref = pp.HashOuterJoin.create(ls, rs, on[:1], jtype, lschema + rschema).execute()
        assert len(one) == len(ref)
        for a, b in zip(one, ref):
            oju.assert_same_columns(a.table.to_host(), b.table.to_host(), f"{how}: one pair vs HashOuterJoin")
    with pytest.raises(ErrorCode) as e:
        pp.MultiKeyHashJoin.create(ls, rs, on, pp.JoinType.Cross, lschema + rschema).execute()
    assert e.value.status == Status.PlanError
    with pytest.raises(ErrorCode) as e:
        pp.MultiKeyHashJoin.create(ls, rs, [], pp.JoinType.Left, lschema + rschema).execute()
    assert e.value.status == Status.PlanError
    # HashJoin keeps reading on[0] alone (quirk Q11 / Q21)
    inner = pp.HashJoin.create(ls, rs, on, pp.JoinType.Inner, lschema + rschema).execute()
    assert sum(b.num_rows for b in inner) > sum(len(p) for p in jku.join_pairs(left, [0, 1], rparts, [2, 1], "inner"))


# ----------------------------------------------------------------------------- seeded sweep
def _random_key(rng, kind, n, card):
    v = rng.integers(0, card, n)
    if kind == "i":
        return i64(v - card // 2), None
    if kind == "u":
        return u64(v.astype(np.uint64) + np.uint64(2**63 - 1)), None
    return oju.utf8_column([("k%d" % x) * int(x % 3) for x in v]), None


def _payload(rng, n):
    kind = int(rng.integers(0, 4))
    mask = rng.random(n) > 0.3 if n and rng.random() < 0.7 else None
    if kind == 0:
        return f64(rng.normal(0, 1, n), mask)
    if kind == 1:
        return Column.from_numpy(rng.random(n) < 0.5, mask)
    if kind == 2:
        items = [None if (mask is not None and not mask[i]) else "p%d" % i for i in range(n)]
        return oju.utf8_column(items)
    return Column.from_numpy(rng.integers(-100, 100, n).astype(np.int64), mask)


@pytest.mark.parametrize("chunk", range(6))
def test_seeded_sweep(ctx, chunk):
    for seed in range(chunk * 6, chunk * 6 + 6):
        rng = np.random.default_rng(5000 + seed)
        k = int(rng.integers(2, 5))
        kinds = [str(rng.choice(["i", "u", "s"], p=[0.5, 0.25, 0.25])) for _ in range(k)]
        nb, m = int(rng.integers(0, 5001)), int(rng.integers(0, 5001))
        card = int(rng.integers(2, 12))
        lk = [_random_key(rng, kd, nb, card)[0] for kd in kinds]
        rk = [_random_key(rng, kd, m, card + 1)[0] for kd in kinds]
        left = lk + [_payload(rng, nb), i64(np.arange(nb))]
        right = [_payload(rng, m)] + rk + [_payload(rng, m)]
        how = jku.HOWS[seed % 4]
        cut = m // 3
        batches = [oju.take_null(right, np.arange(0, cut)), oju.take_null(right, np.arange(cut, m))] if seed % 2 else [right]
        integer = "s" not in kinds
        run_join(ctx, left, list(range(k)), batches, list(range(1, k + 1)), how, path="pack" if integer else "dict", what=f"seed {seed} kinds {kinds} {nb} x {m}")
        if integer:
            run_join(ctx, left, list(range(k)), batches, list(range(1, k + 1)), how, dict_forced=True, path="dict", what=f"seed {seed} kinds {kinds} {nb} x {m}")
