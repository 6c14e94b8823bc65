"""Outer hash joins on the device (nqe_hash_join_probe_outer / nqe_hash_join_unmatched_build, csrc/hash_join_outer_kernels.hpp; quirk
Q19: HashJoin honouring join_type, with the inner hash join's match relation).

The yardstick is the numpy / dict model of tests/outer_join_util.py (checked against pyarrow in tests/test_outer_join_host.py).  Every
comparison is bit for bit: the operator only compares and copies.

Not run here: a build side of 2^32 rows (the size the outer probe refuses because of its no-match mark) needs a 32 GB key column, and
nqe_hash_join_build refuses that size first; the check is a host comparison in front of every launch and is left to code reading."""
import ctypes as C
import gc
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import outer_join_util as oju  # noqa: E402
from naive_query_engine_amd import Column, DType, ErrorCode, Field, RecordBatch, Status  # noqa: E402

pytestmark = pytest.mark.gpu
I64 = np.iinfo(np.int64)


@pytest.fixture(scope="module")
def pp():
    from naive_query_engine_amd import physical_plan

    return physical_plan


@pytest.fixture(scope="module")
def ctx():
    from naive_query_engine_amd import capi

    return capi.default_context()


def i64(a):
    return Column.from_numpy(np.asarray(a, dtype=np.int64))


# ----------------------------------------------------------------------------- build forms (the map at the top of hash_join.hip)
def _unique_sparse_keys(rng, n):
    return np.unique(rng.integers(-(1 << 40), 1 << 40, 2 * n + 8))[:n][rng.permutation(n)].astype(np.int64) if n else np.zeros(0, np.int64)


def form_dense_full(rng, n):  # build_unique_dense: gap-free range, plain payload (dense_full)
    return [i64(rng.permutation(n) + 1000), i64(rng.integers(-5, 5, n))]


def form_dense_gaps(rng, n):  # build_unique_dense with gaps (presence bitmap)
    return [i64(rng.permutation(2 * n)[:n] - 7), Column.from_numpy(rng.normal(0, 1, n))]


def form_sparse_packed(rng, n):  # build_hashed_unique: one packable payload (packed pairs)
    return [i64(rng.integers(0, 1000, n)), i64(_unique_sparse_keys(rng, n))]  # key is column 1


def form_sparse_pairs(rng, n):  # build_hashed_unique: one payload over the full 64-bit range (16-byte pairs)
    pay = rng.integers(I64.min, I64.max, n, dtype=np.int64, endpoint=True)
    if n >= 2:
        pay[:2] = [I64.min, I64.max]
    return [i64(_unique_sparse_keys(rng, n)), i64(pay)]


def form_sparse_check(rng, n):  # build_hashed_unique: two payloads (the check form)
    return [i64(_unique_sparse_keys(rng, n)), i64(rng.integers(0, 9, n)), Column.from_numpy(rng.normal(0, 1, n))]


def form_dup_dense(rng, n):  # build_sorted + build_sorted_dense: duplicate keys over a dense range
    return [i64(rng.integers(0, max(1, n // 3), n)), i64(np.arange(n))]


def form_dup_sparse(rng, n):  # build_sorted: duplicate keys, hashed
    pool = _unique_sparse_keys(rng, max(1, n // 3))
    return [i64(pool[rng.integers(0, pool.size, n)] if n else pool[:0]), i64(np.arange(n))]


def form_utf8(rng, n):  # Utf8 key (non-null): dictionary codes; duplicates about every third row
    return [oju.utf8_column([f"key-{int(v)}-{'x' * int(v % 5)}" for v in rng.integers(0, max(1, (2 * n) // 3), n)]), i64(np.arange(n))]


FORMS = {"dense_full": (form_dense_full, 0), "dense_gaps": (form_dense_gaps, 0), "sparse_packed": (form_sparse_packed, 1), "sparse_pairs": (form_sparse_pairs, 0),
         "sparse_check": (form_sparse_check, 0), "dup_dense": (form_dup_dense, 0), "dup_sparse": (form_dup_sparse, 0), "utf8": (form_utf8, 0)}


def probe_side(rng, build_key, m, miss=0.3):
    """m probe rows: keys drawn from the build keys, about `miss` of them replaced by keys the build side does not have"""
    if build_key.dtype == DType.UTF8:
        raw = oju.utf8_raw(build_key)
        items = [raw[int(i)] if raw and rng.random() >= miss else b"absent-%d" % int(i) for i in rng.integers(0, max(1, len(raw)), m)]
        return [i64(np.arange(m) * 3), oju.utf8_column(items)]
    bk = build_key.to_numpy()
    keys = bk[rng.integers(0, bk.size, m)].copy() if bk.size else np.zeros(m, np.int64)
    absent = rng.random(m) < miss
    keys[absent] = (I64.max - rng.integers(0, 1000, m))[absent]  # no build key is that large
    return [i64(np.arange(m) * 3), i64(keys)]  # key is column 1


def check_table(t, exp, what, zero_rows=None):
    got = t.to_host()
    oju.assert_same_columns(got, exp, what, zero_rows=zero_rows)
    for i, e in enumerate(exp):
        assert int(t.column_info(i).null_count) == e.null_count, f"{what} column {i}: null_count {t.column_info(i).null_count}, expected {e.null_count}"
    return got


def check_unmatched(ctx, jt, marks, left, lkey, probe_keys, dts, what):
    """the final batch of the build-preserving join: left columns against the model, and 0 / false / the empty string in every cell of
    the all-NULL right columns"""
    exp = oju.unmatched_batch(left, lkey, probe_keys, dts)
    rows = exp[0].length if exp else 0
    zero_rows = [None] * len(left) + [np.ones(rows, dtype=bool)] * len(dts)
    return check_table(ctx.hash_join_unmatched_build(jt, marks, dts), exp, what, zero_rows)


def check_probe(ctx, jt, left, lkey, right, rkey, keep_probe, marks, what):
    rt = ctx.table_from_host(right)
    t = ctx.hash_join_probe_outer(jt, rt, rkey, keep_probe=keep_probe, marks=marks)
    xs, _ = oju.probe_pairs(left[lkey], right[rkey], keep_probe)
    nullx = np.asarray(xs, dtype=np.int64) < 0
    zero_rows = [nullx] * len(left) + [None] * len(right)
    return check_table(t, oju.outer_probe(left, lkey, right, rkey, keep_probe), what, zero_rows), rt


def run_form(ctx, left, lkey, batches, rkey, what):
    """every flags x marks combination over the probe batches, the inner join for flags = 0 / marks = NULL, then the unmatched pass"""
    lt = ctx.table_from_host(left)
    jt = ctx.hash_join_build(lt, lkey)
    for keep_probe in (False, True):
        for with_marks in (False, True):
            marks = ctx.join_marks(jt) if with_marks else None
            for bi, right in enumerate(batches):
                w = f"{what} keep_probe={keep_probe} marks={with_marks} batch {bi}"
                got, rt = check_probe(ctx, jt, left, lkey, right, rkey, keep_probe, marks, w)
                if not keep_probe and not with_marks:  # bit for bit the inner join's output
                    oju.assert_same_columns(got, ctx.hash_join_probe(jt, rt, rkey).to_host(), w + " vs hash_join_probe")
            if with_marks:
                dts = [c.dtype for c in batches[0]]
                check_unmatched(ctx, jt, marks, left, lkey, [b[rkey] for b in batches], dts, f"{what} keep_probe={keep_probe} unmatched")
    # fresh marks: nothing matched yet, every build row comes back
    check_unmatched(ctx, jt, ctx.join_marks(jt), left, lkey, [], [DType.INT64, DType.BOOLEAN, DType.UTF8, DType.FLOAT64, DType.UINT64], f"{what} unmatched with fresh marks")


@pytest.mark.parametrize("form", list(FORMS))
def test_every_build_form(ctx, form):
    make, lkey = FORMS[form]
    rng = np.random.default_rng(sorted(FORMS).index(form))
    left = make(rng, 301)
    # the second batch draws from the first 100 build rows only: the marks of two batches differ and some build rows stay unmatched
    head = [Column.from_numpy(c.to_numpy()[:100]) if c.dtype != DType.UTF8 else oju.utf8_column(oju.utf8_raw(c)[:100]) for c in left]
    batches = [probe_side(rng, head[lkey], 5000), probe_side(rng, head[lkey], 1025, miss=0.6)]
    run_form(ctx, left, lkey, batches, 1, form)


def test_unique_build_across_the_scatter_threshold(ctx):
    rng = np.random.default_rng(70000)
    left = form_dense_gaps(rng, 70000)  # >= 2^16 rows: the scatter / finish form of the dense build
    batches = [probe_side(rng, i64(left[0].to_numpy()[:30000]), 20000), probe_side(rng, i64(left[0].to_numpy()[:1000]), 4097, miss=0.5)]
    run_form(ctx, left, 0, batches, 1, "70000-row build")


# ----------------------------------------------------------------------------- size edges
PROBE_ROWS = [0, 1, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, 3 * 4096 + 17]  # wave, sub-tile and tile edges; a line-unaligned out_base
BUILD_ROWS = [0, 1, 31, 32, 33, 63, 64, 65, 4097]  # the edges of the marks words


@pytest.mark.parametrize("m", PROBE_ROWS)
def test_probe_row_counts_at_the_tile_edges(ctx, m):
    rng = np.random.default_rng(m)
    for form in ("dup_dense", "sparse_check"):
        make, lkey = FORMS[form]
        left = make(rng, 97)
        lt = ctx.table_from_host(left)
        jt = ctx.hash_join_build(lt, lkey)
        right = probe_side(rng, left[lkey], m)
        marks = ctx.join_marks(jt)
        for keep_probe in (False, True):
            check_probe(ctx, jt, left, lkey, right, 1, keep_probe, marks, f"{form} m={m} keep_probe={keep_probe}")
        check_unmatched(ctx, jt, marks, left, lkey, [right[1]], [DType.INT64, DType.INT64], f"{form} m={m} unmatched")


@pytest.mark.parametrize("n", BUILD_ROWS)
def test_build_row_counts_at_the_marks_word_edges(ctx, n):
    rng = np.random.default_rng(1000 + n)
    for form in ("dense_gaps", "dup_sparse", "utf8"):
        make, lkey = FORMS[form]
        left = make(rng, n)
        lt = ctx.table_from_host(left)
        jt = ctx.hash_join_build(lt, lkey)
        # the last build row matches (bit n - 1), the first one does not unless it shares the key
        if n:
            last = i64(left[lkey].to_numpy()[n - 1:]) if form != "utf8" else oju.utf8_column(oju.utf8_raw(left[lkey])[n - 1:])
            right = probe_side(rng, last, 70, miss=0.5)
        else:
            right = probe_side(rng, left[lkey], 70)
        marks = ctx.join_marks(jt)
        for keep_probe in (True, False):
            check_probe(ctx, jt, left, lkey, right, 1, keep_probe, marks, f"{form} n={n} keep_probe={keep_probe}")
        dts = [c.dtype for c in right]
        check_unmatched(ctx, jt, marks, left, lkey, [right[1]], dts, f"{form} n={n} unmatched")


# ----------------------------------------------------------------------------- payload types
def payload_columns(rng, n):
    """nullable Int64, Float64 with NaN payloads and -0.0, Boolean with validity, Utf8 with NULLs and empty strings"""
    f = rng.normal(0, 1, n)
    if n:
        f.view(np.uint64)[rng.integers(0, n, max(1, n // 4))] = rng.choice(np.array([0x8000000000000000, 0x7ff8000000001234, 0xfff0000000000001, 0x7ff0000000000000], dtype=np.uint64),
                                                                           max(1, n // 4))
    words = [None, "", "a", "été", "abcdefghijklmnopqrstuvwxyz"]
    return [Column.from_numpy(rng.integers(I64.min, I64.max, n, dtype=np.int64), rng.random(n) > 0.3), Column.from_numpy(f), Column.from_numpy(rng.random(n) < 0.5, rng.random(n) > 0.3),
            oju.utf8_column([words[int(i)] for i in rng.integers(0, len(words), n)])]


@pytest.mark.parametrize("dup", [False, True])
def test_payload_types_validity_presence_and_null_count(ctx, dup):
    rng = np.random.default_rng(11 + dup)
    n, m = 203, 1500
    lk = rng.integers(0, 60, n) if dup else rng.permutation(n) * 5
    left = [i64(lk)] + payload_columns(rng, n)
    right = payload_columns(rng, m) + [i64(rng.integers(0, 80, m) if dup else rng.integers(0, n * 6, m))]
    rkey = len(right) - 1
    lt = ctx.table_from_host(left)
    jt = ctx.hash_join_build(lt, 0)
    marks = ctx.join_marks(jt)
    got, _ = check_probe(ctx, jt, left, 0, right, rkey, True, marks, "payloads keep_probe")
    xs, _ = oju.probe_pairs(left[0], right[rkey], True)
    assert -1 in xs and got[0].validity is not None and got[2].validity is not None  # NULL-extended rows: the plain key and Float64 columns get a bitmap
    got, _ = check_probe(ctx, jt, left, 0, right, rkey, False, None, "payloads inner")
    assert got[0].validity is None and got[2].validity is None and got[1].validity is not None  # none without such rows; a nullable source keeps its own
    # a batch in which every probe row matches has no NULL-extended row: no bitmap on the plain columns even with KEEP_PROBE
    hit = [c for c in oju.take_null(right, [y for x, y in zip(*oju.probe_pairs(left[0], right[rkey], False))][:300])]
    hit = [Column(c.dtype, c.length, c.values, c.validity if oju.has_nulls(c) else None, c.data) for c in hit]
    got, _ = check_probe(ctx, jt, left, 0, hit, rkey, True, None, "payloads keep_probe, all match")
    assert got[0].validity is None and got[2].validity is None
    dts = [c.dtype for c in right]
    check_unmatched(ctx, jt, marks, left, 0, [right[rkey]], dts, "payloads unmatched")


def test_a_null_key_slot_that_equals_a_real_key_matches(ctx):
    left = [Column.from_numpy(np.array([5, 7, 9], dtype=np.int64), np.array([True, False, True])), i64([10, 20, 30])]
    right = [Column.from_numpy(np.array([7, 8, 5], dtype=np.int64), np.array([False, True, True]))]
    lt = ctx.table_from_host(left)
    jt = ctx.hash_join_build(lt, 0)
    marks = ctx.join_marks(jt)
    got, _ = check_probe(ctx, jt, left, 0, right, 0, True, marks, "null key slot")
    assert got[1].to_list() == [20, None, 10]  # the NULL slot 7 matched build row 1 (Q11 / Q19); 8 matched nothing
    t = ctx.hash_join_unmatched_build(jt, marks, [DType.INT64])
    assert t.to_host()[1].to_list() == [30]


# ----------------------------------------------------------------------------- mirrors
def _batches(cols, names, cuts):
    out, lo = [], 0
    for hi in cuts:
        idx = np.arange(lo, hi)
        out.append(RecordBatch([Field(nm, c.dtype, True) for nm, c in zip(names, cols)], oju.take_null(cols, idx)))
        lo = hi
    return out


@pytest.mark.parametrize("dup", [False, True])
def test_mirror_inner_left_right_over_multi_batch_children(ctx, pp, dup):
    rng = np.random.default_rng(21 + dup)
    n, m = 150, 2600
    left = [i64(rng.integers(0, 50, n) if dup else rng.permutation(n)), oju.utf8_column([f"n{i}" for i in range(n)])]
    right = [i64(np.arange(m)), i64(rng.integers(0, 70 if dup else 200, m))]
    lschema = [Field("id", DType.INT64), Field("name", DType.UTF8)]
    rschema = [Field("rid", DType.INT64), Field("fk", DType.INT64)]
    lb = _batches(left, ["id", "name"], [40, 150])
    rb = _batches(right, ["rid", "fk"], [1000, 1001, 2600])
    ls = pp.ScanPlan.create(pp.MemTable.try_create(lschema, lb, ctx))
    rs = pp.ScanPlan.create(pp.MemTable.try_create(rschema, rb, ctx))
    on = [(pp.ColumnRef(None, "id"), pp.ColumnRef(None, "fk"))]
    rparts = [[c for c in b.columns] for b in rb]
    for jtype, keep in ((pp.JoinType.Inner, False), (pp.JoinType.Left, False), (pp.JoinType.Right, True)):
        plan = pp.HashOuterJoin.create(ls, rs, on, jtype, lschema + rschema)
        for execution in range(2):  # nothing is kept between execute() calls: the second result is the first
            out = plan.execute()
            assert len(out) == len(rb) + (1 if jtype == pp.JoinType.Left else 0)
            for bi, part in enumerate(rparts):
                oju.assert_same_columns(out[bi].table.to_host(), oju.outer_probe(left, 0, part, 1, keep), f"type {jtype} execution {execution} batch {bi}")
            if jtype == pp.JoinType.Left:
                exp = oju.unmatched_batch(left, 0, [p[1] for p in rparts], [DType.INT64, DType.INT64])
                oju.assert_same_columns(out[-1].table.to_host(), exp, f"execution {execution} final batch")
                assert [f.name for f in out[-1].fields] == ["id", "name", "rid", "fk"]
    # a probe side without batches: Left gives the final batch alone (every build row), Right and Inner nothing
    empty = pp.ScanPlan.create(pp.MemTable.try_create(rschema, [], ctx))
    out = pp.HashOuterJoin.create(ls, empty, on, pp.JoinType.Left, lschema + rschema).execute()
    assert len(out) == 1
    oju.assert_same_columns(out[0].table.to_host(), oju.unmatched_batch(left, 0, [], [DType.INT64, DType.INT64]), "no right batches")
    assert pp.HashOuterJoin.create(ls, empty, on, pp.JoinType.Right, lschema + rschema).execute() == []
    with pytest.raises(ErrorCode) as e:
        pp.HashOuterJoin.create(ls, rs, on, pp.JoinType.Cross, lschema + rschema).execute()
    assert e.value.status == Status.PlanError
    with pytest.raises(ErrorCode) as e:
        pp.HashOuterJoin.create(ls, rs, [], pp.JoinType.Left, lschema + rschema).execute()
    assert e.value.status == Status.PlanError


# ----------------------------------------------------------------------------- errors
def _status(ctx, fn, *args):
    from naive_query_engine_amd import capi

    h = C.c_void_p()
    st = fn(ctx.handle, *args, C.byref(h))
    if st == 0 and h.value:
        capi.Table(ctx, h)  # released by its destructor
    return st


def test_errors(ctx):
    from naive_query_engine_amd import capi

    L = capi.lib()
    lt = ctx.table_from_host([i64([1, 2, 3]), i64([4, 5, 6])])
    other = ctx.table_from_host([i64([1, 2, 3])])
    rt = ctx.table_from_host([i64([1, 2]), Column.from_numpy(np.array([1.0, 2.0])), Column.from_numpy(np.array([1, 2], dtype=np.uint64))])
    jt, jt2 = ctx.hash_join_build(lt, 0), ctx.hash_join_build(other, 0)
    marks, marks2 = ctx.join_marks(jt), ctx.join_marks(jt2)
    one = (C.c_int32 * 1)(int(DType.INT64))
    assert _status(ctx, L.nqe_hash_join_probe_outer, jt.handle, rt.handle, 0, 2, None) == Status.InvalidArgument  # unknown flag bits
    assert _status(ctx, L.nqe_hash_join_probe_outer, jt.handle, rt.handle, 0, 0x80000001, None) == Status.InvalidArgument
    assert _status(ctx, L.nqe_hash_join_probe_outer, jt.handle, rt.handle, 0, 1, marks2.handle) == Status.InvalidArgument  # marks of another table
    assert _status(ctx, L.nqe_hash_join_unmatched_build, jt.handle, marks2.handle, one, 1) == Status.InvalidArgument
    assert _status(ctx, L.nqe_hash_join_unmatched_build, jt.handle, None, one, 1) == Status.InvalidArgument  # NULL marks
    other_ctx = capi.Context(0)  # marks are bound to the context they were created on as well
    try:
        assert _status(other_ctx, L.nqe_hash_join_probe_outer, jt.handle, rt.handle, 0, 0, marks.handle) == Status.InvalidArgument
        assert _status(other_ctx, L.nqe_hash_join_unmatched_build, jt.handle, marks.handle, one, 1) == Status.InvalidArgument
        assert _status(other_ctx, L.nqe_join_marks_create, jt.handle) == Status.InvalidArgument
    finally:
        other_ctx.close()
    assert _status(ctx, L.nqe_hash_join_unmatched_build, jt.handle, marks.handle, one, -1) == Status.InvalidArgument  # num_right < 0
    for bad in (6, -1, 99):
        assert _status(ctx, L.nqe_hash_join_unmatched_build, jt.handle, marks.handle, (C.c_int32 * 2)(int(DType.INT64), bad), 2) == Status.InvalidArgument
    # as nqe_hash_join_probe: key index, key dtypes, the 32-column limit
    for keep in (0, 1):
        assert _status(ctx, L.nqe_hash_join_probe_outer, jt.handle, rt.handle, 3, keep, None) == _status(ctx, L.nqe_hash_join_probe, jt.handle, rt.handle, 3) == Status.LogicalError
        assert _status(ctx, L.nqe_hash_join_probe_outer, jt.handle, rt.handle, -1, keep, None) == Status.LogicalError
        assert _status(ctx, L.nqe_hash_join_probe_outer, jt.handle, rt.handle, 1, keep, None) == _status(ctx, L.nqe_hash_join_probe, jt.handle, rt.handle, 1) == Status.NotImplemented
        assert _status(ctx, L.nqe_hash_join_probe_outer, jt.handle, rt.handle, 2, keep, None) == _status(ctx, L.nqe_hash_join_probe, jt.handle, rt.handle, 2) == Status.NotSupported
    wide = ctx.table_from_host([i64([1, 2])] * 31)
    assert _status(ctx, L.nqe_hash_join_probe_outer, jt.handle, wide.handle, 0, 1, marks.handle) == _status(ctx, L.nqe_hash_join_probe, jt.handle, wide.handle, 0) == Status.NotSupported
    assert _status(ctx, L.nqe_hash_join_unmatched_build, jt.handle, marks.handle, (C.c_int32 * 31)(*[int(DType.INT64)] * 31), 31) == Status.NotSupported
    # the refused calls launched nothing and marked nothing: every build row is still unmatched
    assert ctx.hash_join_unmatched_build(jt, marks, []).num_rows == 3


@pytest.mark.parametrize("keep_probe", [False, True])
def test_a_probe_tile_beyond_2p32_output_rows_is_out_of_memory(ctx, keep_probe):
    """2^20 + 1 build rows of one key (8 MB) probed by one 4096-row tile of that key: 4096 x 1048577 > 2^32 - 1 output rows.  The count
    pass runs (it is how the size is known) and has set the marks of the refused batch (include/nqe.h says so); nothing of the output's
    size is allocated and the write pass is not launched"""
    n = (1 << 20) + 1
    assert 4096 * n > 0xFFFFFFFF
    lt = ctx.table_from_host([i64(np.full(n, 42))])
    rt = ctx.table_from_host([i64(np.full(4096, 42))])
    jt = ctx.hash_join_build(lt, 0)
    marks = ctx.join_marks(jt)
    ctx.synchronize()
    gc.collect()
    live = ctx.memory_stats()[0]
    ctx.timing_enable(True)
    ctx.timing_reset()
    try:
        with pytest.raises(ErrorCode) as e:
            ctx.hash_join_probe_outer(jt, rt, 0, keep_probe=keep_probe, marks=marks)
        assert e.value.status == Status.OutOfMemory
        assert ctx.timing_query("join_outer_count")[1] == 1 and ctx.timing_query("join_outer_write")[1] == 0 and ctx.timing_query("take")[1] == 0
    finally:
        ctx.timing_enable(False)
        ctx.timing_reset()
    gc.collect()
    assert ctx.memory_stats()[0] == live
    assert ctx.hash_join_unmatched_build(jt, marks, [DType.INT64]).num_rows == 0  # the count pass of the refused call marked the key
    # one row fewer per tile fits: 4095 probe rows of the key are 4095 x 1048577 < 2^32 output rows — too many to materialise here, so
    # the accepted side of the bound is shown on a key the build side does not have
    miss = ctx.table_from_host([i64(np.full(4096, 7))])
    assert ctx.hash_join_probe_outer(jt, miss, 0, keep_probe=keep_probe, marks=marks).num_rows == (4096 if keep_probe else 0)


def _free_device_bytes():
    """hipMemGetInfo of the HIP runtime the library has loaded into this process (a second runtime — torch's — finds no device once
    the first one holds it); 0 when it cannot be asked"""
    try:
        with open("/proc/self/maps") as f:
            path = next(line.split()[-1] for line in f if "libamdhip64" in line)
        free, total = C.c_size_t(), C.c_size_t()
        return int(free.value) if C.CDLL(path).hipMemGetInfo(C.byref(free), C.byref(total)) == 0 else 0
    except Exception:
        return 0


@pytest.mark.timeout(900)
@pytest.mark.parametrize("entry", ["inner", "outer", "outer_keep_probe"])
def test_a_sub_tile_of_exactly_2p31_output_rows(ctx, entry):
    """2^21 build rows of one key (payload = the row number) probed by 1024 rows of that key: ONE 1024-row sub-tile of the write pass
    expands to exactly 2^31 output rows, the smallest shape at which a signed 32-bit position inside a sub-tile goes negative (the whole
    4096-row tile is what is bounded, at 2^32).  The output — one key buffer both key columns share and the payload column, 32 GB — is
    checked on the device: count, min and max of every column, the exact payload sum, and ten rows at three offsets.
    Observed on the commit before the inner entry's positions became 64-bit: the inner case failed at the first value check (minimum
    of the key column 0 instead of 42: 2^31 rows were returned and none had been written — the loop `j0 < int32_t(total)` never ran,
    no error was raised), the two outer cases passed."""
    from naive_query_engine_amd import AggregateFunc as A

    if _free_device_bytes() < 48 * 2**30:
        pytest.skip("needs 48 GB of free device memory")
    nb, m, key = 1 << 21, 1024, 42
    lt = ctx.table_from_host([i64(np.full(nb, key)), i64(np.arange(nb))])
    rt = ctx.table_from_host([i64(np.full(m, key))])
    jt = ctx.hash_join_build(lt, 0)
    if entry == "inner":
        out = ctx.hash_join_probe(jt, rt, 0)
    else:
        out = ctx.hash_join_probe_outer(jt, rt, 0, keep_probe=entry == "outer_keep_probe", marks=None)
    assert out.num_rows == 2**31 and out.num_columns == 3
    cnt, kmin, kmax, pmin, pmax, psum, rmin, rmax = [float(c.to_numpy()[0]) for c in
                                                    ctx.aggregate(out, [(A.Count, 0), (A.Min, 0), (A.Max, 0), (A.Min, 1), (A.Max, 1), (A.Sum, 1), (A.Min, 2), (A.Max, 2)]).to_host()]
    assert cnt == 2.0**31
    assert kmin == kmax == rmin == rmax == float(key)
    assert pmin == 0.0 and pmax == float(nb - 1)
    assert m * nb * (nb - 1) // 2 < 2**53 and psum == float(m * nb * (nb - 1) // 2)  # every partial sum is an integer below 2^53: exact
    for off in (0, nb - 5, 2**31 - 10):  # probe-row-major, ascending build row inside a probe row
        k, p, r = [c.to_numpy() for c in ctx.slice(out, off, 10).to_host()]
        assert (p == (off + np.arange(10)) % nb).all() and (k == key).all() and (r == key).all(), f"{entry}: rows at {off}: {p}"
    del out
    gc.collect()


# ----------------------------------------------------------------------------- one expand path, two entries
AGREE_ROWS = [0, 1, 1023, 1024, 1025, 4096, 4097]  # probe rows: the sub-tile (1024) and tile (4096) edges of the two passes


def check_entries_agree(ctx, jt, right, rkey, what, duplicates):
    """hash_join_probe and hash_join_probe_outer(keep_probe=False, marks=None) over one table: dtypes, values, validity bits (and
    whether a bitmap is there) and null counts.  The outer entry reports the exact null count of every column; the inner entry reports
    it or -1 (not counted), as it always has — what is compared is the number of NULLs under both outputs."""
    rt = ctx.table_from_host(right)
    labels = ("join_probe_count", "join_probe_write", "join_outer_count", "join_outer_write")
    ctx.timing_enable(True)
    ctx.timing_reset()
    try:
        a = ctx.hash_join_probe(jt, rt, rkey)
        b = ctx.hash_join_probe_outer(jt, rt, rkey, keep_probe=False, marks=None)
        launches = [ctx.timing_query(name)[1] for name in labels]
    finally:
        ctx.timing_enable(False)
        ctx.timing_reset()
    assert a.dtypes() == b.dtypes(), what
    ga, gb = a.to_host(), b.to_host()
    oju.assert_same_columns(ga, gb, what)
    for i, (x, y) in enumerate(zip(ga, gb)):
        nulls = int(y.length - y.valid_mask().sum())
        assert int(x.length - x.valid_mask().sum()) == nulls
        assert int(b.column_info(i).null_count) == nulls and int(a.column_info(i).null_count) in (nulls, -1), f"{what} column {i}"
    if duplicates:  # one count pass per entry, and one write pass where there is anything to write
        m, rows = right[rkey].length, a.num_rows
        assert launches == [int(m > 0), int(rows > 0), int(m > 0), int(rows > 0)], f"{what}: {dict(zip(labels, launches))}"
    return a.num_rows


@pytest.mark.parametrize("form", list(FORMS))
def test_inner_and_outer_entries_agree_on_every_build_form(ctx, form):
    make, lkey = FORMS[form]
    rng = np.random.default_rng(300 + sorted(FORMS).index(form))
    left = make(rng, 301)
    lt = ctx.table_from_host(left)
    jt = ctx.hash_join_build(lt, lkey)
    for m in AGREE_ROWS:
        check_entries_agree(ctx, jt, probe_side(rng, left[lkey], m), 1, f"{form} m={m}", form in ("dup_dense", "dup_sparse", "utf8"))


def _payload(kind, rng, n):
    if kind == "plain":
        return Column.from_numpy(rng.integers(I64.min, I64.max, n, dtype=np.int64))
    return payload_columns(rng, n)[{"nullable": 0, "boolean": 2, "utf8": 3}[kind]]


@pytest.mark.parametrize("m", AGREE_ROWS)
@pytest.mark.parametrize("kind", ["plain", "nullable", "boolean", "utf8"])
def test_inner_and_outer_entries_agree_on_duplicate_keys(ctx, kind, m):
    """key k occurs k % 5 + 1 times on the build side: a 1024-row sub-tile expands to about 3000 rows — several steps of the write
    loop (1024 output rows each) — and the output base of every later sub-tile sits anywhere inside its 128-byte line (base & 15)"""
    rng = np.random.default_rng(900 + m)
    keys = np.repeat(np.arange(200), np.arange(200) % 5 + 1)
    keys = keys[rng.permutation(keys.size)]
    left = [i64(keys), _payload(kind, rng, keys.size)]
    right = [_payload(kind, rng, m), i64(rng.integers(0, 250, m))]  # a fifth of the probe keys match nothing
    lt = ctx.table_from_host(left)
    jt = ctx.hash_join_build(lt, 0)
    rows = check_entries_agree(ctx, jt, right, 1, f"{kind} m={m}", True)
    assert rows == int(np.bincount(keys, minlength=250)[right[1].to_numpy()].sum())
    if m >= 1023:
        assert rows > 2 * 1024


# ----------------------------------------------------------------------------- a seeded sweep
def _random_case(seed):
    rng = np.random.default_rng(5000 + seed)
    form = sorted(FORMS)[int(rng.integers(0, len(FORMS)))]
    make, lkey = FORMS[form]
    n = int(rng.choice([1, 2, 33, 64, 100, 1000, 4097, 20000]))
    left = make(rng, n)
    extra = payload_columns(rng, n)
    left = left + [extra[int(i)] for i in rng.integers(0, len(extra), int(rng.integers(0, 3)))]
    batches = []
    for _ in range(int(rng.integers(1, 3))):
        m = int(rng.choice([0, 1, 65, 1000, 4096, 5000, 20000]))
        right = probe_side(rng, left[lkey], m, miss=float(rng.choice([0.0, 0.1, 0.9])))
        pay = payload_columns(rng, m)
        batches.append(right + [pay[int(i)] for i in sorted(rng.integers(0, len(pay), 2).tolist())])
    return form, left, lkey, batches


@pytest.mark.parametrize("chunk", range(8))
def test_seeded_sweep(ctx, chunk):
    for seed in range(chunk * 5, chunk * 5 + 5):
        form, left, lkey, batches = _random_case(seed)
        # the payload columns drawn per batch differ between batches in dtype: one set of dtypes per case
        batches = [b for b in batches if [c.dtype for c in b] == [c.dtype for c in batches[0]]]
        lt = ctx.table_from_host(left)
        jt = ctx.hash_join_build(lt, lkey)
        keep_probe, with_marks = bool(seed & 1), bool(seed & 2)
        marks = ctx.join_marks(jt) if with_marks else None
        for bi, right in enumerate(batches):
            check_probe(ctx, jt, left, lkey, right, 1, keep_probe, marks, f"seed {seed} ({form}) batch {bi}")
        if with_marks:
            dts = [c.dtype for c in batches[0]]
            check_unmatched(ctx, jt, marks, left, lkey, [b[1] for b in batches], dts, f"seed {seed} ({form}) unmatched")
