"""Semi and anti hash joins on the device (nqe_hash_join_probe_semi / nqe_hash_join_marked_build, csrc/hash_join_semi_kernels.hpp; quirk
Q22: which rows of one table have a partner in the other, with the inner hash join's match relation).

The yardstick is the numpy / dict model of tests/semi_join_util.py (checked against pyarrow in tests/test_semi_join_host.py), and the
library itself: SEMI's rows are the distinct probe rows of the inner join, SEMI and ANTI partition the batch, build ANTI is the outer
join's tail.  Every comparison is bit for bit: the operator only compares and copies.  The sizes are the edges of the 64-row keep word
and of the 4096-row tile; miss rates 0 and 1 make one polarity keep everything and the other nothing, which is where a keep mask with
stray bits past the last row shows.

Not tested at size: more than 2^32 probe rows.  The keep mask, its scan and the compaction are the selection's own machinery, which
tests/test_gpu_beyond_2p32.py covers; what this operator adds in front of it handles rows in 64-bit arithmetic throughout."""
import contextlib
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import outer_join_util as oju  # noqa: E402
import semi_join_util as sju  # noqa: E402
from naive_query_engine_amd import Column, DType, Field, RecordBatch, Status  # noqa: E402

pytestmark = pytest.mark.gpu
i64 = sju.i64
BUILD_ROWS = [0, 1, 65, 4097]
PROBE_ROWS = [0, 1, 63, 64, 65, 4095, 4096, 4097, 12289]
MISS = [0.0, 0.3, 1.0]


@pytest.fixture(scope="module")
def ctx():
    from naive_query_engine_amd import capi

    c = capi.default_context()
    c.timing_enable(True)
    yield c
    c.timing_enable(False)


@contextlib.contextmanager
def env(**kv):
    """the join's environment switches are read per call"""
    saved = {k: os.environ.pop(k, None) for k in kv}
    os.environ.update({k: v for k, v in kv.items() if v is not None})
    try:
        yield
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def check_table(t, exp, what):
    got = t.to_host()
    oju.assert_same_columns(got, exp, what)
    for i, e in enumerate(exp):
        assert int(t.column_info(i).null_count) == e.null_count, f"{what} column {i}: null_count {t.column_info(i).null_count}, expected {e.null_count}"
    return got


def keys_of(cols, idx):
    return [cols[i] for i in idx]


def check_both(ctx, jt, build_keys, right, rkeys, what, null_key_unmatched=False, rt=None):
    """probe SEMI and probe ANTI of one batch against the model; together they are the batch.  Returns the uploaded probe table."""
    rt = rt if rt is not None else ctx.table_from_host(right)
    pk = keys_of(right, rkeys)
    kept = []
    for anti in (False, True):
        t = ctx.hash_join_probe_semi(jt, rt, rkeys, anti=anti, null_key_unmatched=null_key_unmatched)
        assert t.num_columns == len(right), f"{what}: every right column and nothing else"
        check_table(t, sju.probe_semi(right, pk, build_keys, anti, null_key_unmatched), f"{what} anti={anti}")
        kept.append(sju.semi_rows(build_keys, pk, anti, null_key_unmatched))
    assert sorted(kept[0] + kept[1]) == list(range(right[0].length)) and not set(kept[0]) & set(kept[1]), f"{what}: SEMI and ANTI partition the batch"
    return rt


# ----------------------------------------------------------------------------- every build form at the size edges
@pytest.mark.parametrize("n", BUILD_ROWS)
@pytest.mark.parametrize("form", list(sju.FORMS))
def test_every_build_form_at_the_word_and_tile_edges(ctx, form, n):
    make, lkey = sju.FORMS[form]
    rng = np.random.default_rng(1000 * sorted(sju.FORMS).index(form) + n)
    left = make(rng, n)
    jt = ctx.hash_join_build(ctx.table_from_host(left), lkey)
    for m in PROBE_ROWS:
        for miss in MISS:
            right = sju.probe_side(rng, left[lkey], m, miss)
            check_both(ctx, jt, left[lkey], right, [1], f"{form} n={n} m={m} miss={miss}")


def test_partitioned_build():
    from naive_query_engine_amd import capi

    rng = np.random.default_rng(17)
    n = 1 << 17
    left = sju.form_dense_bitmap(rng, n)
    c = capi.Context(0)
    try:
        c.timing_enable(True)
        with env(NQE_JOIN_PART_BUILD_MIN="65536"):
            jt = c.hash_join_build(c.table_from_host(left), 0)
        assert c.timing_query("join_build_part_scatter")[1] == 1, "the partitioned build was not taken"
        right = sju.probe_side(rng, left[0], 12289, 0.3)
        rt = check_both(c, jt, left[0], right, [1], "partitioned build")
        marks = c.join_marks(jt)
        assert c.hash_join_probe_semi(jt, rt, [1], marks=marks, want_out=False) is None
        for anti in (False, True):
            check_table(c.hash_join_marked_build(jt, marks, anti=anti), sju.take_rows(left, sju.marked_rows(left[0], [right[1]], anti)), f"partitioned build marked anti={anti}")
    finally:
        c.close()


# ----------------------------------------------------------------------------- payload columns of every kind on the probe side
def payload_probe_side(rng, build_key, m, miss=0.3):
    """[Utf8 with NULLs, Boolean with NULLs, key, Int64 with NULLs, Float64, Boolean, UInt64 row number]"""
    key = sju.probe_side(rng, build_key, m, miss)[1]
    return [oju.utf8_column([None if v % 7 == 0 else "s" * int(v % 4) + str(v) for v in range(m)]), Column.from_numpy(rng.random(m) < 0.5, rng.random(m) > 0.2), key,
            Column.from_numpy(rng.integers(-99, 99, m).astype(np.int64), rng.random(m) > 0.3), Column.from_numpy(rng.normal(0, 1, m)),
            Column.from_numpy(rng.random(m) < 0.5), Column.from_numpy(np.arange(m, dtype=np.uint64))]


@pytest.mark.parametrize("form", ["dense_full", "dense_bitmap", "sparse_check", "dup_sparse", "utf8"])
def test_utf8_boolean_and_nullable_payload_columns(ctx, form):
    make, lkey = sju.FORMS[form]
    rng = np.random.default_rng(50 + len(form))
    left = make(rng, 301)
    jt = ctx.hash_join_build(ctx.table_from_host(left), lkey)
    for m, miss in ((4097, 0.3), (65, 0.0), (64, 1.0)):
        check_both(ctx, jt, left[lkey], payload_probe_side(rng, left[lkey], m, miss), [2], f"{form} payload m={m} miss={miss}")


def test_wider_than_the_joins_column_limit(ctx):
    """the join's 32-column limit does not apply: the columns are compacted one at a time"""
    rng = np.random.default_rng(3)
    left = sju.form_dense_bitmap(rng, 65)
    jt = ctx.hash_join_build(ctx.table_from_host(left), 0)
    key = sju.probe_side(rng, left[0], 130)[1]
    right = [key] + [i64(np.arange(130) + c) for c in range(39)]
    check_both(ctx, jt, left[0], right, [0], "40 probe columns")


# ----------------------------------------------------------------------------- NULL keys match nothing (the flag)
def null_probe_keys(rng, build_key, m):
    """m probe keys with NULLs at rows 0, 63, 64 and m - 1 whose raw slots are build keys, and a third of the other rows missing"""
    bk = build_key.to_numpy()
    keys = sju.probe_side(rng, build_key, m, 0.3)[1].to_numpy().copy()
    mask = np.ones(m, dtype=bool)
    for r in sorted({0, 63, 64, m - 1}):
        if r < m:
            keys[r] = bk[r % bk.size]
            mask[r] = False
    return Column.from_numpy(keys, mask), np.nonzero(~mask)[0].tolist()


@pytest.mark.parametrize("form", ["dense_full", "dense_bitmap", "sparse_packed", "sparse_pairs", "sparse_check", "dup_dense", "dup_sparse"])
def test_null_keys_match_nothing_under_the_flag(ctx, form):
    make, lkey = sju.FORMS[form]
    rng = np.random.default_rng(90 + len(form))
    left = make(rng, 200)
    jt = ctx.hash_join_build(ctx.table_from_host(left), lkey)
    for m in (65, 130, 4097):
        key, null_rows = null_probe_keys(rng, left[lkey], m)
        right = [i64(np.arange(m)), key]
        rt = check_both(ctx, jt, left[lkey], right, [1], f"{form} m={m} NULL slots without the flag")
        check_both(ctx, jt, left[lkey], right, [1], f"{form} m={m} NULL slots with the flag", null_key_unmatched=True, rt=rt)
        plain = ctx.hash_join_probe_semi(jt, rt, [1]).to_host()[0].to_numpy().tolist()
        flagged = ctx.hash_join_probe_semi(jt, rt, [1], null_key_unmatched=True).to_host()[0].to_numpy().tolist()
        assert sorted(set(plain) - set(flagged)) == null_rows and not set(flagged) - set(plain), f"{form} m={m}: the flag changes exactly the NULL rows"
        # a NULL row sets no mark: the marks of the flagged pass are those of the batch without its NULL rows
        marks = ctx.join_marks(jt)
        ctx.hash_join_probe_semi(jt, rt, [1], null_key_unmatched=True, marks=marks, want_out=False)
        check_table(ctx.hash_join_marked_build(jt, marks), sju.take_rows(left, sju.marked_rows(left[lkey], [key], null_unmatched=True)), f"{form} m={m} marks under the flag")


def test_null_flag_on_tuples_and_the_build_side_refusal(ctx):
    rng = np.random.default_rng(7)
    n, m = 150, 130
    left = [i64(rng.integers(0, 12, n)), oju.utf8_column([f"t{v}" for v in rng.integers(0, 6, n)]), i64(np.arange(n))]
    lt = ctx.table_from_host(left)
    jt = ctx.hash_join_build_keys(lt, [0, 1])
    a = Column.from_numpy(rng.integers(0, 14, m).astype(np.int64), rng.random(m) > 0.2)
    b = oju.utf8_column([None if rng.random() < 0.2 else f"t{v}" for v in rng.integers(0, 7, m)])
    braw = [x if x else b"t1" for x in oju.utf8_raw(b)]  # bytes that are a build key under the NULLs of the second position
    b2 = oju.utf8_column(braw)
    b2.validity = b.validity
    right = [i64(np.arange(m)), a, b2]
    rt = check_both(ctx, jt, left[:2], right, [1, 2], "tuple without the flag")
    check_both(ctx, jt, left[:2], right, [1, 2], "tuple with the flag", null_key_unmatched=True, rt=rt)
    assert sju.semi_rows(left[:2], right[1:], null_unmatched=True) != sju.semi_rows(left[:2], right[1:])
    # the build side: a key column with NULLs is refused under the flag, before any launch, and serves without it
    from naive_query_engine_amd import capi

    for which, nl in ((0, [Column.from_numpy(np.array([1, 2, 3], dtype=np.int64), np.array([True, False, True])), oju.utf8_column(["a", "b", "c"])]),
                      (1, [i64([1, 2, 3]), oju.utf8_column(["a", None, "c"])])):
        nt = ctx.table_from_host(nl)
        pt = ctx.table_from_host([i64([2, 9]), oju.utf8_column(["b", "a"])])
        for jn, keys in ((ctx.hash_join_build(nt, which), [which]), (ctx.hash_join_build_keys(nt, [0, 1]), [0, 1])):
            ctx.synchronize()
            ctx.timing_reset()
            with pytest.raises(capi.ErrorCode) as e:
                ctx.hash_join_probe_semi(jn, pt, keys, null_key_unmatched=True)
            assert e.value.status == Status.NotSupported and ctx.timing_query("")[1] == 0
            assert ctx.hash_join_probe_semi(jn, pt, keys).num_rows >= 0  # the context is usable, and without the flag the table serves


# ----------------------------------------------------------------------------- marks
@pytest.mark.parametrize("form", list(sju.FORMS))
def test_mark_only_passes_then_the_marked_build_rows(ctx, form):
    make, lkey = sju.FORMS[form]
    rng = np.random.default_rng(200 + sorted(sju.FORMS).index(form))
    for n in (301, 65, 0):
        left = make(rng, n)
        lt = ctx.table_from_host(left)
        jt = ctx.hash_join_build(lt, lkey)
        head = sju.slice_columns(left, min(n, 100))
        batches = [sju.probe_side(rng, head[lkey], 5000), sju.probe_side(rng, head[lkey], 1025, miss=0.6), sju.probe_side(rng, left[lkey], 64, miss=0.9)]
        marks, outer_marks = ctx.join_marks(jt), ctx.join_marks(jt)
        for right in batches:
            rt = ctx.table_from_host(right)
            ctx.synchronize()
            ctx.timing_reset()
            assert ctx.hash_join_probe_semi(jt, rt, [1], marks=marks, want_out=False) is None
            assert ctx.timing_query("join_semi_keep")[1] == 1 and ctx.timing_query("compact")[1] == 0 and ctx.timing_query("scan")[1] == 0, "the mark-only pass keeps and compacts nothing"
            ctx.hash_join_probe_outer(jt, rt, 1, marks=outer_marks)
        pks = [b[1] for b in batches]
        for anti in (False, True):
            t = ctx.hash_join_marked_build(jt, marks, anti=anti)
            assert t.num_columns == len(left), "the left columns only"
            check_table(t, sju.take_rows(left, sju.marked_rows(left[lkey], pks, anti)), f"{form} n={n} marked anti={anti}")
        # build ANTI is the outer join's tail, from the semi probe's marks and from the outer probe's
        tail = ctx.hash_join_unmatched_build(jt, outer_marks, [DType.INT64, DType.UTF8]).to_host()[:len(left)]
        for mk in (marks, outer_marks):
            oju.assert_same_columns(ctx.hash_join_marked_build(jt, mk, anti=True).to_host(), tail, f"{form} n={n} build ANTI vs unmatched_build")
        # fresh marks: nothing matched
        fresh = ctx.join_marks(jt)
        assert ctx.hash_join_marked_build(jt, fresh).num_rows == 0 and ctx.hash_join_marked_build(jt, fresh, anti=True).num_rows == n


@pytest.mark.parametrize("form", ["dense_full", "dense_bitmap", "sparse_packed", "dup_dense", "utf8"])
def test_marks_and_an_output_in_one_call(ctx, form):
    make, lkey = sju.FORMS[form]
    rng = np.random.default_rng(300 + len(form))
    left = make(rng, 301)
    jt = ctx.hash_join_build(ctx.table_from_host(left), lkey)
    head = sju.slice_columns(left, 120)
    batches = [sju.probe_side(rng, head[lkey], 4097), sju.probe_side(rng, head[lkey], 65, miss=0.5)]
    marks = ctx.join_marks(jt)
    for bi, right in enumerate(batches):
        rt = ctx.table_from_host(right)
        anti = bi == 1
        t = ctx.hash_join_probe_semi(jt, rt, [1], anti=anti, marks=marks)
        check_table(t, sju.probe_semi(right, right[1], left[lkey], anti), f"{form} output with marks, batch {bi}")
    for anti in (False, True):
        check_table(ctx.hash_join_marked_build(jt, marks, anti=anti), sju.take_rows(left, sju.marked_rows(left[lkey], [b[1] for b in batches], anti)), f"{form} marked anti={anti}")


# ----------------------------------------------------------------------------- several keys
def tuple_tables(rng, n, m, utf8):
    """build [a, b, payload] and probe [row number, a, b]: duplicates on both sides, misses at either position"""
    la, ra = rng.integers(-5, 20, n), rng.integers(-5, 24, m)
    lb, rb = rng.integers(0, 6, n), rng.integers(0, 7, m)
    mk = (lambda v: oju.utf8_column([f"b{x}" for x in v])) if utf8 else i64
    return [i64(la), mk(lb), i64(np.arange(n) * 2)], [i64(np.arange(m)), i64(ra), mk(rb)]


@pytest.mark.parametrize("kind", ["packed", "forced_dict", "int_utf8"])
def test_several_keys(ctx, kind):
    rng = np.random.default_rng(400 + len(kind))
    with env(NQE_JOIN_KEYS_FORCE_DICT="1" if kind == "forced_dict" else None):
        for n, m in ((300, 4097), (65, 64), (0, 65), (1, 1)):
            left, right = tuple_tables(rng, n, m, kind == "int_utf8")
            if kind != "int_utf8" and m > 3:  # probe tuples outside the build's ranges, at either position and both
                right[1].values[:3] = [1 << 40, 3, -(1 << 50)]
                right[2].values[:3] = [2, 1 << 45, 1 << 61]
            lt = ctx.table_from_host(left)
            jt = ctx.hash_join_build_keys(lt, [0, 1])
            rt = check_both(ctx, jt, left[:2], right, [1, 2], f"{kind} n={n} m={m}")
            marks = ctx.join_marks(jt)
            ctx.hash_join_probe_semi(jt, rt, [1, 2], marks=marks, want_out=False)
            for anti in (False, True):
                t = ctx.hash_join_marked_build(jt, marks, anti=anti)
                assert t.num_columns == len(left), "never the hidden code column"
                check_table(t, sju.take_rows(left, sju.marked_rows(left[:2], [right[1:]], anti)), f"{kind} n={n} m={m} marked anti={anti}")
            tail = ctx.hash_join_unmatched_build(jt, marks, []).to_host()
            oju.assert_same_columns(ctx.hash_join_marked_build(jt, marks, anti=True).to_host(), tail, f"{kind} n={n} m={m} build ANTI vs unmatched_build")


# ----------------------------------------------------------------------------- the library against itself
@pytest.mark.parametrize("form", list(sju.FORMS))
def test_semi_rows_are_the_distinct_probe_rows_of_the_inner_join(ctx, form):
    make, lkey = sju.FORMS[form]
    rng = np.random.default_rng(500 + sorted(sju.FORMS).index(form))
    left = make(rng, 4097)
    jt = ctx.hash_join_build(ctx.table_from_host(left), lkey)
    for m in (12289, 65):
        right = sju.probe_side(rng, left[lkey], m)  # column 0: the row number * 3
        rt = ctx.table_from_host(right)
        inner = ctx.hash_join_probe_keys(jt, rt, [1]).to_host()[len(left)].to_numpy()
        semi = ctx.hash_join_probe_semi(jt, rt, [1]).to_host()[0].to_numpy()
        anti = ctx.hash_join_probe_semi(jt, rt, [1], anti=True).to_host()[0].to_numpy()
        assert (semi == np.unique(inner)).all() and semi.size == np.unique(inner).size, f"{form} m={m}"
        assert (np.sort(np.concatenate([semi, anti])) == np.arange(m) * 3).all() and (np.diff(anti) > 0).all(), f"{form} m={m}: ANTI is the rest, in probe order"


# ----------------------------------------------------------------------------- dispatch
def launches(ctx):
    return {name: cnt for name, (_, cnt) in ctx.timing_report().items()}


@pytest.mark.parametrize("form,label,marking", [("dense_full", "join_semi_keep_range", "join_semi_keep_lookup"), ("dense_bitmap", "join_semi_keep_bitmap", "join_semi_keep_lookup"),
                                                ("dup_dense", "join_semi_keep_lookup", "join_semi_keep_lookup"), ("utf8", "join_semi_keep_lookup", "join_semi_keep_lookup"),
                                                ("sparse_packed", "join_semi_keep_packed", "join_semi_keep_coop"), ("sparse_pairs", "join_semi_keep_pairs", "join_semi_keep_coop"),
                                                ("sparse_check", "join_semi_keep_coop", "join_semi_keep_coop"), ("dup_sparse", "join_semi_keep_coop", "join_semi_keep_coop")])
def test_each_build_form_takes_its_existence_form(ctx, form, label, marking):
    """the label suffix names the form: RANGE / BITMAP / LOOKUP over dense tables, and over hashed tables the wave-cooperative reads of the
    packed words, the 16-byte pairs or the {key, meta} slots; a pass that marks needs the start of the match (LOOKUP or the slots).
    NQE_SEMI_NO_COOP=1 sends a hashed table through LOOKUP, with the same rows"""
    make, lkey = sju.FORMS[form]
    rng = np.random.default_rng(600)
    left = make(rng, 301)
    jt = ctx.hash_join_build(ctx.table_from_host(left), lkey)
    right = sju.probe_side(rng, left[lkey], 4097)
    rt = ctx.table_from_host(right)
    marks = ctx.join_marks(jt)
    for anti in (False, True):
        ctx.synchronize()
        ctx.timing_reset()
        ctx.hash_join_probe_semi(jt, rt, [1], anti=anti)
        got = launches(ctx)
        assert got.get(label) == 1 and sum(c for k, c in got.items() if k.startswith("join_semi_keep")) == 1, got
        assert not [k for k in got if k.startswith("join_outer_") or k.startswith("join_probe_") or k.startswith("join_fused")], got
        ctx.timing_reset()
        ctx.hash_join_probe_semi(jt, rt, [1], anti=anti, marks=marks)
        got = launches(ctx)
        assert got.get(marking) == 1 and sum(c for k, c in got.items() if k.startswith("join_semi_keep")) == 1, got
        with env(NQE_SEMI_NO_COOP="1"):
            ctx.timing_reset()
            t = ctx.hash_join_probe_semi(jt, rt, [1], anti=anti)
            got = launches(ctx)
            assert sum(c for k, c in got.items() if k.startswith("join_semi_keep")) == 1 and (got.get("join_semi_keep_lookup") == 1 or label in got), got
            check_table(t, sju.probe_semi(right, right[1], left[lkey], anti), f"{form} anti={anti} without the cooperative read")
    ctx.timing_reset()
    ctx.hash_join_marked_build(jt, marks)
    got = launches(ctx)
    assert got.get("join_semi_marked") == 1 and not [k for k in got if k.startswith("join_outer_")], got


# ----------------------------------------------------------------------------- errors
def _status(ctx, fn, *args, out=True):
    from naive_query_engine_amd import capi

    h = C.c_void_p()
    st = fn(ctx.handle, *args, C.byref(h) if out else None)
    if st == 0 and h.value:
        capi.Table(ctx, h)  # released by its destructor
    return st


def test_errors_are_decided_before_any_launch_and_leave_the_context_usable(ctx):
    from naive_query_engine_amd import capi

    L = capi.lib()
    ks = lambda *a: (C.c_int32 * max(1, len(a)))(*a)  # noqa: E731
    f64 = lambda a: Column.from_numpy(np.asarray(a, dtype=np.float64))  # noqa: E731
    u64 = lambda a: Column.from_numpy(np.asarray(a, dtype=np.uint64))  # noqa: E731
    lt = ctx.table_from_host([i64([1, 2, 3]), i64([4, 5, 6]), f64([1, 2, 3]), u64([1, 2, 3]), oju.utf8_column(["a", "b", "c"])])
    rt = ctx.table_from_host([i64([1, 2]), i64([4, 5]), f64([1, 2]), u64([1, 2]), oju.utf8_column(["a", "b"])])
    jt2, jt1 = ctx.hash_join_build_keys(lt, [0, 1]), ctx.hash_join_build(lt, 0)
    other = ctx.hash_join_build_keys(lt, [1, 0])
    marks_other, marks1 = ctx.join_marks(other), ctx.join_marks(jt1)
    ctx.synchronize()
    ctx.timing_reset()
    S, M = L.nqe_hash_join_probe_semi, L.nqe_hash_join_marked_build
    # NULL arguments; neither an output nor marks
    assert S(None, jt1.handle, rt.handle, ks(0), 1, 0, None, C.byref(C.c_void_p())) == Status.InvalidArgument
    assert _status(ctx, S, None, rt.handle, ks(0), 1, 0, None) == Status.InvalidArgument and _status(ctx, S, jt1.handle, None, ks(0), 1, 0, None) == Status.InvalidArgument
    assert _status(ctx, S, jt1.handle, rt.handle, None, 1, 0, None) == Status.InvalidArgument
    assert _status(ctx, S, jt1.handle, rt.handle, ks(0), 1, 0, None, out=False) == Status.InvalidArgument
    # key counts
    assert _status(ctx, S, jt2.handle, rt.handle, ks(0, 1), 0, 0, None) == Status.PlanError and _status(ctx, S, jt1.handle, rt.handle, ks(0), -1, 0, None) == Status.PlanError
    assert _status(ctx, S, jt2.handle, rt.handle, ks(*[0] * 9), 9, 0, None) == Status.NotSupported
    # num_keys against the build's, unknown flag bits, foreign marks
    assert _status(ctx, S, jt2.handle, rt.handle, ks(0), 1, 0, None) == Status.InvalidArgument and _status(ctx, S, jt1.handle, rt.handle, ks(0, 1), 2, 0, None) == Status.InvalidArgument
    assert _status(ctx, S, jt2.handle, rt.handle, ks(0, 1, 1), 3, 0, None) == Status.InvalidArgument
    assert _status(ctx, S, jt1.handle, rt.handle, ks(0), 1, 4, None) == Status.InvalidArgument and _status(ctx, S, jt2.handle, rt.handle, ks(0, 1), 2, 0x80000000, None) == Status.InvalidArgument
    assert _status(ctx, S, jt2.handle, rt.handle, ks(0, 1), 2, 0, marks_other.handle) == Status.InvalidArgument
    assert _status(ctx, S, jt2.handle, rt.handle, ks(0, 1), 2, 0, marks1.handle, out=False) == Status.InvalidArgument
    # the count comes before the key indices, the flags before them too
    assert _status(ctx, S, jt2.handle, rt.handle, ks(9), 1, 0, None) == Status.InvalidArgument and _status(ctx, S, jt1.handle, rt.handle, ks(9), 1, 4, None) == Status.InvalidArgument
    # a key index out of range, in any position
    for bad in (ks(5, 0), ks(0, 5), ks(0, -1)):
        assert _status(ctx, S, jt2.handle, rt.handle, bad, 2, 0, None) == Status.LogicalError
    assert _status(ctx, S, jt1.handle, rt.handle, ks(5), 1, 1, None) == Status.LogicalError and _status(ctx, S, jt1.handle, rt.handle, ks(-1), 1, 0, marks1.handle, out=False) == Status.LogicalError
    # key types: check_key_types' errors for the first offending pair, in pair order; an index error in a later pair comes first
    assert _status(ctx, S, jt2.handle, rt.handle, ks(0, 2), 2, 0, None) == Status.NotImplemented  # a Float64 probe key
    assert _status(ctx, S, jt2.handle, rt.handle, ks(0, 3), 2, 0, None) == Status.NotSupported  # Int64 against UInt64
    assert _status(ctx, S, jt2.handle, rt.handle, ks(4, 2), 2, 0, None) == Status.NotSupported  # the first pair decides (Int64 against Utf8)
    assert _status(ctx, S, jt1.handle, rt.handle, ks(2), 1, 0, None) == Status.NotImplemented and _status(ctx, S, jt1.handle, rt.handle, ks(4), 1, 1, None) == Status.NotSupported
    assert _status(ctx, S, jt2.handle, rt.handle, ks(2, 9), 2, 0, None) == Status.LogicalError
    # nqe_hash_join_marked_build
    assert _status(ctx, M, jt1.handle, None, 0) == Status.InvalidArgument and _status(ctx, M, None, marks1.handle, 0) == Status.InvalidArgument
    assert _status(ctx, M, jt1.handle, marks1.handle, 0, out=False) == Status.InvalidArgument
    assert _status(ctx, M, jt1.handle, marks1.handle, 2) == Status.InvalidArgument and _status(ctx, M, jt1.handle, marks1.handle, 3) == Status.InvalidArgument
    assert _status(ctx, M, jt2.handle, marks_other.handle, 0) == Status.InvalidArgument and _status(ctx, M, jt1.handle, marks_other.handle, 1) == Status.InvalidArgument
    assert ctx.timing_query("")[1] == 0, "a refused call launched a kernel"
    # the context is usable, and nothing above marked anything
    assert ctx.hash_join_probe_semi(jt2, rt, [0, 1]).num_rows == 2 and ctx.hash_join_probe_semi(jt1, rt, [0], anti=True).num_rows == 0
    assert ctx.hash_join_marked_build(jt1, marks1).num_rows == 0 and ctx.hash_join_marked_build(other, marks_other, anti=True).num_rows == 3
    with pytest.raises(capi.ErrorCode) as e:
        ctx.hash_join_probe_semi(jt1, rt, [0], flags=8)
    assert e.value.status == Status.InvalidArgument


# ----------------------------------------------------------------------------- mirror
def test_python_mirror_in_all_four_forms(ctx):
    from naive_query_engine_amd import physical_plan as pp

    rng = np.random.default_rng(800)
    n, m = 200, 500
    left = [i64(rng.integers(0, 30, n)), oju.utf8_column([f"s{v}" for v in rng.integers(0, 4, n)]), i64(np.arange(n))]
    right = [i64(np.arange(m)), oju.utf8_column([f"s{v}" for v in rng.integers(0, 5, m)]), Column.from_numpy(rng.integers(0, 40, m).astype(np.int64), rng.random(m) > 0.1)]
    lf = [Field("k", DType.INT64), Field("s", DType.UTF8), Field("lrow", DType.INT64)]
    rf = [Field("rrow", DType.INT64), Field("t", DType.UTF8), Field("fk", DType.INT64)]
    cut = 300
    lsrc = pp.MemTable.try_create(lf, [RecordBatch(lf, left)])
    rsrc = pp.MemTable.try_create(rf, [RecordBatch(rf, oju.take_null(right, np.arange(0, cut))), RecordBatch(rf, oju.take_null(right, np.arange(cut, m)))])
    rbatches = [oju.take_null(right, np.arange(0, cut)), oju.take_null(right, np.arange(cut, m))]
    T = pp.SemiJoinType
    for on, lks, rks in (([("k", "fk")], [0], [2]), ([("k", "fk"), ("s", "t")], [0, 1], [2, 1])):
        pairs = [(pp.ColumnRef(None, a), pp.ColumnRef(None, b)) for a, b in on]
        for nku in (False, True):
            for st in (T.ProbeSemi, T.ProbeAnti, T.BuildSemi, T.BuildAnti):
                probe = st in (T.ProbeSemi, T.ProbeAnti)
                anti = st in (T.ProbeAnti, T.BuildAnti)
                plan = pp.HashSemiJoin.create(pp.ScanPlan.create(lsrc, None), pp.ScanPlan.create(rsrc, None), pairs, st, rf if probe else lf, null_key_unmatched=nku)
                out = plan.execute()
                what = f"on={on} type={st} null_key_unmatched={nku}"
                if probe:
                    assert len(out) == 2 and [f.name for f in out[0].fields] == ["rrow", "t", "fk"], what
                    for b, rb in zip(out, rbatches):
                        check_table(b.table, sju.probe_semi(rb, keys_of(rb, rks), keys_of(left, lks), anti, nku), what)
                else:
                    assert len(out) == 1 and [f.name for f in out[0].fields] == ["k", "s", "lrow"], what
                    check_table(out[0].table, sju.take_rows(left, sju.marked_rows(keys_of(left, lks), [keys_of(rb, rks) for rb in rbatches], anti, nku)), what)


# ----------------------------------------------------------------------------- fuzz
@pytest.mark.parametrize("seed", range(20))
def test_fuzz(ctx, seed):
    rng = np.random.default_rng(9000 + seed)
    form = list(sju.FORMS)[int(rng.integers(0, len(sju.FORMS)))]
    make, lkey = sju.FORMS[form]
    n = int(rng.choice([0, 1, 2, 63, 64, 65, 300, 4096, 4097, 9000]))
    left = make(rng, n)
    jt = ctx.hash_join_build(ctx.table_from_host(left), lkey)
    marks = ctx.join_marks(jt)
    seen = []
    for _ in range(3):
        m = int(rng.choice([0, 1, 63, 64, 65, 127, 128, 4095, 4096, 4097, 8191, 8193]))
        miss = float(rng.choice([0.0, 0.1, 0.5, 1.0]))
        right = sju.probe_side(rng, left[lkey], m, miss)
        nku = bool(rng.integers(0, 2)) and right[1].dtype != DType.UTF8
        if nku and m:  # NULLs over real slots
            right[1] = Column.from_numpy(right[1].to_numpy(), rng.random(m) > 0.2)
        anti, with_marks, want_out = bool(rng.integers(0, 2)), bool(rng.integers(0, 2)), bool(rng.integers(0, 3))
        what = f"seed {seed} {form} n={n} m={m} miss={miss} anti={anti} nku={nku} marks={with_marks} out={want_out}"
        rt = ctx.table_from_host(right)
        if want_out or not with_marks:
            t = ctx.hash_join_probe_semi(jt, rt, [1], anti=anti, null_key_unmatched=nku, marks=marks if with_marks else None)
            check_table(t, sju.probe_semi(right, right[1], left[lkey], anti, nku), what)
        else:
            ctx.hash_join_probe_semi(jt, rt, [1], anti=anti, null_key_unmatched=nku, marks=marks, want_out=False)
        if with_marks:
            seen.append((right[1], nku))
    mask = np.zeros(n, dtype=bool)
    for pk, nku in seen:
        mask |= sju.marked_mask(left[lkey], [pk], nku)
    for anti in (False, True):
        check_table(ctx.hash_join_marked_build(jt, marks, anti=anti), sju.take_rows(left, np.nonzero(~mask if anti else mask)[0]), f"seed {seed} {form} n={n} marked anti={anti}")
