"""GPU: an NQE_EXPR_STRING_MATCH node (quirk Q27: like, not_like, ilike, not_ilike, starts_with, ends_with, contains, strpos) through
nqe_expr_evaluate, every operator that takes expression trees, and the Python plan mirror — against the plain-Python model of
tests/string_match_util.py.  Every comparison is bit for bit: the packed value bits including the zero tail of the last byte and the 0
under a NULL (for the NOT forms too), the Int64 values including the 0 under a NULL, the validity bits and null_count."""
from collections import Counter

import numpy as np
import pytest

from tests.helpers import fields
from tests.string_match_util import (BIG_CASES, BIG_STRINGS, VERBATIM_ESCAPES, WORD_SIZES, WORD_STRINGS, long_group_cases, long_group_strings, wide_group_strings, word_cases, CONTAINS, ENDS_WITH, ESCAPE_PATTERNS, ESCAPE_STRINGS, GROUP_CASES, GROUPS, ILIKE, ILIKE_PATTERNS, ILIKE_STRINGS, LIKE, NOT_ILIKE, NOT_LIKE,
                                     ONE_PATTERNS, ONE_STRINGS, ROW_CASES, ROW_COUNTS, ROW_POOL, STARTS_WITH, STRPOS, all_strings, exhaustive_cases, group_strings, model, model_rows,
                                     utf8_column)

pytestmark = pytest.mark.gpu

F = fields("s")
MEAN_RANGE = {4: (0, 32), 8: (33, 96), 16: (97, 256), 32: (257, 1024), 64: (1025, 1 << 40)}  # the mean length (bytes // rows) that picks each lane group


@pytest.fixture(scope="module")
def ctx():
    from naive_query_engine_amd import capi

    c = capi.Context(0)
    yield c
    c.close()


def ex():
    from naive_query_engine_amd import expression

    return expression


def col(i):
    return ex().col(i)


def match(op, e, pattern):
    from naive_query_engine_amd import MatchOperator, PhysicalStringMatchExpr

    lit = pattern if isinstance(pattern, ex().PhysicalExpr) else ex().lit_utf8(pattern)
    return PhysicalStringMatchExpr.create(MatchOperator(op), e, lit)


def for_group(items, group):
    """`items` plus rows that bring the column's mean length into the range that gives every string `group` lanes (the device of
    test_gpu_string_args.py)"""
    items = list(items)
    lo, hi = MEAN_RANGE[group]
    mean = lambda: sum(len(s) for s in items) // len(items)
    while mean() > hi:
        items.append(b"")
    while mean() < lo:
        items.append(b"q" * (2 * lo + 8))
    assert lo <= mean() <= hi
    return items


def assert_result(out, op, values, valid, nullable, what=""):
    """`out`: the 1-column result table; values / valid: the model's rows; nullable: whether a validity buffer is expected at all"""
    from naive_query_engine_amd import DType
    from naive_query_engine_amd.arrow_host import pack_bits

    got = out.to_host()[0]
    n = len(values)
    valid = np.asarray(valid, dtype=bool) if n else np.zeros(0, dtype=bool)
    info = out.column_info(0)
    if op == STRPOS:
        assert got.dtype == DType.INT64 and got.length == n, (what, got.dtype, got.length)
        exp = np.asarray(values, dtype=np.int64) if n else np.zeros(0, dtype=np.int64)
        if not (got.to_numpy() == exp).all():
            bad = np.flatnonzero(got.to_numpy() != exp)
            raise AssertionError((what, bad[:8].tolist(), got.to_numpy()[bad[:8]].tolist(), exp[bad[:8]].tolist()))
    else:
        assert got.dtype == DType.BOOLEAN and got.length == n, (what, got.dtype, got.length)
        exp = np.asarray(values, dtype=bool) if n else np.zeros(0, dtype=bool)
        bits = np.asarray(got.values, dtype=np.uint8)[: (n + 7) // 8]
        if not (bits == pack_bits(exp)[: (n + 7) // 8]).all():  # the packed bytes: the zero tail and the zeros under NULLs included
            bad = np.flatnonzero(got.to_numpy() != exp)
            raise AssertionError((what, "value bits", bad[:8].tolist(), bits[-1]))
    assert (got.valid_mask() == valid).all(), (what, "validity")
    if n:  # (a column of no rows may carry a validity buffer of no bytes or none)
        assert bool(info.validity) == bool(nullable), (what, "validity buffer", nullable)
    assert info.null_count == int((~valid).sum()), (what, "null_count", info.null_count)


def check(ctx, t, items, op, pattern, mask=None, what="", values=None):
    if values is None:
        values, valid = model_rows(op, items, pattern, mask)
    else:
        valid = [True] * len(items) if mask is None else list(mask)
    out = ctx.expr_evaluate(t, match(op, col(0), pattern).flatten(F))
    assert_result(out, op, values, valid, (mask is not None and not all(mask)) or pattern is None, f"{what} op {op} {pattern!r:.60}")
    return out


# ----------------------------------------------------------------------------- shapes
@pytest.mark.parametrize("n", ROW_COUNTS)
def test_every_row_count_with_and_without_nulls(ctx, n):
    """a wave owns 64 rows and stores their value word: the word's last row, its neighbours' first, and the zero bits behind row n"""
    items = [ROW_POOL[(i * 7 + i // 64) % len(ROW_POOL)] for i in range(n)]
    mask = [(i * 5) % 7 != 0 for i in range(n)]
    plain, nullable = ctx.table_from_host([utf8_column(items)]), ctx.table_from_host([utf8_column(items, mask)])
    for op, p in ROW_CASES + [(LIKE, b"%"), (NOT_LIKE, b"%"), (CONTAINS, b""), (STRPOS, b"")]:
        check(ctx, plain, items, op, p, what=f"{n} rows")
        check(ctx, nullable, items, op, p, mask=mask, what=f"{n} rows, NULLs")
    # a NULL literal: every row NULL, every value 0, null_count = n
    for op in (LIKE, NOT_LIKE, NOT_ILIKE, ENDS_WITH, STRPOS):
        check(ctx, plain, items, op, None, what=f"{n} rows, NULL literal")
        check(ctx, nullable, items, op, None, mask=mask, what=f"{n} rows, NULL literal over NULLs")


@pytest.mark.parametrize("group", GROUPS)
def test_every_lane_group(ctx, group):
    """strings of 0, 1, G-1, G, G+1, 2G, 2G+1 bytes with the match in chunk 0, across the first chunk edge, in the last partial chunk or
    absent, in a column whose mean length gives every string `group` lanes"""
    items = for_group(group_strings(group), group)
    mask = [i % 5 != 2 for i in range(len(items))]
    plain, nullable = ctx.table_from_host([utf8_column(items)]), ctx.table_from_host([utf8_column(items, mask)])
    for op, p in GROUP_CASES:
        check(ctx, plain, items, op, p, what=f"{group} lanes")
        check(ctx, nullable, items, op, p, mask=mask, what=f"{group} lanes, NULLs")
    # a long literal and a long ONE segment across several chunks of G positions (the one-position-per-lane walk)
    long_items = for_group(long_group_strings(group), group)
    t = ctx.table_from_host([utf8_column(long_items)])
    for op, p in long_group_cases(group):
        check(ctx, t, long_items, op, p, what=f"{group} lanes, long")


@pytest.mark.parametrize("group", GROUPS)
def test_every_lane_group_past_the_first_chunk_of_the_word_walk(ctx, group):
    """a segment of at most 8 literal bytes is searched 8 positions per lane, a chunk is 8G positions: strings of 8G-1, 8G, 8G+1, 16G and
    16G+1 bytes with the match wholly in chunk 0, across the edge at 8G, behind it, in the last partial chunk or absent — strpos with
    two-byte characters in front of a match in a later chunk"""
    items = for_group(wide_group_strings(group), group)
    mask = [i % 5 != 2 for i in range(len(items))]
    plain, nullable = ctx.table_from_host([utf8_column(items)]), ctx.table_from_host([utf8_column(items, mask)])
    for op, p in GROUP_CASES:
        check(ctx, plain, items, op, p, what=f"{group} lanes, wide")
        check(ctx, nullable, items, op, p, mask=mask, what=f"{group} lanes, wide, NULLs")


def test_exhaustive_slice(ctx):
    """every string of up to 5 symbols of the six-symbol alphabet (9331 rows), a pattern of every form, one nqe_expr_evaluate each"""
    items = all_strings(5)
    mask = [(i * 11) % 13 != 0 for i in range(len(items))]
    plain, nullable = ctx.table_from_host([utf8_column(items)]), ctx.table_from_host([utf8_column(items, mask)])
    likes = {}
    for k, (op, p) in enumerate(exhaustive_cases()):
        if op in (LIKE, NOT_LIKE):  # one model pass serves both
            if p not in likes:
                likes[p] = [model(LIKE, s, p) for s in items]
            values = likes[p] if op == LIKE else [not v for v in likes[p]]
        else:
            values = [model(op, s, p) for s in items]
        if k % 4 == 0:
            zero = 0 if op == STRPOS else False
            check(ctx, nullable, items, op, p, mask=mask, what="exhaustive, NULLs", values=[v if ok else zero for v, ok in zip(values, mask)])
        else:
            check(ctx, plain, items, op, p, what="exhaustive", values=values)


def test_one_against_multi_byte_and_broken_characters(ctx):
    t = ctx.table_from_host([utf8_column(ONE_STRINGS)])
    for p in ONE_PATTERNS:
        check(ctx, t, ONE_STRINGS, LIKE, p, what="one")
        check(ctx, t, ONE_STRINGS, NOT_LIKE, p, what="one")
    # the cases of the specification, spelled out
    got = lambda p: ctx.expr_evaluate(t, match(LIKE, col(0), p).flatten(F)).to_host()[0].to_numpy().tolist()
    by = dict(zip(ONE_STRINGS, got(b"_")))
    assert by["é".encode()] and by["😀".encode()] and by[b"\xa9\xa9a"] and by[b"\xa9" * 5] and by[b"\xc3"] and not by[b"a\xc3"] and not by[b""] and not by["éx".encode()]


def test_ilike_folds_a_to_z_only(ctx):
    mask = [i % 4 != 1 for i in range(len(ILIKE_STRINGS))]
    plain, nullable = ctx.table_from_host([utf8_column(ILIKE_STRINGS)]), ctx.table_from_host([utf8_column(ILIKE_STRINGS, mask)])
    for p in ILIKE_PATTERNS:
        for op in (ILIKE, NOT_ILIKE, LIKE):
            check(ctx, plain, ILIKE_STRINGS, op, p, what="ilike")
        check(ctx, nullable, ILIKE_STRINGS, NOT_ILIKE, p, mask=mask, what="not ilike under NULLs")  # 0 under a NULL
        check(ctx, nullable, ILIKE_STRINGS, NOT_LIKE, p, mask=mask, what="not like under NULLs")
    got = ctx.expr_evaluate(plain, match(ILIKE, col(0), "é".encode()).flatten(F)).to_host()[0].to_numpy().tolist()
    assert dict(zip(ILIKE_STRINGS, got))["é".encode()] and not dict(zip(ILIKE_STRINGS, got))["É".encode()]


def test_escapes_and_verbatim_literals(ctx):
    t = ctx.table_from_host([utf8_column(ESCAPE_STRINGS)])
    for p in ESCAPE_PATTERNS:
        check(ctx, t, ESCAPE_STRINGS, LIKE, p, what="escapes")
    for p in VERBATIM_ESCAPES:  # no wildcards and no escape in the verbatim operators
        for op in (STARTS_WITH, ENDS_WITH, CONTAINS, STRPOS):
            check(ctx, t, ESCAPE_STRINGS, op, p, what="verbatim")


def test_long_literals_on_both_sides_of_the_word_compare(ctx):
    """prefixes and suffixes of 1-24 bytes: at most 8 bytes are one masked word from the kernel's arguments, longer ones are read 8 at a time"""
    items = WORD_STRINGS
    mask = [i % 6 != 3 for i in range(len(items))]
    plain, nullable = ctx.table_from_host([utf8_column(items)]), ctx.table_from_host([utf8_column(items, mask)])
    for k in WORD_SIZES:
        for op, p in word_cases(k):
            check(ctx, plain, items, op, p, what=f"{k} bytes")
            check(ctx, nullable, items, op, p, mask=mask, what=f"{k} bytes, NULLs")
    t = ctx.table_from_host([utf8_column(BIG_STRINGS)])
    for op, p in BIG_CASES:
        check(ctx, t, BIG_STRINGS, op, p, what="4096 bytes")


# ----------------------------------------------------------------------------- equivalences with what exists
def test_equivalences_with_compare_substr_and_strpos(ctx):
    from naive_query_engine_amd import Operator

    e = ex()
    rng = np.random.default_rng(3)
    pool = [b"abc", b"ab", b"abcd", b"", b"xab", b"a-b", b"-", b"ab-", "é-x".encode(), b"x", b"xx-x-", b"abx", b"\xa9-q"]
    items = [pool[int(i)] for i in rng.integers(0, len(pool), 300)]
    mask = (rng.random(300) > 0.2).tolist()
    for m in (None, mask):
        t = ctx.table_from_host([utf8_column(items, m)])
        host = lambda expr: ctx.expr_evaluate(t, expr.flatten(F)).to_host()[0]
        same = lambda a, b: (a.values[: (300 + 7) // 8] == b.values[: (300 + 7) // 8]).all() and (a.valid_mask() == b.valid_mask()).all()
        assert same(host(e.like(col(0), "abc")), host(e.binop(col(0), Operator.Eq, e.lit_utf8("abc"))))
        assert same(host(e.starts_with(col(0), "ab")), host(e.binop(e.substr(col(0), 1, 2), Operator.Eq, e.lit_utf8("ab"))))
        assert same(host(e.like(col(0), "ab%")), host(e.starts_with(col(0), "ab")))
        assert same(host(e.binop(e.strpos(col(0), "x"), Operator.Gt, e.lit_i64(0))), host(e.contains(col(0), "x")))
        assert host(e.contains(col(0), "x")).to_numpy().any() and not host(e.contains(col(0), "x")).to_numpy().all()
        # substr(s, strpos(s, '-') + 1): what lies behind the first '-' (the whole string when there is none: strpos 0, start 1)
        after = host(e.substr(col(0), e.binop(e.strpos(col(0), "-"), Operator.Plus, e.lit_i64(1))))
        from tests.string_fn_util import byte_strings

        ok = [True] * 300 if m is None else m
        assert byte_strings(after) == [(s.split(b"-", 1)[1] if b"-" in s else s) if v else b"" for s, v in zip(items, ok)]


def test_the_operand_as_a_node_and_as_a_literal(ctx):
    from naive_query_engine_amd import UnaryOperator
    from tests.string_fn_util import model_lower

    e = ex()
    items = [b"ABc", b"abC", b"xAB", b" ab", b"", b"Ab-Ab", b"aB"] * 20
    mask = [i % 3 != 0 for i in range(len(items))]
    t = ctx.table_from_host([utf8_column(items, mask)])
    lower = [model_lower(s) for s in items]
    out = ctx.expr_evaluate(t, e.like(e.strop(UnaryOperator.Lower, col(0)), "ab%").flatten(F))
    assert_result(out, LIKE, *model_rows(LIKE, lower, b"ab%", mask), True, "like(lower(s), 'ab%')")
    out = ctx.expr_evaluate(t, e.strpos(e.replace(col(0), "-", "--"), "-A").flatten(F))
    assert_result(out, STRPOS, *model_rows(STRPOS, [s.replace(b"-", b"--") for s in items], b"-A", mask), True, "strpos(replace(s))")
    out = ctx.expr_evaluate(t, e.ends_with(e.substr(col(0), 1, 2), "b").flatten(F))
    assert_result(out, ENDS_WITH, *model_rows(ENDS_WITH, [s[:2] for s in items], b"b", mask), True, "ends_with(substr(s))")
    # a literal `s` is expanded to the table's rows; a NULL literal `s` is all NULL
    n = len(items)
    for op, s, p in ((LIKE, b"abc", b"a_c"), (LIKE, b"abc", b"b%"), (STRPOS, "éab".encode(), b"b"), (CONTAINS, b"", b"")):
        out = ctx.expr_evaluate(t, match(op, e.lit_utf8(s), p).flatten(F))
        assert_result(out, op, [model(op, s, p)] * n, [True] * n, False, "literal s")
    out = ctx.expr_evaluate(t, match(LIKE, e.lit_utf8(None), b"a").flatten(F))
    assert_result(out, LIKE, [False] * n, [False] * n, True, "NULL literal s")


# ----------------------------------------------------------------------------- launches
def launches(ctx, run):
    ctx.timing_enable(True)
    ctx.timing_reset()
    try:
        out = run()
        return out, set(ctx.timing_report())
    finally:
        ctx.timing_enable(False)


def test_one_launch_per_node_and_none_where_nothing_is_to_match(ctx):
    items = [ROW_POOL[i % len(ROW_POOL)] for i in range(500)]
    t = ctx.table_from_host([utf8_column(items)])
    empty = ctx.table_from_host([utf8_column([])])
    run = lambda op, p, tab=t: launches(ctx, lambda: ctx.expr_evaluate(tab, match(op, col(0), p).flatten(F)))
    for op, p in ((LIKE, b"ab"), (LIKE, b"ab%"), (LIKE, b"%ab"), (LIKE, b"a%b"), (ILIKE, b"A%"), (STARTS_WITH, b"a"), (ENDS_WITH, b"b"), (NOT_LIKE, b"a%")):
        assert run(op, p)[1] == {"str_match_anchor"}, (op, p)
    for op, p in ((LIKE, b"%ab%"), (LIKE, b"a_%"), (LIKE, b"%a%b%"), (ILIKE, b"%A%"), (CONTAINS, b"a"), (STRPOS, b"a"), (LIKE, b"_")):
        assert run(op, p)[1] == {"str_match_scan"}, (op, p)
    for op, p in ((LIKE, b"%"), (CONTAINS, b""), (STARTS_WITH, b"")):  # ALWAYS: no matching kernel
        assert not run(op, p)[1] & {"str_match_anchor", "str_match_scan"}, (op, p)
    for op, p in ((NOT_LIKE, b"%"), (LIKE, None), (STRPOS, None)):
        assert run(op, p)[1] == set(), (op, p)
    for op, p in ((LIKE, b"a%"), (LIKE, b"%a_%"), (STRPOS, b"a"), (LIKE, None), (LIKE, b"%")):  # zero rows: a well-formed empty column
        out, ran = run(op, p, empty)
        assert ran == set(), (op, p, ran)
        assert_result(out, op, [], [], p is None, "0 rows")


# ----------------------------------------------------------------------------- every consumer, 257 rows
N_CONS = 257
NAMES = [b"ab-cd", b"abc", b" ab", b"ab", b"a b c", b"xab", b"ab ab", "abé".encode(), b"", b"a", b"b-a", b"  a  b  "]
FC = fields("id", "s", "v")


def consumer_table(ctx, nullable=False):
    from naive_query_engine_amd import Column

    rng = np.random.default_rng(8)
    items = [NAMES[int(i)] for i in rng.integers(0, len(NAMES), N_CONS)]
    ids = np.arange(N_CONS, dtype=np.int64)
    v = rng.integers(-50, 50, N_CONS).astype(np.float64)
    mask = (rng.random(N_CONS) > 0.25) if nullable else np.ones(N_CONS, dtype=bool)
    t = ctx.table_from_host([Column.from_numpy(ids), utf8_column(items, mask if nullable else None), Column.from_numpy(v)])
    return t, ids, items, v, mask


@pytest.mark.parametrize("nullable", (False, True))
def test_selection_alone_and_under_and_or(ctx, nullable):
    from naive_query_engine_amd import Operator
    from tests.string_fn_util import byte_strings

    e = ex()
    t, ids, items, v, mask = consumer_table(ctx, nullable)
    like = np.array([model(LIKE, s, b"ab%") for s in items])
    assert 0 < like.sum() < N_CONS
    # a NULL predicate emits a NULL row (quirk Q4)
    got = ctx.selection(t, e.like(col(1), "ab%").flatten(FC)).to_host()
    assert got[0].length == int((like & mask).sum() + (~mask).sum())
    assert (got[0].to_numpy()[got[0].valid_mask()] == ids[like & mask]).all()
    if not nullable:
        assert byte_strings(got[1]) == [s for s, k in zip(items, like) if k] and (got[2].to_numpy() == v[like]).all()
    # like … and v > 0: Kleene — false and NULL is false, true and NULL is NULL
    pred = e.binop(e.like(col(1), "ab%"), Operator.And, e.binop(col(2), Operator.Gt, e.lit_f64(0.0)))
    got = ctx.selection(t, pred.flatten(FC)).to_host()
    true_rows, null_rows = like & mask & (v > 0), ~mask & (v > 0)
    assert got[0].length == int(true_rows.sum() + null_rows.sum()) and (got[0].to_numpy()[got[0].valid_mask()] == ids[true_rows]).all()
    # like … or id % 3 = 0: true or NULL is true
    pred = e.binop(e.like(col(1), "ab%"), Operator.Or, e.binop(e.binop(col(0), Operator.Modulos, e.lit_i64(3)), Operator.Eq, e.lit_i64(0)))
    got = ctx.selection(t, pred.flatten(FC)).to_host()
    true_rows, null_rows = (like & mask) | (ids % 3 == 0), ~mask & (ids % 3 != 0)
    assert got[0].length == int(true_rows.sum() + null_rows.sum()) and (got[0].to_numpy()[got[0].valid_mask()] == ids[true_rows]).all()


@pytest.mark.parametrize("nullable", (False, True))
def test_projection_and_selection_projection(ctx, nullable):
    from naive_query_engine_amd import Operator

    e = ex()
    t, ids, items, v, mask = consumer_table(ctx, nullable)
    exprs = [e.like(col(1), "%b%"), e.strpos(col(1), "b"), e.not_ilike(col(1), "A_%"), e.binop(e.strpos(col(1), "-"), Operator.Plus, col(0)), col(0)]
    out = ctx.projection(t, [x.flatten(FC) for x in exprs])
    got = out.to_host()
    for k, (op, p) in enumerate(((LIKE, b"%b%"), (STRPOS, b"b"), (NOT_ILIKE, b"A_%"))):
        values, valid = model_rows(op, items, p, mask if nullable else None)
        assert got[k].to_numpy().tolist() == values and got[k].valid_mask().tolist() == valid and out.column_info(k).null_count == int((~mask).sum()), k
    assert (got[3].to_numpy()[mask] == (np.array([model(STRPOS, s, b"-") for s in items]) + ids)[mask]).all() and (got[4].to_numpy() == ids).all()
    # the node in the predicate, in the list, or in both
    keep = np.array([model(CONTAINS, s, b" ") for s in items]) & mask
    nulls = int((~mask).sum())
    got = ctx.selection_projection(t, e.contains(col(1), " ").flatten(FC), [col(0).flatten(FC), e.strpos(col(1), "b").flatten(FC)]).to_host()
    assert got[0].length == int(keep.sum()) + nulls and (got[0].to_numpy()[got[0].valid_mask()] == ids[keep]).all()
    small = ids < 100
    got = ctx.selection_projection(t, e.binop(col(0), Operator.Lt, e.lit_i64(100)).flatten(FC), [e.ends_with(col(1), "b").flatten(FC), col(0).flatten(FC)]).to_host()
    values, valid = model_rows(ENDS_WITH, [s for s, k in zip(items, small) if k], b"b", mask[small] if nullable else None)
    assert got[0].to_numpy().tolist() == values and got[0].valid_mask().tolist() == valid and (got[1].to_numpy() == ids[small]).all()


@pytest.mark.parametrize("nullable", (False, True))
def test_aggregate_predicate_and_group_key(ctx, nullable):
    from naive_query_engine_amd import AggregateFunc

    e = ex()
    t, ids, items, v, mask = consumer_table(ctx, nullable)
    like = np.array([model(LIKE, s, b"%a_b%") for s in items]) & mask
    assert 0 < like.sum() < N_CONS
    pred = e.like(col(1), "%a_b%").flatten(FC)
    got = [c.to_numpy()[0] for c in ctx.aggregate(t, [(AggregateFunc.Count, 2), (AggregateFunc.Sum, 2), (AggregateFunc.Min, 2), (AggregateFunc.Max, 2)], pred_nodes=pred).to_host()]
    assert got == [like.sum(), v[like].sum(), v[like].min(), v[like].max()]
    # group by strpos(s, 'b'): a row with a NULL key is dropped
    pos = np.array([model(STRPOS, s, b"b") for s in items])
    key = e.strpos(col(1), "b").flatten(FC)
    for p, sel in ((None, mask), (pred, like)):
        exp = Counter(pos[sel].tolist())
        got = ctx.group_aggregate(t, [key], [(AggregateFunc.Count, 0)], pred_nodes=p).to_host()
        assert got[0].to_numpy().tolist() == sorted(exp) and got[1].to_numpy().tolist() == [exp[k] for k in sorted(exp)]


def test_plan_mirrors_fused_and_unfused_and_a_sort_key(ctx):
    from naive_query_engine_amd import DType, Field, Operator, RecordBatch
    from naive_query_engine_amd import physical_plan as pp
    from naive_query_engine_amd.rewrite import plan_shape, rewrite

    e = ex()
    for nullable in (False, True):
        t, ids, items, v, mask = consumer_table(ctx, nullable)
        flds = [Field("id", DType.INT64, False), Field("s", DType.UTF8, nullable), Field("v", DType.FLOAT64, False)]
        scan = lambda: pp.ScanPlan.create(pp.MemTable.try_create(flds, [RecordBatch(flds, t.to_host())], ctx), None)
        pred = e.binop(e.ilike(col("s"), "AB%"), Operator.And, e.binop(col("v"), Operator.Gt, e.lit_f64(0.0)))
        exprs = [col("id"), e.strpos(col("s"), "b"), e.contains(col("s"), "-")]
        schema = [flds[0], Field("strpos", DType.INT64, nullable), Field("contains", DType.BOOLEAN, nullable)]
        chain = pp.ProjectionPlan.create(pp.SelectionPlan.create(scan(), pred), schema, exprs)
        fused = rewrite(pp.ProjectionPlan.create(pp.SelectionPlan.create(scan(), pred), schema, exprs))
        assert plan_shape(fused) == ["FusedSelectionProjectionPlan", "ScanPlan"] and plan_shape(chain) == ["ProjectionPlan", "SelectionPlan", "ScanPlan"]
        a, b = chain.execute()[0].table.to_host(), fused.execute()[0].table.to_host()
        keep = np.array([model(ILIKE, s, b"AB%") for s in items]) & mask & (v > 0)
        assert 0 < keep.sum() < N_CONS
        for got in (a, b):
            rows = got[0].valid_mask()
            assert (got[0].to_numpy()[rows] == ids[keep]).all()
            assert (got[1].to_numpy()[rows] == np.array([model(STRPOS, s, b"b") for s in items])[keep]).all()
            assert (got[2].to_numpy()[rows] == np.array([model(CONTAINS, s, b"-") for s in items])[keep]).all()
        assert a[0].length == b[0].length == int(keep.sum() + (~mask & (v > 0)).sum())
    # ORDER BY strpos(s, 'b'): the temporary key column is dropped again; stable
    t, ids, items, v, _ = consumer_table(ctx)
    flds = [Field("id", DType.INT64, False), Field("s", DType.UTF8, False), Field("v", DType.FLOAT64, False)]
    scan = pp.ScanPlan.create(pp.MemTable.try_create(flds, [RecordBatch(flds, t.to_host())], ctx), None)
    out = pp.PhysicalSortPlan.create(scan, [pp.PhysicalSortExpr(e.strpos(col("s"), "b"))]).execute()
    assert len(out) == 1 and out[0].num_columns == 3
    order = sorted(range(N_CONS), key=lambda i: model(STRPOS, items[i], b"b"))
    assert out[0].table.to_host()[0].to_numpy().tolist() == [int(ids[i]) for i in order]


# ----------------------------------------------------------------------------- errors, decided before any launch
def test_error_ladder_through_every_entry(ctx):
    from naive_query_engine_amd import Column, DType, ErrorCode, ScalarValue, Status, UnaryOperator
    from naive_query_engine_amd.arrow_host import node_column, node_string_match
    from naive_query_engine_amd.expression import PhysicalLiteralExpr, lit_i64, lit_utf8, strop

    n = 100
    t = ctx.table_from_host([Column.from_numpy(np.arange(n, dtype=np.int64)), Column.from_numpy(np.arange(n, dtype=np.uint64)),
                             Column.from_numpy(np.arange(n) % 2 == 0), Column.from_numpy(np.ones(n)), Column.from_list(["ab"] * n, DType.UTF8)])
    f = fields("i", "u", "b", "v", "s")
    I, U, B, V, S = (col(k) for k in range(5))
    entries = [("expr_evaluate", lambda nodes: ctx.expr_evaluate(t, nodes)), ("selection", lambda nodes: ctx.selection(t, nodes)),
               ("projection", lambda nodes: ctx.projection(t, [nodes])), ("selection_projection", lambda nodes: ctx.selection_projection(t, B.flatten(f), [nodes])),
               ("selection_projection predicate", lambda nodes: ctx.selection_projection(t, nodes, [I.flatten(f)]))]

    def status_of(nodes, only_evaluate=False):
        seen = set()
        for name, run in entries[:1] if only_evaluate else entries:
            ctx.timing_enable(True)
            ctx.timing_reset()
            try:
                with pytest.raises(ErrorCode) as err:
                    run(nodes)
                assert ctx.timing_report() == {}, (name, "a kernel was launched before the error was raised")
                seen.add(err.value.status)
            finally:
                ctx.timing_enable(False)
        assert len(seen) == 1, seen
        return seen.pop()

    null_typed = PhysicalLiteralExpr.create(ScalarValue.Null())
    # 1. op outside nqe_match_operator — before the empty stack (2.) and the Int64 `s` (3.)
    bad = node_string_match(0)
    for op in (8, 13, -1, 1000):
        bad.op = op
        assert status_of([bad], only_evaluate=True) == Status.InvalidArgument
        assert status_of([node_column(0), node_column(0), bad]) == Status.InvalidArgument
    # 2. fewer than two values — before `s` (3.) and the pattern (4.)
    for op in range(8):
        assert status_of([node_string_match(op)], only_evaluate=True) == Status.InvalidArgument
        assert status_of([node_column(0), node_string_match(op)], only_evaluate=True) == Status.InvalidArgument
    # 3. `s` not Utf8 — also with a pattern 4. would refuse
    for c in (I, U, B, V, lit_i64(3), null_typed, strop(UnaryOperator.CharacterLength, S)):
        assert status_of(match(LIKE, c, b"a").flatten(f)) == Status.NotSupported
        assert status_of(match(STRPOS, c, I).flatten(f)) == Status.NotSupported
    # 4. a pattern that is not a Utf8 literal: a column, a subtree, another dtype, a Null-typed literal
    for p in (S, strop(UnaryOperator.Trim, S), strop(UnaryOperator.Lower, lit_utf8("a")), I, lit_i64(1), null_typed, PhysicalLiteralExpr.create(ScalarValue.Int64(None))):
        for op in (LIKE, NOT_ILIKE, CONTAINS, STRPOS):
            assert status_of(match(op, S, p).flatten(f)) == Status.NotSupported
    # 5. more than NQE_MAX_MATCH_PATTERN bytes
    for op in (LIKE, ENDS_WITH, STRPOS):
        assert status_of(match(op, S, b"a" * 4097).flatten(f)) == Status.NotSupported
    # kind 7 is unknown
    kind7 = node_string_match(0)
    kind7.kind = 7
    assert status_of([node_column(4), lit_utf8("a").flatten(f)[0], kind7]) == Status.InvalidArgument
    # and a well-formed call still works on this context, the largest pattern included
    assert ctx.expr_evaluate(t, match(LIKE, S, b"a_").flatten(f)).to_host()[0].to_numpy().all()
    assert not ctx.expr_evaluate(t, match(LIKE, S, b"a" * 4096).flatten(f)).to_host()[0].to_numpy().any()
    assert ctx.selection(t, match(STARTS_WITH, S, b"a").flatten(f)).to_host()[0].length == n
