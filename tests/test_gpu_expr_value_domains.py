"""Edge values through every place that evaluates an expression on the device, against the independent model of the semantics
(tests/expr_value_util.py): Int64 and UInt64 over their whole ranges with the range ends planted, Float64 with NaN, +-inf, +-0, subnormals and
f64::MAX.  Compared exactly — bit for bit, the sign of zero included, any NaN equal to any NaN — on plain and on nullable columns.

Every case asserts from the timing report that the path it is named after ran (and that the path it replaces did not), so a path that is
not reached fails instead of passing vacuously.  Several kernels share a label; which instance runs is decided by
  expr.hip:150-158       expr_tree / expr_tree_compact: (some column nullable or a NULL literal or a NULL predicate, <= 2 / 3-4 distinct columns)
  expr.hip:211-222       a tree that fits the stack machine -> expr_tree (or expr_jit from three steps and NQE_JIT_MIN_ROWS rows on)
  selection.hip:298-352  keep_from_simple: a range test over a plain 8-byte column -> the range tile (Float64: through the order map), anything
                         else -> the interpreting kernel; keep_from_conj<NC>: NC = the distinct tested columns, 1-4
  selection.hip:512-527  compact_expr: plain words from 64 tiles on -> staged (`x * mul + add` chains: the affine form, else interpreted), plain
                         words below -> strided, a Boolean output or validity -> the general kernel
and the cases reach each instance by construction (table plain / nullable, the tree's distinct columns, the row count).

Row counts: 257 (one 256-row chunk and a ragged one), 8449 (two 4096-row tiles and a ragged one, past one 6144-row ticket of the fused
selection), 64 * 4096 + 1 for the two staged compaction forms.  The specialised kernels are cached per context: those cases run in a
context of their own, once interpreted (the kernel is being compiled), once specialised, both against the model.

Not reachable: keep_from_conj with ONE test behind an arithmetic step — `(a + 1) > 5` alone is a SimpleExpr, which selection and aggregate
both take first (selection.hip mask_for_predicate, aggregate.hip plan_predicate): those run here through keep_from_simple's interpreting
kernel and inside the lists.  agg_grouped_jit takes fault-free keys and predicates only (expr.hip plan_aggregate_key, aggregate.hip
plan_predicate), so it has no fault case; keys and predicates that can fault go through the aggregate's checked kernels
(test_faults_through_the_aggregate)."""
import contextlib
import functools
import os

import numpy as np
import pytest

from naive_query_engine_amd import AggregateFunc
from naive_query_engine_amd.arrow_host import ErrorCode
from tests import expr_value_util as ev
from tests.expr_value_util import A, B, ID, UU, XX, Z, F, I, L, O, U, X
from tests.helpers import fields

pytestmark = pytest.mark.gpu

FLD = fields(*ev.NAMES)
N_CHUNK, N_TILES, N_STAGED = 257, 8449, 64 * 4096 + 1
SWITCHES = ("NQE_NO_EXPR_TREE", "NQE_NO_JIT", "NQE_JIT_MIN_ROWS", "NQE_NO_JIT_DISK_CACHE", "NQE_JIT_SYNC", "NQE_NO_FUSED_SELECT", "NQE_NO_AGG_JIT", "NQE_NO_PLAN_HINTS",
            "NQE_NO_KEY_SAMPLE", "NQE_DEBUG")
JIT = {"NQE_JIT_MIN_ROWS": "1000", "NQE_NO_JIT_DISK_CACHE": "1"}
NULLABLE = [False, True]
NULLABLE_IDS = ["plain", "nullable"]
EVALUATED = dict(ev.VALUE_TREES, **ev.PRED_TREES, **ev.CONJ_TREES)
TREES = {k: v for k, v in EVALUATED.items() if ev.chain_steps(v) is None}        # what the stack machine is for: everything but col-op-lit chains
DEEP = {k: v for k, v in dict(ev.VALUE_TREES, **ev.PRED_TREES).items() if ev.steps_of(v) >= 3}   # what the specialised kernels take
KEEP_ALL = X(ID, O.GtEq, I(0))
AGGS = [(AggregateFunc.Count, ev.NAMES.index("z")), (AggregateFunc.Min, ev.NAMES.index("z")), (AggregateFunc.Max, ev.NAMES.index("z"))]


@contextlib.contextmanager
def switches(env):
    """the switches are read per call: exactly `env` is set while a case runs, and what was set before is restored"""
    saved = {k: os.environ.pop(k, None) for k in SWITCHES}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


class Device:
    """a context and the tables uploaded to it"""

    def __init__(self):
        from naive_query_engine_amd import capi

        self.ctx = capi.Context(0)
        self.tables = {}

    def table(self, t):
        if id(t) not in self.tables:
            self.tables[id(t)] = (t, self.ctx.table_from_host(t.columns()))
        return self.tables[id(t)][1]

    def close(self):
        self.tables.clear()
        self.ctx.close()


@pytest.fixture(scope="module")
def dev():
    d = Device()
    yield d
    d.close()


@pytest.fixture
def fresh():
    """a context of its own: the specialised kernels are cached per context"""
    d = Device()
    yield d
    d.close()


@functools.lru_cache(maxsize=None)
def host_table(n, nullable, plant=frozenset(), null_the_faults=False):
    """the catalogue's table plants no faulting divisor in z / zf"""
    return ev.make_table(n, 7 * n + 2 * int(nullable) + int(null_the_faults) + 13 * len(plant), nullable, plant=plant, null_the_faults=null_the_faults)


def fault_tables(case, n=N_TILES):
    """(plain, nullable, nullable with every fault under a NULL slot) of one fault case"""
    plant = ev.FAULT_CASES[case][1]
    plant = frozenset([plant] if plant else [])
    return host_table(n, False, plant), host_table(n, True, plant), host_table(n, True, plant, True)


def nodes(tree):
    return ev.to_expr(tree).flatten(FLD)


@functools.lru_cache(maxsize=256)
def model(t, op, pred, trees):
    if op == "evaluate":
        return ev.outcome(ev.model_evaluate, trees[0], t)
    if op == "select":
        return ev.outcome(ev.model_select, pred, t)
    return ev.outcome(ev.model_select_project, pred, list(trees), t)


def execute(dev, t, op, pred, trees):
    d, ctx = dev.table(t), dev.ctx
    ctx.timing_enable(True)
    ctx.timing_reset()
    try:
        if op == "evaluate":
            return ctx.expr_evaluate(d, nodes(trees[0])).to_host()
        if op == "select":
            return ctx.selection(d, nodes(pred)).to_host()
        return ctx.selection_projection(d, nodes(pred), [nodes(x) for x in trees]).to_host()
    finally:
        ctx.timing_enable(False)


def check(dev, t, op, pred=None, trees=(), what="", expect=None):
    """one execution against the model — the same status when the model raises; returns the launches {label: count}.
    expect: "raises" / "ok" — what the case is built to show (a table that does not plant its fault fails here, not silently)"""
    want = model(t, op, pred, tuple(trees))
    assert expect is None or want[0] == expect, f"{what}: the model {want[0]}, the case is built for {expect}"
    if want[0] == "raises":
        with pytest.raises(ErrorCode) as err:
            execute(dev, t, op, pred, trees)
        assert err.value.status == want[1], f"{what}: status {err.value.status}, the model raises {want[1]}"
    else:
        ev.assert_columns_match(execute(dev, t, op, pred, trees), want[1], what)
    return {name: cnt for name, (_, cnt) in sorted(dev.ctx.timing_report().items())}


def ran(names, want, forbid=(), what=""):
    """want: {label: launches, or None for at least one}"""
    for label, count in want.items():
        got = names.get(label, 0)
        assert got == count if count is not None else got >= 1, f"{what}: {label} ran {got} times, expected {count if count is not None else 'at least once'}: {names}"
    for label in forbid:
        assert label not in names, f"{what}: {label} ran: {names}"


def report(path, trees, names):
    print(f"PATH {path}: {trees} trees, labels {names}")


def by_columns(trees, wide):
    """the trees over <= 2 (wide = False) or 3-4 distinct columns: the NC = 2 / NC = 4 instances (expr.hip:150-158)"""
    return {k: v for k, v in trees.items() if (len(ev.columns_of(v)) > 2) == wide}


# --------------------------------------------------------------------------- expr_evaluate
@pytest.mark.parametrize("nullable", NULLABLE, ids=NULLABLE_IDS)
def test_node_at_a_time(dev, nullable):
    """NQE_NO_EXPR_TREE=1: one expr_binary launch per operator node (expr.hip eval_node), make_aux per literal divisor"""
    t = host_table(N_CHUNK, nullable)
    trees = dict(EVALUATED, **ev.PLAIN_COMPARES, **ev.AFFINE_CHAINS, **ev.WORD_CHAINS)
    with switches({"NQE_NO_EXPR_TREE": "1"}):
        for name, tree in trees.items():
            names = check(dev, t, "evaluate", trees=[tree], what=f"node at a time, {name}")
            ran(names, {"expr_binary": ev.steps_of(tree)}, ("expr_tree", "expr_jit"), name)
    report(f"expr_binary nullable={nullable}", len(trees), names)


@pytest.mark.parametrize("wide", [False, True], ids=["2_columns", "4_columns"])
@pytest.mark.parametrize("nullable", NULLABLE, ids=NULLABLE_IDS)
def test_expr_tree(dev, nullable, wide):
    """expr_tree_kernel<NULLS, 2 / 4> (expr.hip:150-153: needs_valid — a nullable column or a NULL literal —, P.ncols <= 2); 257 rows: one whole
    256-row chunk and one of a single row.  Chains are one- to four-step programs of the same machine here (expr.hip:211-217)"""
    t = host_table(N_CHUNK, nullable)
    trees = by_columns(dict(EVALUATED, **ev.PLAIN_COMPARES, **ev.AFFINE_CHAINS, **ev.WORD_CHAINS), wide)
    assert len(trees) >= 8
    for name, tree in trees.items():
        names = check(dev, t, "evaluate", trees=[tree], what=f"expr_tree, {name}")
        ran(names, {"expr_tree": 1}, ("expr_binary", "expr_jit"), name)
    report(f"expr_tree nullable={nullable} wide={wide}", len(trees), names)


@pytest.mark.parametrize("nullable", NULLABLE, ids=NULLABLE_IDS)
@pytest.mark.parametrize("name", list(DEEP))
def test_expr_jit(fresh, name, nullable):
    """trees of three or more steps over NQE_JIT_MIN_ROWS rows: interpreted while the kernel is compiled, then expr_jit (expr_jit.hpp emit_steps:
    integer literal divisors baked in, Float64 `/` a real division where the interpreter multiplies by the reciprocal of +-2^k)"""
    t, tree = host_table(N_TILES, nullable), DEEP[name]
    with switches(JIT):
        first = check(fresh, t, "evaluate", trees=[tree], what=f"{name}, interpreted")
        ran(first, {"expr_tree": 1}, ("expr_jit",), name)
        fresh.ctx.jit_wait()
        names = check(fresh, t, "evaluate", trees=[tree], what=f"{name}, specialised")
        ran(names, {"expr_jit": 1}, ("expr_tree", "expr_binary"), name)
    report(f"expr_jit nullable={nullable} {name}", 1, names)


# --------------------------------------------------------------------------- behind a selection
PLAIN_PREDICATES = [X(UU, O.Gt, U(1 << 62)), X(XX, O.Lt, F(50.0))]      # an integer and a Float64 range test (NaN rows are dropped, NULL rows emitted)


@pytest.mark.parametrize("wide", [False, True], ids=["2_columns", "4_columns"])
@pytest.mark.parametrize("nullable", NULLABLE, ids=NULLABLE_IDS)
def test_expr_tree_compact(dev, nullable, wide):
    """expr_tree_compact_kernel<NULLS, 2 / 4> (expr.hip:155-158, 230: needs_valid || km.pvalid): a plain compare as predicate — over the nullable
    table its NULL rows are emitted as NULL rows in which literals stay valid —, every tree of the class in one projection list"""
    t = host_table(N_TILES, nullable)
    trees = by_columns(TREES, wide)
    assert len(trees) >= 6
    for pred in PLAIN_PREDICATES:
        names = check(dev, t, "select_project", pred, list(trees.values()), what=f"expr_tree_compact nullable={nullable} wide={wide} {list(trees)}")
        ran(names, {"expr_tree_compact": len(trees), "keep_from_simple": 1}, ("expr_tree", "expr_binary", "compact_expr", "proj_jit", "select_project_jit"))
    report(f"expr_tree_compact nullable={nullable} wide={wide}", len(trees), names)


COMPACT_FORMS = {
    # form: (rows, nullable, chains)            the kernel by selection.hip:512-527
    "general_nullable": (N_TILES, True, dict(ev.AFFINE_CHAINS, **ev.WORD_CHAINS, **ev.BOOL_CHAINS)),     # validity: compact_kernel<true, false, false>
    "general_boolean": (N_TILES, False, ev.BOOL_CHAINS),                                               # a Boolean output: the same kernel
    "strided": (N_TILES, False, dict(ev.AFFINE_CHAINS, **ev.WORD_CHAINS)),                             # plain words, 3 tiles: compact_strided_kernel<true>
    "staged_interpreted": (N_STAGED, False, {k: ev.WORD_CHAINS[k] for k in ("a_div_magic", "a_mod_shift", "x_div_pow2", "x_signed_zero")}),  # 65 tiles: compact_staged_kernel<1>
    "staged_affine": (N_STAGED, False, ev.AFFINE_CHAINS),                                              # … and `x * mul + add`: compact_staged_kernel<2> (affine_form)
}


@pytest.mark.parametrize("form", list(COMPACT_FORMS))
def test_compact_expr_chains(dev, form):
    """`col op lit` chains behind a selection: eval_simple inside the four compaction kernels, affine_form in the staged one"""
    n, nullable, chains = COMPACT_FORMS[form]
    t = host_table(n, nullable)
    for pred in PLAIN_PREDICATES[:1 if n == N_STAGED else 2]:
        names = check(dev, t, "select_project", pred, list(chains.values()), what=f"compact_expr {form} {list(chains)}")
        ran(names, {"compact_expr": len(chains), "keep_from_simple": 1}, ("expr_tree_compact", "expr_tree", "proj_jit"))
    report(f"compact_expr {form}", len(chains), names)


PROJECTION_LISTS = {
    "integers": ["int_wrap_chain", "magic_divisors", "column_divisors", "u64_divisors"],
    "divisors": ["shift_divisors", "magic_divisors_wide", "u64_shift_divisors", "null_literal"],
    "floats": ["contraction_bait", "fmod_column", "signed_zero", "kleene"],
    "reciprocals": ["reciprocal_limits", "reciprocal_outside", "true_division", "nan_inf_in_predicate"],
}


@pytest.mark.parametrize("nullable", NULLABLE, ids=NULLABLE_IDS)
@pytest.mark.parametrize("which", list(PROJECTION_LISTS))
def test_proj_jit(fresh, which, nullable):
    """a projection list of three or more steps in all behind a selection: per expression while the kernel is compiled, then ONE proj_jit pass
    (expr.hip project_specialised; nullable inputs: the NULL rows of the predicate are emitted and literals stay valid in them)"""
    t = host_table(N_TILES, nullable)
    trees = [EVALUATED[k] for k in PROJECTION_LISTS[which]]
    with switches(JIT):
        first = check(fresh, t, "select_project", PLAIN_PREDICATES[1], trees, what=f"{which}, per expression")
        ran(first, {"keep_from_simple": 1}, ("proj_jit", "select_project_jit"), which)
        fresh.ctx.jit_wait()
        names = check(fresh, t, "select_project", PLAIN_PREDICATES[1], trees, what=f"{which}, specialised")
        ran(names, {"proj_jit": 1, "keep_from_simple": 1}, ("expr_tree_compact", "compact_expr", "select_project_jit"), which)
    report(f"proj_jit nullable={nullable} {which}", len(trees), names)


FUSED = {
    # predicate TREE of three or more operators over plain 8-byte columns: the word-typed list evaluated behind it (with two bare columns: four outputs)
    "u64_compare_and_wrap": ["u64_divisors", "int_wrap_chain"],
    "i64_wrap_in_predicate": ["magic_divisors", "column_divisors"],
    "nan_inf_in_predicate": ["contraction_bait", "reciprocal_limits"],
    "float_columns_in_predicate": ["fmod_column", "true_division"],
    "four_columns_predicate": ["shift_divisors", "fmod_literal"],
    "list_and_3_pre_3col": ["magic_divisors_wide", "reciprocal_outside"],
    "nested_pre": ["u64_shift_divisors", "int_literal_minus"],
}


@pytest.mark.parametrize("fused", [True, False], ids=["one_pass", "no_fused_select"])
@pytest.mark.parametrize("which", list(FUSED))
def test_select_project_jit(fresh, which, fused):
    """selection and projection in one specialised pass (expr.hip select_project_fused: no NULLs anywhere; 8449 rows are past one 6144-row
    ticket).  NQE_NO_FUSED_SELECT=1: the mask of the same predicate, then proj_jit"""
    t = host_table(N_TILES, False)
    pred, trees = EVALUATED[which], [EVALUATED[k] for k in FUSED[which]] + [A, XX]
    with switches(JIT if fused else dict(JIT, NQE_NO_FUSED_SELECT="1")):
        first = check(fresh, t, "select_project", pred, trees, what=f"{which}, two kernels")
        ran(first, {}, ("proj_jit", "select_project_jit"), which)
        fresh.ctx.jit_wait()
        names = check(fresh, t, "select_project", pred, trees, what=f"{which}, specialised")
        if fused:
            ran(names, {"select_project_jit": 1}, ("proj_jit", "keep_from_simple", "keep_from_conj", "keep_from_pred", "expr_tree_compact"), which)
        elif len(ev.model_keep(pred, t)[0]) == 0:      # (`(u - 1) < 10 and …` keeps no row: the one-pass kernel still runs, a mask that keeps nothing projects nothing)
            ran(names, {"keep_from_conj": 1}, ("select_project_jit", "proj_jit", "expr_tree_compact"), which)
        else:
            ran(names, {"proj_jit": 1}, ("select_project_jit", "expr_tree_compact"), which)
    report(f"select_project_jit fused={fused} {which}", len(trees), names)


# --------------------------------------------------------------------------- the keep mask
@pytest.mark.parametrize("nullable", NULLABLE, ids=NULLABLE_IDS)
@pytest.mark.parametrize("column", list(ev.COMPARE_LITERALS))
def test_keep_from_simple(dev, column, nullable):
    """the plain compares as selection predicates (make_fast_pred): over a plain column the integer range tile (a, u) or the Float64 one through
    the order map (x: selection.hip:318-321); over a nullable column the interpreting kernel (selection.hip:323), which also takes the chains
    that are no range test"""
    t = host_table(N_TILES, nullable)
    preds = {k: v for k, v in ev.PLAIN_COMPARES.items() if ev.columns_of(v) == [column]}
    preds.update({k: v for k, v in dict(ev.CONJ_TREES, **ev.BOOL_CHAINS).items() if ev.chain_steps(v) is not None and ev.columns_of(v) == [column]})
    assert len(preds) >= 60
    for name, pred in preds.items():
        names = check(dev, t, "select", pred, what=f"keep_from_simple {name} nullable={nullable}")
        ran(names, {"keep_from_simple": 1}, ("keep_from_conj", "keep_from_pred", "expr_tree"), name)
    report(f"keep_from_simple {column} nullable={nullable}", len(preds), names)


def test_keep_from_conj(dev):
    """and / or lists of two to four tests and one nested shape over plain columns: the straight list of range tests and the truth-table form
    with its arithmetic pre-steps (match_conj, conj_pre), over 1, 2, 3 and 4 source columns (keep_from_conj_kernel<NC>: selection.hip:351)"""
    t = host_table(N_TILES, False)
    preds = {k: v for k, v in ev.CONJ_TREES.items() if ev.chain_steps(v) is None}
    assert sorted({len(ev.columns_of(v)) for v in preds.values()}) == [1, 2, 3, 4]
    for name, pred in preds.items():
        names = check(dev, t, "select", pred, what=f"keep_from_conj {name}")
        ran(names, {"keep_from_conj": 1}, ("keep_from_simple", "keep_from_pred", "expr_tree"), name)
    report("keep_from_conj", len(preds), names)


@pytest.mark.parametrize("nullable", NULLABLE, ids=NULLABLE_IDS)
def test_keep_from_pred(dev, nullable):
    """predicates match_conj declines — a column compared with a column, `a + 1 > a`, a Boolean column, and over nullable columns every list —:
    the tree's Boolean column through expr_tree, then keep_from_pred"""
    t = host_table(N_TILES, nullable)
    preds = dict(ev.PRED_TREES, **({k: v for k, v in ev.CONJ_TREES.items() if ev.chain_steps(v) is None} if nullable else {}))
    for name, pred in preds.items():
        names = check(dev, t, "select", pred, what=f"keep_from_pred {name} nullable={nullable}")
        ran(names, {"keep_from_pred": 1, "expr_tree": 1}, ("keep_from_simple", "keep_from_conj"), name)
    report(f"keep_from_pred nullable={nullable}", len(preds), names)


# --------------------------------------------------------------------------- aggregates
def model_groups(t, key, pred):
    """{key: (count, min, max)} of z over the rows the predicate passes — a NULL predicate emits a NULL row, whose NULL key drops it like any
    NULL key; a NULL value is not counted; rows the predicate drops never fault (the key is evaluated on the filtered batch)"""
    rows = range(t.n) if pred is None else [i for i, ok in zip(*ev.model_keep(pred, t)) if ok]
    k = ev.eval_tree(key, t)
    for i in rows:
        if k.fault[i]:
            raise ev.Fault(k.fault[i])
    z, zv = t.rows("z")
    groups = {}
    for i in rows:
        if not k.valid[i]:
            continue
        c, mn, mx = groups.get(k.vals[i], (0, ev.F64_MAX, -ev.F64_MAX))
        groups[k.vals[i]] = (c + 1, min(mn, float(z[i])), max(mx, float(z[i]))) if zv[i] else (c, mn, mx)
    return k.kind, groups


def check_groups(dev, t, key, pred, what, expect=None):
    d, ctx = dev.table(t), dev.ctx
    want = ev.outcome(lambda: [model_groups(t, key, pred)])
    assert expect is None or want[0] == expect, f"{what}: the model {want[0]}, the case is built for {expect}"
    ctx.timing_enable(True)
    ctx.timing_reset()
    try:
        if want[0] == "raises":
            with pytest.raises(ErrorCode) as err:
                ctx.aggregate(d, AGGS, group_nodes=nodes(key), pred_nodes=nodes(pred) if pred is not None else None, with_keys=True)
            assert err.value.status == want[1], f"{what}: status {err.value.status}, the model raises {want[1]}"
        else:
            out, keys = ctx.aggregate(d, AGGS, group_nodes=nodes(key), pred_nodes=nodes(pred) if pred is not None else None, with_keys=True)
    finally:
        ctx.timing_enable(False)
    names = {name: cnt for name, (_, cnt) in sorted(ctx.timing_report().items())}
    if want[0] == "raises":
        return names
    kind, groups = want[1][0]
    cnt, mn, mx = (c.to_numpy() for c in out.to_host())
    got_keys = keys.to_host()[0].to_numpy() if keys is not None else np.zeros(0, dtype=ev.NP_DTYPES[kind])
    assert got_keys.dtype == ev.NP_DTYPES[kind], f"{what}: keys are {got_keys.dtype}"
    got = {int(k): (int(c), float(a), float(b)) for k, c, a, b in zip(got_keys.tolist(), cnt.tolist(), mn.tolist(), mx.tolist())}
    assert len(got) == len(got_keys), f"{what}: a key occurs twice"
    assert got == groups, f"{what}: {len(got)} groups, the model has {len(groups)}; differing keys {sorted(k for k in set(got) | set(groups) if got.get(k) != groups.get(k))[:6]}"
    return names


# The aggregate's kernels load the key column, the first value column and at most ONE more: lists and trees over those are evaluated per row
# inside them (conj_pass / conj_pre, the predicate stack machine); anything wider is materialised as a Boolean column first (expr_tree).
_P, _ID3 = ev.PRE_TESTS, X(X(ID, O.Modulos, I(3)), O.Eq, I(0))
AGG_LISTS = {
    "list_and_2_pre_1col": ev.CONJ_TREES["list_and_2_pre_1col"],
    "and_a_z": ev.AND(_P["a_plus"], X(Z, O.Gt, I(0))),
    "or_a_id": ev.OR(_P["a_times"], _ID3),
    "or_u_id_z": ev.OR(_P["u_minus"], _ID3, X(Z, O.Lt, I(-5))),
    "or_x_z": ev.OR(_P["x_times"], X(Z, O.Lt, I(-5))),
    "and_x_id": ev.AND(_P["x_plus_huge"], X(ID, O.Lt, I(5000))),
    "and_4_a_id_z": ev.AND(_P["a_div"], _P["lit_minus_a"], X(ID, O.GtEq, I(1)), X(Z, O.NotEq, I(2))),
    "plain_or_3": ev.OR(X(XX, O.Lt, F(-0.0)), X(ID, O.Lt, I(100)), X(Z, O.Eq, I(9))),
    "nested_a_z": ev.OR(ev.AND(_P["a_plus"], _P["a_mod"]), X(Z, O.Gt, I(3))),
}
AGG_TREES = {
    "u64_compare_and_wrap": ev.PRED_TREES["u64_compare_and_wrap"],
    "nan_inf_in_predicate": ev.PRED_TREES["nan_inf_in_predicate"],
    "i64_wrap_against_z": ev.AND(X(X(A, O.Plus, I(1)), O.Gt, A), X(X(A, O.Multiply, I(2)), O.LtEq, Z)),      # (a + 1) > a and (a * 2) <= z
    "contraction_in_predicate": X(X(X(XX, O.Multiply, XX), O.Plus, F(0.25)), O.GtEq, F(2.5)),                 # x * x + 0.25 >= 2.5 (one value alive at a time)
}
AGG_MATERIALISED = {k: v for k, v in ev.CONJ_TREES.items() if len(ev.columns_of(v)) > 1}
AGG_PREDICATES = {
    # which: (predicates, a Boolean column is materialised for them)
    "a": ({k: v for k, v in ev.PLAIN_COMPARES.items() if ev.columns_of(v) == ["a"]}, False),
    "u": ({k: v for k, v in ev.PLAIN_COMPARES.items() if ev.columns_of(v) == ["u"]}, False),
    "x": ({k: v for k, v in ev.PLAIN_COMPARES.items() if ev.columns_of(v) == ["x"]}, False),
    "chains": ({k: v for k, v in dict(ev.CONJ_TREES, **ev.BOOL_CHAINS).items() if ev.chain_steps(v) is not None}, False),
    "lists": (AGG_LISTS, False),
    "trees": (AGG_TREES, False),
    "wider_lists": (AGG_MATERIALISED, True),
}


@pytest.mark.parametrize("which", list(AGG_PREDICATES))
def test_aggregate_under_a_predicate(dev, which):
    """count, min and max (all exact) of a small-integer column grouped by `id % 7` under the plain compares and chains (range tests and
    eval_simple inside the aggregate kernels), the lists (conj_pass, conj_pre) and trees (the predicate stack machine) over the columns those
    kernels load — no Boolean column is materialised for them — and the catalogue's wider lists, which are"""
    t = host_table(N_TILES, False)
    key = X(ID, O.Modulos, I(7))
    preds, materialised = AGG_PREDICATES[which]
    with switches({"NQE_NO_AGG_JIT": "1"}):
        for name, pred in preds.items():
            names = check_groups(dev, t, key, pred, f"aggregate under {name}")
            assert any(k.startswith("agg_grouped") for k in names), f"{name}: {names}"
            if materialised:
                ran(names, {"expr_tree": 1}, ("agg_grouped_jit",), name)
            else:
                ran(names, {}, ("expr_tree", "expr_binary", "keep_from_pred", "agg_grouped_jit"), name)
    report(f"aggregate under a predicate, {which}", len(preds), names)


# (the kernel loads at most four columns: the key's, the value's and the predicate's)
AGG_JIT_PREDICATES = ["u64_compare_and_wrap", "i64_wrap_in_predicate", "nan_inf_in_predicate", "float_columns_in_predicate", "list_and_2_pre_1col", "list_or_2_pre_2col", "nested_pre"]


@pytest.mark.parametrize("name", AGG_JIT_PREDICATES)
def test_agg_grouped_jit(fresh, name):
    """key `id % 600`, one value column, a predicate tree of three or more operators as straight-line code in the specialised streaming kernel
    (emit_steps in nqe_jit_agg): the static kernels while it is compiled, then agg_grouped_jit"""
    t = host_table(N_TILES, False)
    key, pred = X(ID, O.Modulos, I(600)), EVALUATED[name]
    with switches(JIT):
        first = check_groups(fresh, t, key, pred, f"{name}, static")
        ran(first, {}, ("agg_grouped_jit",), name)
        fresh.ctx.jit_wait()
        names = check_groups(fresh, t, key, pred, f"{name}, specialised")
        ran(names, {"agg_grouped_jit": 1}, ("agg_grouped_fast", "agg_grouped"), name)
    report(f"agg_grouped_jit {name}", 1, names)


GROUP_KEYS = {
    "a_mod_1000": X(A, O.Modulos, I(1000)),
    "a_mod_minus_7": X(A, O.Modulos, I(-7)),
    "a_div_wide": X(A, O.Divide, I((1 << 40) + 7)),
    "u_mod_2p20": X(UU, O.Modulos, U(1 << 20)),
}


@pytest.mark.parametrize("name", list(GROUP_KEYS))
def test_group_keys_through_eval_simple(dev, name):
    """group keys over the wide columns: the key set and every key's count, min and max equal the model's (eval_simple<false> in the aggregate
    kernels: the magic multiply and the shift / mask of make_aux over the whole range, negative dividends and a negative divisor)"""
    t = host_table(N_TILES, False)
    with switches({"NQE_NO_AGG_JIT": "1"}):
        for pred in (None, X(A, O.Lt, I(0))):
            names = check_groups(dev, t, GROUP_KEYS[name], pred, f"group by {name} pred={pred is not None}")
            assert any(k.startswith("agg_") for k in names), names
            ran(names, {}, ("expr_tree", "expr_binary"), name)
    report(f"group keys {name}", 1, names)


# --------------------------------------------------------------------------- faults
def predicate_of(tree):
    """the faulting tree inside a predicate"""
    return X(tree, O.Eq, L(ev.kind_of(tree), 1 if ev.kind_of(tree) != "f" else 1.0))


@pytest.mark.parametrize("case", list(ev.FAULT_CASES))
def test_faults_through_the_interpreting_paths(dev, case):
    """a zero divisor (integer, +0.0, -0.0) and i64::MIN / -1, % -1 (column and literal divisor) raise ArrowError from a valid kept row through
    expr_tree, expr_binary, expr_tree_compact and a predicate's tree — and do not under a NULL slot or in a row the predicate drops"""
    tree, _, guard = ev.FAULT_CASES[case]
    plain, nullable, nulled = fault_tables(case)
    # (the literal divisor -1 makes a chain: behind a selection and as a predicate it is the consumer kernels' — test_faults_through_the_chains)
    chain = ev.chain_steps(tree) is not None
    behind, mask = ("compact_expr", "keep_from_simple") if chain else ("expr_tree_compact", "keep_from_pred")
    for t in (plain, nullable):
        ran(check(dev, t, "evaluate", trees=[tree], what=f"{case} expr_tree", expect="raises"), {"expr_tree": 1})
        with switches({"NQE_NO_EXPR_TREE": "1"}):
            ran(check(dev, t, "evaluate", trees=[tree], what=f"{case} expr_binary", expect="raises"), {"expr_binary": 1})
        ran(check(dev, t, "select_project", KEEP_ALL, [tree, A], what=f"{case} {behind}, kept", expect="raises"), {behind: 1})
        ran(check(dev, t, "select_project", guard, [tree, A], what=f"{case} {behind}, dropped", expect="ok"), {behind: 1})
        ran(check(dev, t, "select", predicate_of(tree), what=f"{case} in a predicate", expect="raises"), {mask: 1})
    ran(check(dev, nulled, "evaluate", trees=[tree], what=f"{case} expr_tree, NULL slots", expect="ok"), {"expr_tree": 1})
    with switches({"NQE_NO_EXPR_TREE": "1"}):
        ran(check(dev, nulled, "evaluate", trees=[tree], what=f"{case} expr_binary, NULL slots", expect="ok"), {"expr_binary": 1})
    ran(check(dev, nulled, "select_project", KEEP_ALL, [tree, A], what=f"{case} {behind}, NULL slots", expect="ok"), {behind: 1})
    ran(check(dev, nulled, "select", predicate_of(tree), what=f"{case} in a predicate, NULL slots", expect="ok"), {mask: 1})


@pytest.mark.parametrize("case", list(ev.CHAIN_FAULTS))
def test_faults_through_the_chains(dev, case):
    """`a / -1` with i64::MIN present, `100 / a`, `100 % a` with 0 present, `1.0 / x` with both zeros present: eval_simple in the strided, staged
    and general compaction kernels and in keep_from_simple's interpreting kernel"""
    tree, guard = ev.CHAIN_FAULTS[case]
    for form, t in (("strided", host_table(N_TILES, False)), ("general", host_table(N_TILES, True)), ("staged", host_table(N_STAGED, False))):
        ran(check(dev, t, "select_project", KEEP_ALL, [tree], what=f"{case} {form}, kept", expect="raises"), {"compact_expr": 1}, ("expr_tree_compact",))
        ran(check(dev, t, "select_project", guard, [tree], what=f"{case} {form}, dropped", expect="ok"), {"compact_expr": 1}, ("expr_tree_compact",))
        if form != "staged":
            ran(check(dev, t, "select", predicate_of(tree), what=f"{case} {form}, in a predicate", expect="raises"), {"keep_from_simple": 1})
    if case == "a_over_minus_one":
        nulled = fault_tables("min_divided_by_minus_one_literal")[2]
        ran(check(dev, nulled, "select_project", KEEP_ALL, [tree], what=f"{case}, NULL slots", expect="ok"), {"compact_expr": 1})
        ran(check(dev, nulled, "select", predicate_of(tree), what=f"{case} in a predicate, NULL slots", expect="ok"), {"keep_from_simple": 1})


@pytest.mark.parametrize("case", list(ev.CHAIN_FAULTS))
def test_faults_through_the_aggregate(dev, case):
    """the chains that fault as a group key (eval_simple in the general aggregate kernel: a key that may fault never takes the unchecked
    kernels) — raised from a row the predicate keeps, not from one it drops — and as the predicate"""
    tree, guard = ev.CHAIN_FAULTS[case]
    for t in (host_table(N_TILES, False), host_table(N_TILES, True)):
        if ev.kind_of(tree) != "f":      # (group by takes Int64 / UInt64 keys)
            names = check_groups(dev, t, tree, None, f"group by {case}", expect="raises")
            assert any(k.startswith("agg_") for k in names), names
            names = check_groups(dev, t, tree, guard, f"group by {case} behind its guard", expect="ok")
            assert any(k.startswith("agg_") for k in names), names
        names = check_groups(dev, t, X(ID, O.Modulos, I(7)), predicate_of(tree), f"aggregate under {case}", expect="raises")
    if case == "a_over_minus_one":
        nulled = fault_tables("min_divided_by_minus_one_literal")[2]
        check_groups(dev, nulled, tree, None, f"group by {case}, NULL slots", expect="ok")
        check_groups(dev, nulled, X(ID, O.Modulos, I(7)), predicate_of(tree), f"aggregate under {case}, NULL slots", expect="ok")


KEEP_ALL_TREE = ev.AND(X(B, O.NotEq, I(0)), X(B, O.NotEq, I(-1)), X(ID, O.GtEq, I(0)))      # three tests: every row of the plain table passes


@pytest.mark.parametrize("path", ["expr_jit", "proj_jit", "select_project_jit"])
@pytest.mark.parametrize("case", list(ev.FAULT_CASES))
def test_faults_through_the_specialised_paths(fresh, case, path):
    """the same faults from the interpreted and the specialised execution alike (the generated source restates the fault tests: emit_steps)"""
    tree, _, guard = ev.FAULT_CASES[case]
    wide = ev.widen(tree)
    plain, nullable, nulled = fault_tables(case)
    if path == "expr_jit":
        runs = [(t, "evaluate", None, [wide], "raises") for t in (plain, nullable)] + [(nulled, "evaluate", None, [wide], "ok")]
    elif path == "proj_jit":
        runs = [(t, "select_project", KEEP_ALL, [wide, A], "raises") for t in (plain, nullable)]
        runs += [(t, "select_project", guard, [wide, A], "ok") for t in (plain, nullable)] + [(nulled, "select_project", KEEP_ALL, [wide, A], "ok")]
    else:
        guard3 = ev.AND(guard, guard, X(ID, O.GtEq, I(0)))
        runs = [(plain, "select_project", KEEP_ALL_TREE, [tree, A], "raises"), (plain, "select_project", guard3, [tree, A], "ok")]
    with switches(JIT):
        for i, (t, op, pred, trees, expect) in enumerate(runs):
            first = check(fresh, t, op, pred, trees, what=f"{case} {path}, interpreted", expect=expect)
            if i == 0:      # (a later run may share its kernel with an earlier one, whose compilation may have finished)
                ran(first, {}, (path,), case)
        fresh.ctx.jit_wait()
        for t, op, pred, trees, expect in runs:
            names = check(fresh, t, op, pred, trees, what=f"{case} {path}, specialised", expect=expect)
            ran(names, {path: 1}, (), case)
    report(f"faults {path} {case}", len(runs), names)
