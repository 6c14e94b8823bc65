"""Shared by tests/test_gpu_plan_trees.py (device against oracle) and tests/test_plan_trees_oracle.py (oracle against numpy models):
multi-batch six-column tables whose batch lengths sit on the edges of the bitmap word, the 256-thread block and the 4096-row tile,
result comparison, and the seeded random plan trees (a tree is a `Node`; `to_plan` builds the mirror operators from it, `to_oracle`
runs the same tree through the oracle's operators, one `raw=True` handle feeding the next)."""
import numpy as np

from naive_query_engine_amd import AggregateFunc, Column, DType, ErrorCode, Field, Operator, RecordBatch
from naive_query_engine_amd.expression import binop, col, lit_f64, lit_i64, lit_u64
from oracle import oracle as orc
from tests.helpers import assert_batches_equal, random_batch, random_utf8

NAMES = ("id", "k", "v", "u", "b", "s")
DTYPES = (DType.INT64, DType.INT64, DType.FLOAT64, DType.UINT64, DType.BOOLEAN, DType.UTF8)
EDGES = [0, 1, 63, 64, 65, 127, 255, 257, 1000, 4095, 4096, 4097, 8193, 20000]
RTOL = 1e-9  # nqe.h's contract for sums taken in another order
A = AggregateFunc
EXACT_FUNCS = (A.Count, A.Min, A.Max)


def schema(prefix=""):
    return [Field(prefix + n, dt, True) for n, dt in zip(NAMES, DTYPES)]


def _with_values(old, vals):
    return Column.from_numpy(vals, old.valid_mask() if old.validity is not None else None)


def make_batch(rng, n, null_frac=0.0, nan_frac=0.0, id_base=None, id_nulls=True, v_all_null=False):
    """random_batch(with_bool=True) + random_utf8: [id Int64, k Int64, v Float64, u UInt64, b Boolean, s Utf8].  `v` is redrawn
    positive (1 .. 200, so that no sum is decided by cancellation), with NaN at `nan_frac`; `id_base`: ids are id_base + a
    permutation of 0..n-1 (unique over a table whose batches use disjoint ranges); id_nulls=False: the id column has no bitmap."""
    cols = random_batch(rng, n, null_frac, with_bool=True)
    v = rng.random(n) * 199.0 + 1.0
    if nan_frac:
        v[rng.random(n) < nan_frac] = np.nan
    cols[2] = Column.from_numpy(v, np.zeros(n, dtype=bool)) if v_all_null else _with_values(cols[2], v)
    ids = cols[0].to_numpy() + (0 if id_base is None else id_base)
    cols[0] = _with_values(cols[0], ids) if id_nulls else Column.from_numpy(ids)
    cols.append(random_utf8(rng, n, null_frac))
    return cols


def make_batches(seed, lengths, null_fracs, **kw):
    rng = np.random.default_rng(seed)
    return [make_batch(rng, n, nf, **kw) for n, nf in zip(lengths, null_fracs)]


def mem_table(pp, fields, batches, ctx):
    return pp.MemTable.try_create(fields, [RecordBatch(fields, b) for b in batches], ctx)


def batch_lengths(handle):
    L = orc.lib()
    return [int(L.orc_batch_num_rows(handle.ptr, i)) for i in range(L.orc_batches_count(handle.ptr))]


_LISTS = {}


def np_take(c, idx, also_valid=None):
    """rows `idx` of a host column, in numpy / Python; also_valid: a further per-output-row validity (False = NULL)"""
    idx = np.asarray(idx, dtype=np.int64)
    valid = c.valid_mask()[idx]
    if also_valid is not None:
        valid = valid & also_valid
    if c.dtype == DType.UTF8:
        if id(c) not in _LISTS:
            _LISTS[id(c)] = (c, c.to_list())  # holds the column, so that the id stays its own
        items = _LISTS[id(c)][1]
        return Column.from_list([items[i] if ok else None for i, ok in zip(idx, valid)], DType.UTF8)
    return Column.from_numpy(c.to_numpy()[idx], valid)


def assert_same_batches(got, exp, what=""):
    """got / exp: lists of batches (lists of host Columns): the same number of batches, the same lengths, and every batch equal
    with no tolerance (values, validity, strings)"""
    assert len(got) == len(exp), f"{what}: {len(got)} batches vs {len(exp)}"
    gl, el = [b[0].length if b else 0 for b in got], [b[0].length if b else 0 for b in exp]
    assert gl == el, f"{what}: batch lengths {gl} vs {el}"
    for i, (g, e) in enumerate(zip(got, exp)):
        assert_batches_equal(g, e, what=f"{what} batch {i}")


def assert_aggregate_equal(got, exp, funcs, what=""):
    """one aggregate output batch against the oracle's, rows as a multiset: count / min / max columns exact (NaN equals NaN), sum /
    avg columns within RTOL.  Rows are ordered by the exact columns first, so a sum's last bit never decides the pairing."""
    assert [c.dtype for c in got] == [c.dtype for c in exp], what
    assert len(got) == len(funcs)
    g, e = (np.stack([c.to_numpy().astype(np.float64) for c in cols], axis=1) for cols in (got, exp))
    assert g.shape == e.shape, f"{what}: shape {g.shape} vs {e.shape}"
    order = [i for i, f in enumerate(funcs) if f in EXACT_FUNCS] + [i for i, f in enumerate(funcs) if f not in EXACT_FUNCS]

    def srt(m):
        keys = []
        for c in order:
            nan = np.isnan(m[:, c])
            keys += [np.where(nan, np.inf, m[:, c]), nan.astype(np.float64)]
        return m[np.lexsort(keys[::-1])]

    g, e = srt(g), srt(e)
    for c, f in enumerate(funcs):
        if f in EXACT_FUNCS:
            same = (g[:, c] == e[:, c]) | (np.isnan(g[:, c]) & np.isnan(e[:, c]))
            assert same.all(), f"{what}: {A(f).name} column {c} differs at rows {np.nonzero(~same)[0][:6]}: {g[~same, c][:4]} vs {e[~same, c][:4]}"
        else:
            assert np.allclose(g[:, c], e[:, c], rtol=RTOL, atol=0, equal_nan=True), f"{what}: {A(f).name} column {c} differs beyond rtol={RTOL}"


# ----------------------------------------------------------------------------- plan trees
class Node:
    """op: scan(table) | sel(pred) | proj(exprs) | off(n) | lim(n) | join(lname, rname) | agg(key, aggs);
    `fields` is the operator's output schema, the one its parent resolves column names against"""

    def __init__(self, op, children=(), fields=None, **kw):
        self.op, self.children, self.fields, self.kw = op, list(children), fields, kw

    def __repr__(self):
        args = ", ".join(f"{k}={v!r}" for k, v in self.kw.items())
        inner = ", ".join(repr(c) for c in self.children)
        return f"{self.op}({args}{'; ' if args and inner else ''}{inner})"

    def depth(self):
        return (0 if self.op == "scan" else 1) + max([c.depth() for c in self.children], default=0)

    def ops(self):
        return [self.op] + [o for c in self.children for o in c.ops()]


_AGG_CLASS = {A.Count: "Count", A.Sum: "Sum", A.Avg: "Avg", A.Min: "Min", A.Max: "Max"}


def to_plan(node, pp, tables):
    """the mirror operators of a tree; tables: name -> MemTable"""
    kids = [to_plan(c, pp, tables) for c in node.children]
    k = node.kw
    if node.op == "scan":
        return pp.ScanPlan.create(tables[k["table"]], None)
    if node.op == "sel":
        return pp.SelectionPlan.create(kids[0], k["pred"])
    if node.op == "proj":
        return pp.ProjectionPlan.create(kids[0], node.fields, k["exprs"])
    if node.op == "off":
        return pp.PhysicalOffsetPlan.create(kids[0], k["n"])
    if node.op == "lim":
        return pp.PhysicalLimitPlan.create(kids[0], k["n"])
    if node.op == "join":
        return pp.HashJoin.create(kids[0], kids[1], [(pp.ColumnRef(None, k["lname"]), pp.ColumnRef(None, k["rname"]))], pp.JoinType.Inner, node.fields)
    if node.op == "agg":
        ops = [getattr(pp, _AGG_CLASS[f]).create(col(c)) for f, c in k["aggs"]]
        return pp.PhysicalAggregatePlan.create([k["key"]] if k["key"] is not None else [], ops, kids[0])
    raise ValueError(node.op)


def _index_of(fields, name):
    return [f.name for f in fields].index(name)


def oracle_step(node, handles, host):
    """one operator of the oracle chain over its children's raw handles"""
    k = node.kw
    if node.op == "scan":
        return orc.upload(host[k["table"]], [int(d) for d in DTYPES])
    cf = node.children[0].fields
    if node.op == "sel":
        return orc.selection(handles[0], k["pred"].flatten(cf), raw=True)
    if node.op == "proj":
        return orc.projection(handles[0], [e.flatten(cf) for e in k["exprs"]], raw=True)
    if node.op == "off":
        return orc.offset(handles[0], k["n"], raw=True)
    if node.op == "lim":
        return orc.limit(handles[0], k["n"], raw=True)
    if node.op == "join":
        return orc.hash_join(handles[0], handles[1], _index_of(cf, k["lname"]), _index_of(node.children[1].fields, k["rname"]), raw=True)
    if node.op == "agg":
        return orc.aggregate(handles[0], k["aggs"], group_nodes=k["key"].flatten(cf) if k["key"] is not None else None, raw=True)
    raise ValueError(node.op)


def to_oracle(node, host):
    """the whole tree through the oracle's operators -> raw handle (raises ErrorCode where the reference fails)"""
    return oracle_step(node, [to_oracle(c, host) for c in node.children], host)


# ----------------------------------------------------------------------------- random trees
def _ref(rng, fields, i):
    """column i by name where the name resolves to it (first match, Q12) and by index otherwise"""
    if rng.random() < 0.5 and _index_of(fields, fields[i].name) == i:
        return col(fields[i].name)
    return col(i)


def _cols_of(fields, *dtypes):
    return [i for i, f in enumerate(fields) if f.dtype in dtypes]


_CMP = [Operator.Lt, Operator.LtEq, Operator.Gt, Operator.GtEq, Operator.Eq, Operator.NotEq]


def _pred_leaf(rng, fields, candidates):
    i = int(rng.choice(candidates))
    dt = fields[i].dtype
    if dt == DType.BOOLEAN:
        return _ref(rng, fields, i)
    op = _CMP[int(rng.integers(0, 4 if dt != DType.INT64 else 6))]
    if dt == DType.FLOAT64:
        lit = lit_f64(float(rng.choice([50.0, 100.0, 150.0, 1000.0, float("nan")])))
    elif dt == DType.UINT64:
        lit = lit_u64(int(rng.choice([1 << 38, 1 << 39, 1 << 39, 1 << 41])))
    else:
        lit = lit_i64(int(rng.choice([-10, 0, 7, 25, 100, 1000, 3000])))
    return binop(_ref(rng, fields, i), op, lit)


def random_pred(rng, fields, only=None):
    """one to three tests over Int64 / Float64 / UInt64 / Boolean columns joined by and / or; only: restrict to these columns"""
    cand = [i for i in _cols_of(fields, DType.INT64, DType.FLOAT64, DType.UINT64, DType.BOOLEAN) if only is None or i in only]
    if not cand:
        return None
    e = _pred_leaf(rng, fields, cand)
    for _ in range(int(rng.integers(0, 3))):
        e = binop(e, Operator.And if rng.random() < 0.5 else Operator.Or, _pred_leaf(rng, fields, cand))
    return e


def random_projection(rng, fields):
    """two to four expressions: bare columns of any type (the name is kept), sign-preserving Float64 arithmetic, Int64 / UInt64
    arithmetic with literals (a zero divisor only by design, rarely), a comparison.  -> (exprs, names)"""
    exprs, names = [], []
    for j in range(int(rng.integers(2, 5))):
        i = int(rng.integers(0, len(fields)))
        dt, r = fields[i].dtype, rng.random()
        if r < 0.45 or dt in (DType.UTF8, DType.BOOLEAN):
            exprs.append(_ref(rng, fields, i))
            names.append(fields[i].name)
            continue
        c = _ref(rng, fields, i)
        if dt == DType.FLOAT64:
            op, v = [(Operator.Multiply, 2.0), (Operator.Plus, 1.5), (Operator.Divide, 4.0)][int(rng.integers(0, 3))]
            e = binop(c, op, lit_f64(v))
        elif dt == DType.UINT64:
            e = binop(c, [Operator.Plus, Operator.Modulos][int(rng.integers(0, 2))], lit_u64(int(rng.choice([3, 4097, 1 << 20]))))
        elif r > 0.9:
            e = binop(c, Operator.Lt, lit_i64(int(rng.choice([0, 100, 3000]))))
        else:
            op = [Operator.Plus, Operator.Minus, Operator.Multiply, Operator.Divide, Operator.Modulos][int(rng.integers(0, 5))]
            v = int(rng.choice([1, 2, 3, 7, 64, 1000]))
            if op in (Operator.Divide, Operator.Modulos) and rng.random() < 0.04:
                v = 0  # by design: DivideByZero wherever a valid row meets it
            e = binop(c, op, lit_i64(v))
        exprs.append(e)
        names.append(f"e{j}")
    return exprs, names


def random_aggregate(rng, fields):
    """-> (key or None, [(func, column)]): one to three numeric value columns with random function subsets, count over a Utf8 /
    Boolean column when there is one; key: none, an integer or Utf8 column, or Int64 column % m"""
    num = _cols_of(fields, DType.INT64, DType.FLOAT64, DType.UINT64)
    funcs = [A.Count, A.Sum, A.Avg, A.Min, A.Max]
    aggs = []
    if num:
        for c in rng.choice(num, size=min(len(num), int(rng.integers(1, 4))), replace=False):
            aggs += [(A(int(f)), int(c)) for f in rng.choice(funcs, size=int(rng.integers(1, 6)), replace=False)]
    other = _cols_of(fields, DType.UTF8, DType.BOOLEAN)
    if other and (not aggs or rng.random() < 0.5):
        aggs.append((A.Count, int(rng.choice(other))))
    keys = _cols_of(fields, DType.INT64, DType.UINT64, DType.UTF8)
    r = rng.random()
    if r < 0.4 or not keys:
        return None, aggs
    i = int(rng.choice(keys))
    if fields[i].dtype == DType.INT64 and r < 0.8:
        return binop(_ref(rng, fields, i), Operator.Modulos, lit_i64(int(rng.choice([3, 1000, 5000])))), aggs
    return _ref(rng, fields, i), aggs


def random_tables(rng):
    """host tables of a fuzz case: "a" (names id, k, ...) and "b" (names r_id, r_k, ...), 2-5 batches each with lengths from
    EDGES (at most one batch above 4097 rows), null fractions per batch; ids are unique within a batch and never NULL, so a join
    on them emits at most one row per (build batch, probe row)"""
    out = {}
    for name in ("a", "b"):
        nb = int(rng.integers(2, 6))
        lengths = [int(rng.choice(EDGES[:12])) for _ in range(nb)]
        if rng.random() < 0.5:
            lengths[int(rng.integers(0, nb))] = int(rng.choice(EDGES[12:]))
        if lengths[0] == 0 and rng.random() < 0.8:
            lengths[0] = 65  # a zero-row first batch empties every selection above it: kept rare
        out[name] = [make_batch(rng, n, float(rng.choice([0.0, 0.0, 0.1, 0.5])), nan_frac=float(rng.choice([0.0, 0.0, 0.02])), id_nulls=False)
                     for n in lengths]
    return out


FUZZ_FIELDS = {"a": schema(), "b": schema("r_")}


def _boundary(rng, lengths):
    """an offset / limit at a batch boundary of the input, one either side of it, a word further, or past the end"""
    total = sum(lengths)
    cuts = [0, total] + list(np.cumsum(lengths))
    return max(0, int(rng.choice(cuts)) + int(rng.choice([-65, -1, 0, 0, 1, 63, 64, 65, 5])))


class _Grower:
    """grows a tree bottom-up and keeps the oracle's result of what it has built so far, so that offsets and limits are drawn
    around the real batch boundaries and no operator is placed where the device path is documented not to go (an aggregate or a
    join build over an empty batch list)"""

    def __init__(self, rng, host):
        self.rng, self.host, self.error = rng, host, None

    def leaf(self, table):
        n = Node("scan", fields=FUZZ_FIELDS[table], table=table)
        return n, oracle_step(n, [], self.host)

    def push(self, node, handles):
        try:
            return node, oracle_step(node, handles, self.host)
        except ErrorCode as e:
            self.error = e.status
            return node, None

    def unary(self, cur, h, kinds, pred_only=None):
        rng = self.rng
        lengths = batch_lengths(h)
        kind = str(rng.choice(kinds))
        if not lengths and kind == "proj":
            kind = "sel"  # over no batches at all: the selection's own error (input[0]), by design
        if kind == "sel":
            pred = random_pred(rng, cur.fields, only=pred_only)
            if pred is None:
                kind = "lim"
            else:
                return self.push(Node("sel", [cur], cur.fields, pred=pred), [h])
        if kind == "proj":
            exprs, names = random_projection(rng, cur.fields)
            node, nh = self.push(Node("proj", [cur], None, exprs=exprs), [h])
            if nh is not None:
                node.fields = [Field(n, c.dtype, True) for n, c in zip(names, nh.to_python()[0])]
            else:
                node.fields = [Field(n, DType.INT64, True) for n in names]  # never resolved against: the tree ends here
            return node, nh
        return self.push(Node(kind, [cur], cur.fields, n=_boundary(rng, lengths)), [h])


def random_tree(seed):
    """-> (host tables, tree, status the oracle raised while the tree was grown or None).  Depth <= 4: Selection, Projection,
    Offset, Limit, at most one HashJoin (on id = r_id, below everything that renames columns), an optional Aggregate at the root"""
    rng = np.random.default_rng(seed)
    host = random_tables(rng)
    g = _Grower(rng, host)
    budget = int(rng.integers(1, 5))
    want_agg = budget >= 2 and rng.random() < 0.4
    if budget >= 2 and rng.random() < 0.4:
        sides = []
        for table, key in (("a", 0), ("b", 0)):
            cur, h = g.leaf(table)
            # below the join only tests of the never-NULL key: a NULL predicate row is a NULL key of value 0 on each side (Q4), and
            # those all match one another
            if rng.random() < 0.5 and budget >= 2 + int(want_agg):
                cur, h = g.unary(cur, h, ["sel", "off", "lim"], pred_only=[key])
            sides.append((cur, h))
        (lc, lh), (rc, rh) = sides
        if g.error is None and batch_lengths(lh):
            cur, h = g.push(Node("join", [lc, rc], lc.fields + rc.fields, lname="id", rname="r_id"), [lh, rh])
        else:
            cur, h = (lc, lh)
    else:
        cur, h = g.leaf("a")
    while g.error is None and cur.depth() < budget - int(want_agg):
        cur, h = g.unary(cur, h, ["sel", "proj", "off", "lim"])
    if g.error is None and want_agg and batch_lengths(h):
        key, aggs = random_aggregate(rng, cur.fields)
        if aggs:
            cur, h = g.push(Node("agg", [cur], None, key=key, aggs=aggs), [h])
    return host, cur, g.error
