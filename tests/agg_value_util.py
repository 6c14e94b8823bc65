"""An independent model of the aggregate functions' numerics (quirk Q10: every Int64 / UInt64 value is converted to f64 first and
accumulated in f64), the value-domain generators the value-domain suites share, and a comparator of a result batch against the
model.  Plain numpy and Python; nothing here calls the oracle.

The model (a second reading of the reference's sum.rs, avg.rs, min.rs, max.rs, count.rs):
  conversion  int64 / uint64 -> float64 by `astype`: round to nearest even, as v_cvt_f64 / cvtsi2sd do
  count       the number of valid rows of the group, UInt64
  sum         finite rows: math.fsum of the converted values — the correctly rounded exact sum; NaN if any value is NaN or both
              infinities occur, the infinity itself if only one sign occurs; 0.0 for a group without valid rows
  avg         sum / float(uint32(count)): NaN for a group without valid rows
  min         starts at f64::MAX and ignores NaN (so a group of nothing but +inf keeps f64::MAX)
  max         starts at f64::MIN and becomes NaN if any value is NaN (so a group of nothing but -inf keeps f64::MIN)
  keys        rows with a NULL key are dropped; the result has no key column and its rows are in no particular order

The comparator (assert_matches_model) asks, row by row after aligning both sides on their exact columns:
  count       equal
  min, max    equal bit for bit; every NaN equals every NaN; +0.0 equals -0.0 (OrderedFloat makes them equal: which one survives
              depends on the order of the rows)
  sum         both NaN, or the same infinity; otherwise |got - exact| <= n_g * 2^-52 * sum|x_i| over the group's finite converted
              values — twice the first-order worst-case bound (n - 1) * 2^-53 * sum|x| of recursive summation in ANY order, so it holds
              for whatever tree a kernel adds in.  Derived, not measured.
  avg         the same bound divided by the count, plus one ulp of the quotient
There is no relative tolerance anywhere for count, min or max."""
import math

import numpy as np

from naive_query_engine_amd import AggregateFunc

F64_MAX = float(np.finfo(np.float64).max)
I64_MIN, I64_MAX = int(np.iinfo(np.int64).min), int(np.iinfo(np.int64).max)
NULL_FRAC = 0.10
DOMAINS = ["i64_wide", "i64_same_sign", "u64_high", "f64_special"]
VARIANTS = [(d, nullable) for d in DOMAINS for nullable in (False, True)]
VARIANT_IDS = [d + ("_nullable" if nullable else "") for d, nullable in VARIANTS]
SPECIALS = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 5e-324, -5e-324, 2.2250738585072014e-308, -2.2250738585072014e-308, 1e300, -1e300])
ALL_AGGS = lambda c: [(AggregateFunc.Count, c), (AggregateFunc.Sum, c), (AggregateFunc.Avg, c), (AggregateFunc.Min, c), (AggregateFunc.Max, c)]


# --------------------------------------------------------------------------- generators
def gen_values(domain, rng, n, nullable):
    """(values, validity mask or None) of one value column of `n` rows.  The planted values sit at random rows and are valid."""
    if domain == "i64_wide":
        v = rng.integers(I64_MIN, I64_MAX, n, dtype=np.int64, endpoint=True)
        plant = np.array([I64_MIN, I64_MAX, (1 << 53) + 1, -((1 << 53) + 1), 0, -1], dtype=np.int64)
    elif domain == "i64_same_sign":      # a few rows already exceed 2^63 in f64: integer registers would wrap where f64 does not
        v = rng.integers(1 << 61, 1 << 62, n, dtype=np.int64)
        plant = np.array([1 << 61, (1 << 62) - 1], dtype=np.int64)
    elif domain == "u64_high":           # a conversion through a signed path turns every one of these negative
        v = rng.integers(1 << 63, (1 << 64) - 1, n, dtype=np.uint64, endpoint=True)
        plant = np.array([1 << 63, (1 << 63) + 1, (1 << 64) - 1, (1 << 64) - 1025, (1 << 53) + 1], dtype=np.uint64)
    elif domain == "f64_special":        # (sum|x| stays below 1e307 per group while fewer than 10^7 rows hold +-1e300: no order of summation overflows)
        v = rng.random(n) * 200.0 - 100.0
        where = rng.random(n) < 0.02
        v[where] = SPECIALS[rng.integers(0, len(SPECIALS), int(where.sum()))]
        plant = SPECIALS
    else:
        raise ValueError(domain)
    mask = (rng.random(n) >= NULL_FRAC) if nullable else None
    if n >= 4 * len(plant):
        at = rng.choice(n, len(plant), replace=False)
        v[at] = plant
        if mask is not None:
            mask[at] = True
    return v, mask


def plant_only_groups(v, mask, key, pinf_key, ninf_key, nan_key, null_key):
    """Float64 "special": the groups of `pinf_key`, `ninf_key`, `nan_key` hold nothing but +inf, -inf, NaN; the group of `null_key` nothing
    but NULL (a nullable column only: without a validity bitmap there is no NULL, and that group stays as it was)"""
    v[key == pinf_key] = np.inf
    v[key == ninf_key] = -np.inf
    v[key == nan_key] = np.nan
    if mask is not None:
        mask[key == null_key] = False


def interior_keys(key, keep=None):
    """four distinct group keys from the middle of the key range (never its smallest or largest): the "only" groups then land in an
    interior partition of the partitioned tiers.  Fewer than six groups: whatever there is, cycled."""
    u = np.unique(key if keep is None else key[keep])
    if len(u) >= 6:
        mid = len(u) // 2
        return [u[mid - 1], u[mid], u[mid + 1], u[mid + 2]]
    return [u[(1 + i) % len(u)] for i in range(4)]


# --------------------------------------------------------------------------- the model
class ModelResult:
    def __init__(self, funcs, cols, tols):
        self.funcs, self.cols, self.tols = funcs, cols, tols   # per output column: AggregateFunc, values, absolute bound (sum / avg) or None
        self.rows = len(cols[0]) if cols else 0


def _column_state(v, mask, rows, gid, G):
    """count, exact sum, min, max, the sum's bound — per group — of one value column over the rows `rows` (group of row i: gid[i])"""
    x = v[rows].astype(np.float64)
    g = gid
    if mask is not None:
        ok = mask[rows]
        x, g = x[ok], g[ok]
    order = np.argsort(g, kind="stable")          # rows by group, once
    xs, gs = x[order], g[order]
    count = np.bincount(gs, minlength=G).astype(np.uint64)
    total = np.zeros(G)
    bound = np.zeros(G)
    mn = np.full(G, F64_MAX)
    mx = np.full(G, -F64_MAX)
    if len(xs):
        present, starts = np.unique(gs, return_index=True)
        isnan = np.isnan(xs)
        mn[present] = np.minimum(F64_MAX, np.minimum.reduceat(np.where(isnan, np.inf, xs), starts))
        m = np.maximum(-F64_MAX, np.maximum.reduceat(np.where(isnan, -np.inf, xs), starts))
        any_nan = np.add.reduceat(isnan.astype(np.int64), starts) > 0
        mx[present] = np.where(any_nan, np.nan, m)
        any_pinf = np.add.reduceat((xs == np.inf).astype(np.int64), starts) > 0
        any_ninf = np.add.reduceat((xs == -np.inf).astype(np.int64), starts) > 0
        fin = np.isfinite(xs)
        xf, gf = xs[fin], gs[fin]
        exact = np.zeros(G)
        nfin = np.bincount(gf, minlength=G)
        if len(xf):
            pf, sf = np.unique(gf, return_index=True)
            cf = nfin[pf]
            one, two = cf == 1, cf == 2
            exact[pf[one]] = xf[sf[one]]
            exact[pf[two]] = xf[sf[two]] + xf[sf[two] + 1]     # one addition is correctly rounded: the exact sum of two
            many = np.nonzero(cf >= 3)[0]
            if len(many):
                lst = xf.tolist()
                exact[pf[many]] = [math.fsum(lst[s:s + c]) for s, c in zip(sf[many].tolist(), cf[many].tolist())]
            bound[pf] = nfin[pf] * 2.0 ** -52 * np.add.reduceat(np.abs(xf), sf)
        t = exact[present]
        t = np.where(any_pinf, np.inf, t)
        t = np.where(any_ninf, -np.inf, t)
        t = np.where(any_nan | (any_pinf & any_ninf), np.nan, t)
        total[present] = t
        bound[~np.isfinite(total)] = 0.0
    return count, total, mn, mx, bound


def model_aggregate(columns, aggs, key=None, key_mask=None, keep=None):
    """columns: [(values, mask or None)] — the whole table, indexed as the aggregates index it; key: the group key of every row
    (an integer array, computed by the caller from the key expression) or None for the un-grouped form; keep: the rows the
    predicate passes (None: all)."""
    n = len(columns[0][0])
    rows = np.ones(n, dtype=bool) if keep is None else keep.copy()
    if key is not None:
        if key_mask is not None:
            rows &= key_mask
        _, gid = np.unique(key[rows], return_inverse=True)
        gid = gid.reshape(-1)
        G = int(gid.max()) + 1 if len(gid) else 0
    else:
        gid = np.zeros(int(rows.sum()), dtype=np.int64)
        G = 1
    states = {}
    funcs, cols, tols = [], [], []
    for fn, c in aggs:
        if c not in states:
            states[c] = _column_state(columns[c][0], columns[c][1], rows, gid, G)
        count, total, mn, mx, bound = states[c]
        funcs.append(fn)
        if fn == AggregateFunc.Count:
            cols.append(count), tols.append(None)
        elif fn == AggregateFunc.Sum:
            cols.append(total), tols.append(bound)
        elif fn == AggregateFunc.Avg:
            with np.errstate(invalid="ignore", divide="ignore"):
                d = count.astype(np.uint32).astype(np.float64)
                avg = total / d
                tol = np.where(np.isfinite(avg), bound / np.maximum(d, 1.0) + np.spacing(np.abs(np.where(np.isfinite(avg), avg, 0.0))), 0.0)
            cols.append(avg), tols.append(tol)
        elif fn == AggregateFunc.Min:
            cols.append(mn), tols.append(None)
        elif fn == AggregateFunc.Max:
            cols.append(mx), tols.append(None)
        else:
            raise ValueError(fn)
    return ModelResult(funcs, cols, tols)


# --------------------------------------------------------------------------- the comparator
_NAN_KEY = np.uint64(0xFFFFFFFFFFFFFFFF)


def _order_key(x, fold_zero):
    """float64 -> uint64 whose unsigned order is the total order of the bit patterns; NaN canonical and last; (min / max) -0.0 as +0.0"""
    x = np.ascontiguousarray(x, dtype=np.float64)
    if fold_zero:
        x = np.where(x == 0.0, 0.0, x)
    b = x.view(np.uint64)
    k = np.where((b >> np.uint64(63)) != 0, ~b, b | np.uint64(1 << 63))
    return np.where(np.isnan(x), _NAN_KEY, k)


def _aligned(funcs, cols):
    """row order by (count, min, max, …) — the exact columns first — then sum and avg"""
    exact = [i for i, f in enumerate(funcs) if f in (AggregateFunc.Count, AggregateFunc.Min, AggregateFunc.Max)]
    rest = [i for i, f in enumerate(funcs) if i not in exact]
    exact.sort(key=lambda i: (0 if funcs[i] == AggregateFunc.Count else 1, i))
    keys = []
    for i in exact + rest:
        keys.append(cols[i].astype(np.uint64) if funcs[i] == AggregateFunc.Count else _order_key(cols[i], funcs[i] in (AggregateFunc.Min, AggregateFunc.Max)))
    return np.lexsort(keys[::-1]) if keys else np.zeros(0, dtype=np.int64)


def assert_matches_model(got_cols, model, what=""):
    """got_cols: the Columns of one result batch (device or oracle); model: the ModelResult of the same query"""
    from naive_query_engine_amd import DType

    assert len(got_cols) == len(model.funcs), f"{what}: {len(got_cols)} columns, the query has {len(model.funcs)} aggregates"
    got = []
    for i, (c, fn) in enumerate(zip(got_cols, model.funcs)):
        want = DType.UINT64 if fn == AggregateFunc.Count else DType.FLOAT64
        assert c.dtype == want, f"{what}: column {i} is {c.dtype}, expected {want}"
        assert c.valid_mask().all(), f"{what}: column {i} has NULLs"
        got.append(c.to_numpy())
        assert len(got[-1]) == model.rows, f"{what}: {len(got[-1])} rows, the model has {model.rows} groups"
    go, mo = _aligned(model.funcs, got), _aligned(model.funcs, model.cols)
    count_cols = [i for i, fn in enumerate(model.funcs) if fn == AggregateFunc.Count]
    counts = model.cols[count_cols[0]][mo] if count_cols else None   # (for the failure message)
    for i, fn in enumerate(model.funcs):
        g, e = got[i][go], model.cols[i][mo]
        if fn == AggregateFunc.Count:
            same = g == e
        elif fn in (AggregateFunc.Min, AggregateFunc.Max):
            same = (g.view(np.uint64) == e.view(np.uint64)) | (np.isnan(g) & np.isnan(e)) | ((g == 0.0) & (e == 0.0))
        else:
            tol = model.tols[i][mo]
            with np.errstate(invalid="ignore"):
                close = np.isfinite(g) & np.isfinite(e) & (np.abs(g - e) <= tol)
            same = (np.isnan(g) & np.isnan(e)) | (np.isinf(g) & np.isinf(e) & (g == e)) | close
        if not same.all():
            bad = np.nonzero(~same)[0]
            tol = model.tols[i][mo] if model.tols[i] is not None else None
            rows = []
            for j in bad[:4]:
                row = f"row {j}: got {g[j]!r} model {e[j]!r}"
                if tol is not None:
                    row += f" bound {tol[j]!r}"
                if counts is not None:
                    row += f" (count {counts[j]})"
                rows.append(row)
            raise AssertionError(f"{what}: aggregate {i} ({fn.name}) differs from the model in {len(bad)} of {len(g)} groups: {'; '.join(rows)}")
