"""The yardstick of the window-function tests (quirk Q23): a row-at-a-time Python model and a comparator.  Nothing here touches the
device or the library.

The window of one call (all its functions share it):
  sorted order   order_by_util.sort_indices by (the partition keys with default options, then the order keys as given): stable
  partition      rows whose order_by_util.row_keys tie on every partition key (the sort's own ties: -0.0 = +0.0, every NaN equals
                 every NaN, NULL equals NULL and differs from every value)
  peers          rows of one partition that also tie on every order key
  frame          PARTITION: every row of the partition; ROWS: the partition's rows up to the row itself in sorted order; RANGE: up
                 to the row's LAST peer
The functions:
  row_number     1 + the partition rows before the row          rank   1 + the partition rows before the row's first peer
  dense_rank     the peer groups up to and including the row's own
  count / sum / avg / min / max   agg_value_util's definitions (quirk Q10) over the frame's rows: the model walks every partition once
                 and keeps the state of agg_value_util._column_state incrementally (valid count, the EXACT sum of the finite values as
                 Shewchuk partials, NaN / +inf / -inf seen, min ignoring NaN, max, the bound n_frame * 2^-52 * sum|x| over the frame's
                 finite values — derived, not measured); frame_states_by_groups states the same through _column_state itself, every
                 frame one group, and tests/test_window_model.py holds the two against each other
The comparator (assert_matches_window): ranking, count, min, max equal (every NaN equals every NaN, +0.0 equals -0.0 for min / max);
sum and avg within the bound (avg: the bound over the count plus one ulp of the quotient).  No case is left out and there is no
relative tolerance.

window_np is the same model in whole-array numpy steps, for the tables of 10^6 rows of tests/test_gpu_window_sizes.py (a narrower value
domain, on which every sum is exact); layout_lengths / layout_table build those tables.  tests/test_large_models_host.py holds window_np
against window."""
import math

import numpy as np

import agg_value_util as avu
import order_by_util as obu
from naive_query_engine_amd import Column, DType, WindowFrame, WindowFunc

RANKING = (WindowFunc.RowNumber, WindowFunc.Rank, WindowFunc.DenseRank)
AGGREGATES = (WindowFunc.Count, WindowFunc.Sum, WindowFunc.Min, WindowFunc.Max, WindowFunc.Avg)
FRAMES = (WindowFrame.Partition, WindowFrame.Rows, WindowFrame.Range)
ALL_AGGS = lambda c, frame: [(f, c, frame) for f in AGGREGATES]


def normalise_funcs(funcs):
    out = []
    for f in funcs:
        f = (f,) if isinstance(f, int) else tuple(f)
        f = (f + (None, None))[:3]
        out.append((WindowFunc(f[0]), f[1], WindowFrame.Range if f[2] is None else WindowFrame(f[2])))
    return out


# ----------------------------------------------------------------------------- the window's structure
class Layout:
    """the sorted order and, per sorted position, the first / last position of its partition and of its peer group"""

    def __init__(self, cols, partition_by, order_by):
        n = cols[0].length if cols else 0
        keys = [(int(c), False, True) for c in partition_by] + obu.normalise_keys(order_by)
        self.n = n
        self.order = obu.sort_indices(cols, keys) if keys else list(range(n))
        rk = obu.row_keys(cols, keys) if keys else [()] * n
        npart = len(partition_by)
        self.part_first, self.peer_first, self.part_last, self.peer_last, self.dense = [0] * n, [0] * n, [0] * n, [0] * n, [0] * n
        for i in range(n):
            if i == 0 or rk[self.order[i]][:npart] != rk[self.order[i - 1]][:npart]:
                self.part_first[i], self.peer_first[i], self.dense[i] = i, i, 1
            elif rk[self.order[i]] != rk[self.order[i - 1]]:
                self.part_first[i], self.peer_first[i], self.dense[i] = self.part_first[i - 1], i, self.dense[i - 1] + 1
            else:
                self.part_first[i], self.peer_first[i], self.dense[i] = self.part_first[i - 1], self.peer_first[i - 1], self.dense[i - 1]
        for i in range(n - 1, -1, -1):
            last = i == n - 1
            self.part_last[i] = i if last or self.part_first[i + 1] == i + 1 else self.part_last[i + 1]
            self.peer_last[i] = i if last or self.peer_first[i + 1] == i + 1 else self.peer_last[i + 1]

    def frame_end(self, i, frame):
        return i if frame == WindowFrame.Rows else self.peer_last[i] if frame == WindowFrame.Range else self.part_last[i]


# ----------------------------------------------------------------------------- Q10's state, row at a time
class _Running:
    def __init__(self):
        self.count, self.nfin, self.abs_sum = 0, 0, 0.0
        self.partials = []
        self.nan = self.pinf = self.ninf = False
        self.mn, self.mx = avu.F64_MAX, -avu.F64_MAX

    def add(self, x):
        """one VALID row's value, already converted to f64"""
        self.count += 1
        if math.isnan(x):
            self.nan = True
            return
        self.mn, self.mx = min(self.mn, x), max(self.mx, x)
        if math.isinf(x):
            if x > 0:
                self.pinf = True
            else:
                self.ninf = True
            return
        self.nfin += 1
        self.abs_sum += abs(x)
        i = 0
        for y in self.partials:     # Shewchuk: the partials stay an exact, non-overlapping expansion of the sum
            if abs(x) < abs(y):
                x, y = y, x
            hi = x + y
            lo = y - (hi - x)
            if lo:
                self.partials[i] = lo
                i += 1
            x = hi
        self.partials[i:] = [x]

    def state(self):
        """(count, sum, min, max, the sum's bound)"""
        if self.nan or (self.pinf and self.ninf):
            total = math.nan
        elif self.pinf or self.ninf:
            total = math.inf if self.pinf else -math.inf
        else:
            total = math.fsum(self.partials)
        bound = self.nfin * 2.0 ** -52 * self.abs_sum if math.isfinite(total) else 0.0
        return self.count, total, self.mn, (math.nan if self.nan else self.mx), bound


def position_states(col, lay):
    """per sorted position: the state over the partition's rows up to and including it (the ROWS frame's state)"""
    v = col.to_numpy().astype(np.float64).tolist()
    ok = col.valid_mask().tolist()
    out, run = [], None
    for i in range(lay.n):
        if lay.part_first[i] == i:
            run = _Running()
        r = lay.order[i]
        if ok[r]:
            run.add(v[r])
        out.append(run.state())
    return out


def frame_states_by_groups(col, lay, frame):
    """the same states through agg_value_util._column_state: every position's frame is one group (quadratic: small tables only)"""
    rows, gid = [], []
    for i in range(lay.n):
        for p in range(lay.part_first[i], lay.frame_end(i, frame) + 1):
            rows.append(lay.order[p])
            gid.append(i)
    count, total, mn, mx, bound = avu._column_state(col.to_numpy(), col.valid_mask() if col.validity is not None else None, np.array(rows, dtype=np.int64),
                                                    np.array(gid, dtype=np.int64), lay.n)
    return [(int(count[i]), float(total[i]), float(mn[i]), float(mx[i]), float(bound[i])) for i in range(lay.n)]


# ----------------------------------------------------------------------------- the model
class ModelWindow:
    def __init__(self, funcs, cols, tols):
        self.funcs, self.cols, self.tols = funcs, cols, tols   # per function: (func, column, frame), values in INPUT order, bound or None


def window(cols, partition_by, order_by, funcs):
    funcs = normalise_funcs(funcs)
    lay = Layout(cols, partition_by, order_by)
    n = lay.n
    states = {}
    out_cols, out_tols = [], []
    rows = np.array(lay.order, dtype=np.int64)
    for fn, c, frame in funcs:
        tol = None
        if fn in RANKING:
            first = np.array(lay.part_first, dtype=np.int64)
            sorted_vals = {WindowFunc.RowNumber: np.arange(n, dtype=np.int64) - first + 1, WindowFunc.Rank: np.array(lay.peer_first, dtype=np.int64) - first + 1,
                           WindowFunc.DenseRank: np.array(lay.dense, dtype=np.int64)}[fn].astype(np.uint64)
        else:
            assert cols[c].dtype in (DType.INT64, DType.UINT64, DType.FLOAT64)
            if c not in states:
                states[c] = position_states(cols[c], lay)
            st = [states[c][lay.frame_end(i, frame)] for i in range(n)]
            if fn == WindowFunc.Count:
                sorted_vals = np.array([s[0] for s in st], dtype=np.uint64)
            elif fn == WindowFunc.Min:
                sorted_vals = np.array([s[2] for s in st], dtype=np.float64)
            elif fn == WindowFunc.Max:
                sorted_vals = np.array([s[3] for s in st], dtype=np.float64)
            else:
                sorted_vals = np.array([s[1] for s in st], dtype=np.float64)
                sorted_tol = np.array([s[4] for s in st], dtype=np.float64)
                if fn == WindowFunc.Avg:
                    d = np.array([s[0] for s in st], dtype=np.uint64).astype(np.uint32).astype(np.float64)
                    with np.errstate(invalid="ignore", divide="ignore"):
                        sorted_vals = sorted_vals / d
                        fin = np.isfinite(sorted_vals)
                        sorted_tol = np.where(fin, sorted_tol / np.maximum(d, 1.0) + np.spacing(np.abs(np.where(fin, sorted_vals, 0.0))), 0.0)
                tol = np.zeros(n, dtype=np.float64)
                tol[rows] = sorted_tol
        vals = np.zeros(n, dtype=sorted_vals.dtype)
        vals[rows] = sorted_vals
        out_cols.append(vals)
        out_tols.append(tol)
    return ModelWindow(funcs, out_cols, out_tols)


# ----------------------------------------------------------------------------- the same model, vectorised
NP_VALUE_LIMIT = 2 ** 20   # window_np: finite values are integers of smaller magnitude
_INF_KEY = NP_VALUE_LIMIT + 1   # +inf / -inf as integers beyond every finite value
_NONE_KEY = NP_VALUE_LIMIT + 2  # "no value yet": the start values F64_MAX (min) and -F64_MAX (max)
_BIG = 4 * _NONE_KEY           # more than the distance between any two keys: the offset between two partitions


def _since_partition_start(x, part_first):
    """per position: the sum of x over its partition's positions up to and including it (int64: exact)"""
    c = np.cumsum(x, dtype=np.int64)
    return c - (c[part_first] - x[part_first])


def _running_extreme(key, pidx, largest, partition_offset=True):
    """per position: the smallest (largest) key of its partition up to and including it.  Partition p's keys are moved by p * _BIG away
    from those of every earlier partition, in the direction the accumulation prefers, so one pass over the table never carries a value
    across a partition start.  (partition_offset=False is the WRONG variant tests/test_large_models_host.py must tell apart.)"""
    off = pidx * _BIG if partition_offset else np.zeros_like(pidx)
    return np.maximum.accumulate(key + off) - off if largest else np.minimum.accumulate(key - off) + off


def _key_to_f64(k):
    out = k.astype(np.float64)
    out[k == _INF_KEY], out[k == -_INF_KEY] = np.inf, -np.inf
    out[k == _NONE_KEY], out[k == -_NONE_KEY] = avu.F64_MAX, -avu.F64_MAX
    return out


def window_np(cols, partition_by, order_by, funcs, _partition_offset=True):
    """`window` in whole-array numpy steps, fast enough for 10^6 rows.  Defined for value columns whose finite values are integers of
    magnitude < 2^20 (Int64, or Float64 with +-inf, NaN anywhere), NULLs anywhere, fewer than 2^32 rows.  Every frame's sum is then an
    integer below 2^53: every order of the additions gives it exactly, so the bound of sum is 0 and avg's one ulp of the quotient.
    tests/test_large_models_host.py holds it against `window`."""
    funcs = normalise_funcs(funcs)
    n = cols[0].length if cols else 0
    keys = [(int(c), False, True) for c in partition_by] + obu.normalise_keys(order_by)
    order = obu.sort_indices_np(cols, keys)
    idx = np.arange(n, dtype=np.int64)
    # starts: a sorted position whose row differs from the row before it on a partition key (on any key: a peer start)
    part_start, peer_start = idx == 0, idx == 0
    for k, arrs in enumerate(obu.key_arrays(cols, keys)):
        for a in arrs:
            s = a[order]
            differs = np.concatenate([[True], s[1:] != s[:-1]]) if n else np.zeros(0, dtype=bool)
            peer_start = peer_start | differs
            if k < len(partition_by):
                part_start = part_start | differs
    part_first = np.maximum.accumulate(np.where(part_start, idx, 0))
    peer_first = np.maximum.accumulate(np.where(peer_start, idx, 0))
    # the mirror: the nearest start AFTER a position, less one; none: the last position
    nearest = lambda start: np.minimum.accumulate(np.where(start, idx, n)[::-1])[::-1]
    part_last = np.concatenate([nearest(part_start)[1:], [n]])[:n] - 1
    peer_last = np.concatenate([nearest(peer_start)[1:], [n]])[:n] - 1
    dense = np.cumsum(peer_start, dtype=np.int64)
    pidx = np.cumsum(part_start, dtype=np.int64) - 1
    ends = {WindowFrame.Rows: idx, WindowFrame.Range: peer_last, WindowFrame.Partition: part_last}

    states = {}

    def state(c):
        """per sorted position, over its partition's rows up to and including it: count, sum, min, max"""
        if c not in states:
            assert cols[c].dtype in (DType.INT64, DType.UINT64, DType.FLOAT64)
            x = cols[c].to_numpy().astype(np.float64)[order]
            ok = cols[c].valid_mask()[order]
            nan, fin = ok & np.isnan(x), ok & np.isfinite(x)
            if not ((np.abs(x[fin]) < NP_VALUE_LIMIT).all() and (x[fin] == np.round(x[fin])).all()):
                raise ValueError("window_np: a finite value is no integer of magnitude < 2^20; use window")
            v = np.where(fin, x, 0.0).astype(np.int64)
            since = lambda a: _since_partition_start(a.astype(np.int64), part_first)
            count, total = since(ok), since(v).astype(np.float64)
            any_nan, pinf, ninf = since(nan) > 0, since(ok & (x == np.inf)) > 0, since(ok & (x == -np.inf)) > 0
            total = np.where(any_nan | (pinf & ninf), np.nan, np.where(pinf, np.inf, np.where(ninf, -np.inf, total)))
            key = np.where(x == np.inf, _INF_KEY, np.where(x == -np.inf, -_INF_KEY, v))
            # (Q10: min starts at F64_MAX and max at -F64_MAX, so +inf never shows in a min nor -inf in a max)
            mn = _key_to_f64(_running_extreme(np.where(ok & ~nan & (x != np.inf), key, _NONE_KEY), pidx, False, _partition_offset))  # min skips a NaN
            mx = _key_to_f64(_running_extreme(np.where(ok & ~nan & (x != -np.inf), key, -_NONE_KEY), pidx, True, _partition_offset))
            states[c] = count, total, mn, np.where(any_nan, np.nan, mx)                                              # max keeps it
        return states[c]

    out_cols, out_tols = [], []
    for fn, c, frame in funcs:
        tol = None
        if fn in RANKING:
            sorted_vals = {WindowFunc.RowNumber: idx - part_first + 1, WindowFunc.Rank: peer_first - part_first + 1,
                           WindowFunc.DenseRank: dense - dense[part_first] + 1}[fn].astype(np.uint64)
        else:
            count, total, mn, mx = (a[ends[frame]] for a in state(c))
            if fn == WindowFunc.Count:
                sorted_vals = count.astype(np.uint64)
            elif fn == WindowFunc.Min:
                sorted_vals = mn
            elif fn == WindowFunc.Max:
                sorted_vals = mx
            else:
                sorted_vals, sorted_tol = total, np.zeros(n, dtype=np.float64)
                if fn == WindowFunc.Avg:
                    with np.errstate(invalid="ignore", divide="ignore"):
                        sorted_vals = total / count.astype(np.float64)
                        fin = np.isfinite(sorted_vals)
                        sorted_tol = np.where(fin, np.spacing(np.abs(np.where(fin, sorted_vals, 0.0))), 0.0)
                tol = np.zeros(n, dtype=np.float64)
                tol[order] = sorted_tol
        vals = np.zeros(n, dtype=sorted_vals.dtype)
        vals[order] = sorted_vals
        out_cols.append(vals)
        out_tols.append(tol)
    return ModelWindow(funcs, out_cols, out_tols)


# ----------------------------------------------------------------------------- partition layouts by explicit lengths
LAYOUTS = ("one_partition", "tile_edges", "flagless_chunk", "every_row_its_own", "random_lengths")


def layout_lengths(name, n, tile, chunk, rng=None, inside=5000, longest=10_000):
    """the partition lengths of one layout over n rows, in built order.  `tile`: the rows of one scan tile; `chunk`: the rows of the
    tiles ONE trip of the carry scans covers.
      one_partition      the running state crosses every tile and chunk
      tile_edges         a start on the last row of the tile in front of the first chunk edge and one on the first row behind it
                         (fewer rows than a chunk: at the edge of the middle tile)
      flagless_chunk     one partition from `inside` rows in front of the first chunk edge to the middle of what lies behind the second:
                         the chunk between holds no start at all (no more than two chunks of rows: the same over thirds of the tiles)
      every_row_its_own  n partitions
      random_lengths     seeded lengths between 1 and `longest`"""
    if n == 0:
        return []
    tiles = (n + tile - 1) // tile
    if name == "one_partition":
        lengths = [n]
    elif name == "tile_edges":
        edge = chunk if n >= chunk else max(1, tiles // 2) * tile
        lengths = [edge - 1, 1, n]
    elif name == "flagless_chunk":
        c = chunk if n > 2 * chunk else max(1, tiles // 3) * tile
        a, tail = min(inside, max(1, c // 4)), max(0, n - 2 * c)
        lengths = [c - a, a + c + tail // 2, max(1, (tail - tail // 2) // 2), n]
    elif name == "every_row_its_own":
        return [1] * n
    else:
        assert name == "random_lengths"
        lengths = rng.integers(1, longest, n // max(1, longest // 2) + 8, endpoint=True).tolist() + [n]
    out, left = [], n   # cut the list off at n rows
    for length in lengths:
        length = min(int(length), left)
        if length > 0:
            out.append(length)
            left -= length
    assert sum(out) == n
    return out


def layout_table(lengths, rng, peers_of_three, poisoned=None):
    """(columns in built order, partition keys, order keys): column 0 the partition number, column 1 the order key — the built position,
    so the sorted order is the built order, or a third of it: peer groups of three that straddle whatever edge the lengths straddle —,
    column 2 Int64 in (-2^20, 2^20) with about 10 % NULLs, column 3 Float64 with integer values of that range.  In the partition
    `poisoned` every third row of column 3 is +inf, -inf or NaN in turn (the cancellation trap: "the prefix at the row minus the prefix
    at the partition's start" gives NaN for every later partition)."""
    n = int(np.sum(lengths)) if len(lengths) else 0
    part = np.repeat(np.arange(len(lengths), dtype=np.int64), lengths)
    pos = np.arange(n, dtype=np.int64)
    v = rng.integers(-NP_VALUE_LIMIT + 1, NP_VALUE_LIMIT, n).astype(np.int64)
    x = rng.integers(-NP_VALUE_LIMIT + 1, NP_VALUE_LIMIT, n).astype(np.float64)
    if poisoned is not None and n:
        rows = np.nonzero(part == poisoned)[0]
        x[rows[::9]], x[rows[3::9]], x[rows[6::9]] = np.inf, -np.inf, np.nan
    cols = [Column.from_numpy(part), Column.from_numpy(pos // 3 if peers_of_three else pos), Column.from_numpy(v, rng.random(n) > 0.1), Column.from_numpy(x)]
    return cols, [0], [1]


def split_model(model, lo, hi):
    """the ModelWindow of functions [lo, hi) of a call (one call takes at most 16 functions; the model is computed once)"""
    return ModelWindow(model.funcs[lo:hi], model.cols[lo:hi], model.tols[lo:hi])


# ----------------------------------------------------------------------------- the comparator
def same_mask(fn, g, e, tol):
    """per row: does the value `g` agree with the model's `e` for function fn"""
    if fn in RANKING or fn == WindowFunc.Count:
        return g == e
    if fn in (WindowFunc.Min, WindowFunc.Max):
        return (g.view(np.uint64) == e.view(np.uint64)) | (np.isnan(g) & np.isnan(e)) | ((g == 0.0) & (e == 0.0))
    with np.errstate(invalid="ignore"):
        close = np.isfinite(g) & np.isfinite(e) & (np.abs(g - e) <= tol)
    return (np.isnan(g) & np.isnan(e)) | (np.isinf(g) & np.isinf(e) & (g == e)) | close


def assert_matches_window(got_cols, model, what=""):
    """got_cols: the Columns of the operator's result table; model: the ModelWindow of the same call"""
    assert len(got_cols) == len(model.funcs), f"{what}: {len(got_cols)} columns, the call has {len(model.funcs)} functions"
    for i, (c, (fn, col, frame)) in enumerate(zip(got_cols, model.funcs)):
        want = DType.UINT64 if fn in RANKING or fn == WindowFunc.Count else DType.FLOAT64
        w = f"{what}: function {i} ({fn.name}, column {col}, {frame.name})"
        assert c.dtype == want, f"{w} is {c.dtype}, expected {want}"
        assert c.validity is None or c.valid_mask().all(), f"{w} has NULLs"
        g, e = c.to_numpy(), model.cols[i]
        assert len(g) == len(e), f"{w}: {len(g)} rows, the model has {len(e)}"
        same = same_mask(fn, g, e, model.tols[i])
        if not same.all():
            bad = np.nonzero(~same)[0]
            rows = [f"row {j}: got {g[j]!r} model {e[j]!r}" + (f" bound {model.tols[i][j]!r}" if model.tols[i] is not None else "") for j in bad[:4]]
            raise AssertionError(f"{w} differs from the model in {len(bad)} of {len(g)} rows: {'; '.join(rows)}")
