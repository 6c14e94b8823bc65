"""The yardstick of the semi / anti hash join tests (quirk Q22): a numpy / dict model on top of outer_join_util.  Nothing here touches
the device or the library.

Match relation: the hash join's, Q11 included, at every key position — left = build side, right = probe side, key validity IGNORED
(the raw 8-byte slot of an Int64 / UInt64 key, also under a NULL; the bytes between the offsets of a Utf8 key).  With `null_unmatched`
(NQE_SEMI_NULL_KEY_UNMATCHED) a PROBE row with a NULL at any key position matches nothing.
  probe SEMI / ANTI: the probe rows that have at least one match / have none, each once, ascending
  build SEMI / ANTI: the build rows that matched in some probe batch / in none, ascending
An output column is the compaction of its source: values of the valid rows bit for bit, validity preserved, a bitmap iff the source has
NULLs (an uploaded column keeps its bitmap only then)."""
import numpy as np

import outer_join_util as oju
from naive_query_engine_amd import Column, DType

I64 = np.iinfo(np.int64)


def i64(a):
    return Column.from_numpy(np.asarray(a, dtype=np.int64))


# ----------------------------------------------------------------------------- the model
def _as_tuple(keys):
    return [keys] if isinstance(keys, Column) else list(keys)


def tuple_slots(keys):
    """what the join compares, per row: the tuple of raw key slots"""
    return list(zip(*[oju.key_slots(c) for c in _as_tuple(keys)]))


def _probe_valid(keys, null_unmatched):
    cols = _as_tuple(keys)
    ok = np.ones(cols[0].length, dtype=bool)
    if null_unmatched:
        for c in cols:
            ok &= c.valid_mask()
    return ok


def semi_rows(build_keys, probe_keys, anti=False, null_unmatched=False):
    """the probe rows kept, ascending"""
    have = set(tuple_slots(build_keys))
    ok = _probe_valid(probe_keys, null_unmatched)
    hit = np.array([bool(v) and (k in have) for k, v in zip(tuple_slots(probe_keys), ok.tolist())], dtype=bool)
    return np.nonzero(~hit if anti else hit)[0].tolist()


def marked_mask(build_keys, probe_batches, null_unmatched=False):
    """bool per build row: matched in some probe batch (`probe_batches`: one key column or key tuple per batch)"""
    pos = {}
    for r, k in enumerate(tuple_slots(build_keys)):
        pos.setdefault(k, []).append(r)
    hit = np.zeros(_as_tuple(build_keys)[0].length, dtype=bool)
    for pk in probe_batches:
        ok = _probe_valid(pk, null_unmatched)
        for k, v in zip(tuple_slots(pk), ok.tolist()):
            if v:
                for r in pos.get(k, ()):
                    hit[r] = True
    return hit


def marked_rows(build_keys, probe_batches, anti=False, null_unmatched=False):
    """the build rows kept, ascending"""
    m = marked_mask(build_keys, probe_batches, null_unmatched)
    return np.nonzero(~m if anti else m)[0].tolist()


def take_rows(cols, rows):
    """the compaction of `cols` to `rows`"""
    return oju.take_null(cols, np.asarray(rows, dtype=np.int64))


def probe_semi(right, probe_keys, build_keys, anti=False, null_unmatched=False):
    """the output batch of one probe: every right column and nothing else"""
    return take_rows(right, semi_rows(build_keys, probe_keys, anti, null_unmatched))


def slice_columns(cols, n):
    """the first n rows of every column"""
    return oju.take_null(cols, np.arange(n, dtype=np.int64))


# ----------------------------------------------------------------------------- build forms (the map at the top of hash_join.hip)
# (the generators of test_gpu_outer_join.py, copied: a test file is not imported)
def _unique_sparse_keys(rng, n):
    return np.unique(rng.integers(-(1 << 40), 1 << 40, 2 * n + 8))[:n][rng.permutation(n)].astype(np.int64) if n else np.zeros(0, np.int64)


def form_dense_full(rng, n):  # build_unique_dense: gap-free range, plain payload (dense_full)
    return [i64(rng.permutation(n) + 1000), i64(rng.integers(-5, 5, n))]


def form_dense_gaps(rng, n):  # build_unique_dense with gaps (presence bitmap)
    return [i64(rng.permutation(2 * n)[:n] - 7), Column.from_numpy(rng.normal(0, 1, n))]


def form_dense_bitmap(rng, n):  # not among the eight: dense_gaps draws keys below 0, whose UNSIGNED range is not dense (a hashed table); these stay dense → `presence`
    return [i64(rng.permutation(2 * n)[:n] + 7), Column.from_numpy(rng.normal(0, 1, n))]


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
         "sparse_check": (form_sparse_check, 0), "dup_dense": (form_dup_dense, 0), "dup_sparse": (form_dup_sparse, 0), "utf8": (form_utf8, 0),
         "dense_bitmap": (form_dense_bitmap, 0)}


def probe_side(rng, build_key, m, miss=0.3):
    """m probe rows [row number * 3, key]: keys drawn from the build keys, about `miss` of them (all of them at 1, none at 0) replaced
    by keys the build side does not have; an empty build side has only such keys"""
    if build_key.dtype == DType.UTF8:
        raw = oju.utf8_raw(build_key)
        items = [raw[int(i)] if raw and rng.random() >= miss else b"absent-%d" % int(i) for i in rng.integers(0, max(1, len(raw)), m)]
        return [i64(np.arange(m) * 3), oju.utf8_column(items)]
    bk = build_key.to_numpy()
    keys = bk[rng.integers(0, bk.size, m)].copy() if bk.size else np.zeros(m, np.int64)
    absent = rng.random(m) < miss if bk.size else np.ones(m, dtype=bool)
    keys[absent] = (I64.max - rng.integers(0, 1000, m))[absent]  # no build key is that large
    return [i64(np.arange(m) * 3), i64(keys)]  # key is column 1
