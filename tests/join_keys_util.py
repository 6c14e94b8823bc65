"""The yardstick of the tests of the hash join on several keys (quirk Q21): plain Python over tuples of raw key slots.  Nothing here
touches the device or the library, and nothing here knows of codes.

Match relation (the hash join's own, Q11 included, applied to every key pair): left = build side, right = probe side; two rows match iff
for every pair the raw 8-byte slot (the bytes between the offsets for Utf8) is equal — also under a NULL: key validity is ignored.
  per probe batch: probe-row-major (x, y) pairs, the matches of a probe row in ascending build row; with `keep_probe` (right / full) a
                   probe row without a match gives (None, y) in its place
  left / full:     one final list of (x, None) for the build rows that matched in none of the probe batches, ascending
The expected columns follow from the pairs through outer_join_util.take_null: a NULL-extended cell holds 0 / false / the empty string
under a NULL, and an output column has a validity bitmap iff its source has NULLs or the batch holds a NULL-extended row on that side."""
import numpy as np

import outer_join_util as oju

HOWS = ("inner", "left", "right", "full")


def tuples_of(cols, keys):
    """per row the tuple of raw key slots (unsigned words, bytes for Utf8)"""
    slots = [oju.key_slots(cols[k]) for k in keys]
    return list(zip(*slots)) if slots else []


def positions(left, lkeys):
    pos = {}
    for r, t in enumerate(tuples_of(left, lkeys)):
        pos.setdefault(t, []).append(r)
    return pos


def join_pairs(left, lkeys, batches, rkeys, how):
    """one list of (build row | None, probe row | None) per probe batch; for left / full one more: the never-matched build rows"""
    assert how in HOWS and len(lkeys) == len(rkeys) and lkeys
    keep_probe = how in ("right", "full")
    pos = positions(left, lkeys)
    nleft = left[0].length if left else 0
    hit = np.zeros(nleft, dtype=bool)
    out = []
    for right in batches:
        pairs = []
        for y, t in enumerate(tuples_of(right, rkeys)):
            m = pos.get(t)
            if m:
                pairs.extend((x, y) for x in m)
                hit[m] = True
            elif keep_probe:
                pairs.append((None, y))
        out.append(pairs)
    if how in ("left", "full"):
        out.append([(int(x), None) for x in np.nonzero(~hit)[0]])
    return out


def _idx(vals):
    return np.array([-1 if v is None else v for v in vals], dtype=np.int64)


def batch_columns(left, right, pairs):
    """the expected output columns of one probe batch: every left column taken by x, then every right column by y"""
    return oju.take_null(left, _idx([x for x, _ in pairs])) + oju.take_null(right, _idx([y for _, y in pairs]))


def final_columns(left, right_dtypes, pairs):
    """the expected final batch of a left / full join: the never-matched build rows, then all-NULL right columns"""
    assert all(y is None for _, y in pairs)
    return oju.take_null(left, _idx([x for x, _ in pairs])) + oju.null_columns(right_dtypes, len(pairs))


def expected_batches(left, lkeys, batches, rkeys, how, right_dtypes=None):
    """[(columns, null-extended mask of the left side, of the right side)] per output batch"""
    pairs = join_pairs(left, lkeys, batches, rkeys, how)
    out = []
    for right, p in zip(batches, pairs):
        out.append((batch_columns(left, right, p), np.array([x is None for x, _ in p], dtype=bool), np.zeros(len(p), dtype=bool)))
    if how in ("left", "full"):
        dts = right_dtypes if right_dtypes is not None else [c.dtype for c in batches[0]]
        p = pairs[-1]
        out.append((final_columns(left, dts, p), np.zeros(len(p), dtype=bool), np.ones(len(p), dtype=bool)))
    return out


def null_counts(cols):
    return [int(c.length - c.valid_mask().sum()) for c in cols]


def dense_tuple_ids(left, lkeys, batches, rkeys):
    """one Int64 id per row, equal iff the key tuples are equal, numbered by first appearance over the build side and then the probe
    batches: a single key that stands for the tuple (what the unmodified single-key oracle is handed)"""
    ids = {}
    lid = np.array([ids.setdefault(t, len(ids)) for t in tuples_of(left, lkeys)], dtype=np.int64)
    rids = [np.array([ids.setdefault(t, len(ids)) for t in tuples_of(right, rkeys)], dtype=np.int64) for right in batches]
    return lid, rids
