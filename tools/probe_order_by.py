#!/usr/bin/env python3
"""ORDER BY on the device (nqe_sort_execute, csrc/order_by.hip): the time of a call and its split over the launch labels, the digit
passes of the radix sort that ran, and the bytes the passes and the final take must move as a share of 8 TB/s.

  cases   one Int64 key (random over the full range / below 2^24), one Float64 key, one nullable Int64 key, two keys, one 16-byte Utf8
          key; each with one and with four Int64 payload columns; the one-key case with fetch = 10
  bytes   per sort call: the histogram reads 8 n; a digit pass reads 8 n (count) and moves 12 n in and 12 n out (scatter); an encode pass
          writes 8 n (+ 4 n positions for the first) and reads the key (8 n; Utf8: offsets and bytes) and, from the second pass on, 4 n of
          permutation; the take reads 4 m and writes 8 m positions, then per 8-byte column reads 8 m positions and 8 m values and writes 8 m

Usage: python tools/probe_order_by.py [--sizes 1000000,10000000,100000000] [--reps K] [--out DIR]   (on a GPU machine; writes
DIR/probe.txt and DIR/probe.json)
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from naive_query_engine_amd import Column, DType, capi  # noqa: E402

PEAK = 8e12


def utf8_16(rng, n):
    raw = rng.integers(97, 123, (n, 16), dtype=np.uint8)
    return Column(DType.UTF8, n, (np.arange(n + 1, dtype=np.int64) * 16).astype(np.int32), None, raw.reshape(-1))


def cases(rng, n):
    i64 = np.iinfo(np.int64)
    full = rng.integers(i64.min, i64.max, n, dtype=np.int64)
    out = [("int64_full", [Column.from_numpy(full)], [0], None),
           ("int64_below_2p24", [Column.from_numpy(rng.integers(0, 1 << 24, n).astype(np.int64))], [0], None),
           ("float64", [Column.from_numpy(rng.normal(0, 1, n))], [0], None),
           ("int64_nullable", [Column.from_numpy(full, rng.random(n) > 0.1)], [0], None),
           ("two_keys", [Column.from_numpy(rng.integers(0, 1000, n).astype(np.int64)), Column.from_numpy(rng.normal(0, 1, n))], [0, 1], None),
           ("int64_full_fetch_10", [Column.from_numpy(full)], [0], 10)]
    if n * 16 < 2 ** 31:  # int32 offsets
        out.insert(5, ("utf8_16_bytes", [utf8_16(rng, n)], [0], None))
    return out


def key_bytes(c):
    return (c.length + 1) * 4 + int(c.data.size) if c.dtype == DType.UTF8 else c.length * 8


def measure(ctx, table, keys, fetch, reps):
    walls, reports = [], []
    for rep in range(reps + 1):
        ctx.synchronize()
        ctx.timing_reset()
        t0 = time.perf_counter()
        out = ctx.order_by(table, keys, fetch)
        ctx.synchronize()
        wall = (time.perf_counter() - t0) * 1e3
        rpt = ctx.timing_report()
        del out
        if rep:
            walls.append(wall)
            reports.append(rpt)
    names = sorted({k for r in reports for k in r})
    med = {k: float(np.median([r.get(k, (0.0, 0))[0] for r in reports])) for k in names}
    cnt = {k: reports[-1].get(k, (0.0, 0))[1] for k in names}
    return float(np.median(walls)), med, cnt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1000000,10000000,100000000")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "order_by"))
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    ctx = capi.Context(0)
    ctx.timing_enable(True)
    rows = []
    lines = [f"medians of {a.reps} repetitions after a warm-up; ms; bytes = what the passes and the take must move (tools/probe_order_by.py), share of 8 TB/s at the kernel time",
             f"{'rows':>10} {'case':>20} {'payload':>7} | {'wall':>8} {'kernels':>8} {'encode':>7} {'hist':>6} {'count':>7} {'scan':>6} {'scatter':>8} {'take':>7} | {'sorts':>5} {'digit passes':>12} {'GB':>7} {'share':>6}"]
    for n in [int(s) for s in a.sizes.split(",")]:
        rng = np.random.default_rng(n)
        for name, kcols, keys, fetch in cases(rng, n):
            for npay in (1, 4):
                cols = kcols + [Column.from_numpy(np.arange(n, dtype=np.int64) + p) for p in range(npay)]
                table = ctx.table_from_host(cols)
                wall, ms, cnt = measure(ctx, table, keys, fetch, a.reps)
                g = lambda pre: sum(v for k, v in ms.items() if k.startswith(pre))
                c = lambda pre: sum(v for k, v in cnt.items() if k.startswith(pre))
                sorts, passes, enc = c("radix_hist"), c("radix_scatter"), c("ob_encode")
                m = n if fetch is None else min(fetch, n)
                kb = sum(key_bytes(cols[k]) for k in keys)
                moved = sorts * 8 * n + passes * 32 * n + enc * 8 * n + 4 * n + kb + max(0, enc - 1) * 4 * n + 12 * m + len(cols) * 24 * m
                kern = sum(ms.values())
                rows.append(dict(rows=n, case=name, payload_columns=npay, fetch=fetch, wall_ms=wall, kernel_ms=kern, by_label_ms=ms, launches=cnt, sort_calls=sorts,
                                 digit_passes=passes, bytes_moved=moved, share_of_8TBps=moved / (kern * 1e-3) / PEAK))
                lines.append(f"{n:>10} {name:>20} {npay:>7} | {wall:8.3f} {kern:8.3f} {g('ob_encode'):7.3f} {g('radix_hist'):6.3f} {g('radix_count'):7.3f} {g('scan'):6.3f} {g('radix_scatter'):8.3f} "
                             f"{g('take') + g('utf8_take') + g('ob_positions'):7.3f} | {sorts:>5} {passes:>12} {moved / 1e9:7.3f} {moved / (kern * 1e-3) / PEAK:6.3f}")
                print(lines[-1], flush=True)
                del table
        with open(os.path.join(a.out, "probe.txt"), "w") as f:
            f.write("\n".join(lines) + "\n")
        with open(os.path.join(a.out, "probe.json"), "w") as f:
            json.dump(rows, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
