#!/usr/bin/env python3
"""Window functions on the device (nqe_window_execute, csrc/window.hip): the time of a call and its split over the launch labels, the
bytes each pass moves by design as a share of 8 TB/s, the rate of the permutation-ordered gather and of the scatter, and the window's
own kernels as a share of the whole call beside the sort passes of the same keys.

  table   id Int64 0 … n-1, k = id % 1024 (Int64), v Float64 normal; `partition by k order by v`
  cases   row_number() alone; plus sum(v) ROWS; plus sum(v) PARTITION
  bytes by design, n rows (K key columns of 8 bytes: here 2)
          win_bounds        4 n permutation + 8 n K key words (row i and row i - 1 share all but one fetch) + n / 4 for the two bitmaps
          win_pos_reduce    n / 4                  win_pos_apply   n / 4 + 4 n per position array
          win_gather        4 n + 8 n read + 8 n written        (bound by line fetches: every value is its own 64-byte line)
          win_scan_reduce   8 n + n / 8            win_scan_apply  8 n + n / 8 + 8 n per f64 operator (4 n for count)
          win_emit          4 n permutation + 4 n per position array + 8 n per state read + 8 n per column written (the scatter)

Usage: python tools/probe_window.py [--rows 100000000] [--reps K] [--out DIR]   (on a GPU machine; writes DIR/probe.txt and DIR/probe.json)
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from naive_query_engine_amd import Column, WindowFrame as F, WindowFunc as W, capi  # noqa: E402

PEAK = 8e12
WINDOW_LABELS = ("win_bounds", "win_pos_reduce", "win_pos_carry", "win_pos_apply", "win_gather", "win_scan_reduce", "win_scan_carry", "win_scan_apply", "win_emit")
CASES = [("row_number", [(W.RowNumber,)]), ("row_number+sum_rows", [(W.RowNumber,), (W.Sum, 2, F.Rows)]),
         ("row_number+sum_rows+sum_partition", [(W.RowNumber,), (W.Sum, 2, F.Rows), (W.Sum, 2, F.Partition)])]


def design_bytes(n, funcs, nkeys=2):
    """label -> bytes the pass moves by design for this function list (one value column, the sum operator)"""
    ranking = [f for f in funcs if len(f) == 1]
    aggs = [f for f in funcs if len(f) == 3]
    pos = {"part_first"} if ranking else set()
    pos |= {"part_last" for f in aggs if f[2] == F.Partition} | {"peer_last" for f in aggs if f[2] == F.Range}
    b = {"win_bounds": 4 * n + 8 * n * nkeys + n // 4}
    if pos:
        b["win_pos_reduce"] = n // 4
        b["win_pos_apply"] = n // 4 + 4 * n * len(pos)
    if aggs:
        b["win_gather"] = 4 * n + 8 * n + 8 * n
        b["win_scan_reduce"] = 8 * n + n // 8
        b["win_scan_apply"] = 8 * n + n // 8 + 8 * n
    b["win_emit"] = 4 * n + 4 * n * len(pos) + 8 * n * len(aggs) + 8 * n * len(funcs)
    return b


def measure(ctx, table, funcs, reps):
    walls, reports = [], []
    for rep in range(reps + 1):
        ctx.synchronize()
        ctx.timing_reset()
        t0 = time.perf_counter()
        out = ctx.window(table, [1], [2], funcs)
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
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "window"))
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    n = a.rows
    rng = np.random.default_rng(1)
    ids = np.arange(n, dtype=np.int64)
    ctx = capi.Context(0)
    table = ctx.table_from_host([Column.from_numpy(ids), Column.from_numpy(ids % 1024), Column.from_numpy(rng.normal(0, 1, n))])
    ctx.timing_enable(True)
    rows = []
    lines = [f"{n} rows, partition by id % 1024 order by v; medians of {a.reps} repetitions after a warm-up; ms; GB = bytes by design (tools/probe_window.py); share of 8 TB/s at the kernel time"]
    for name, funcs in CASES:
        wall, ms, cnt = measure(ctx, table, funcs, a.reps)
        design = design_bytes(n, funcs)
        kern = sum(ms.values())
        win = sum(v for k, v in ms.items() if k.startswith("win_"))
        lines.append(f"--- {name}: wall {wall:.3f}  all kernels {kern:.3f}  window kernels {win:.3f} ({win / kern:.3f} of the call)  sort and the rest {kern - win:.3f}")
        lines.append(f"{'label':>18} {'launches':>8} {'ms':>9} {'GB':>8} {'share':>6} {'Grows/s':>8}")
        for k in sorted(ms, key=lambda k: (not k.startswith("win_"), WINDOW_LABELS.index(k) if k in WINDOW_LABELS else 0, k)):
            gb = design.get(k)
            share = f"{gb / (ms[k] * 1e-3) / PEAK:6.3f}" if gb and ms[k] > 0 else "      "
            rate = f"{n / (ms[k] * 1e-3) / 1e9:8.2f}" if k in ("win_gather", "win_emit", "win_bounds") and ms[k] > 0 else "        "
            lines.append(f"{k:>18} {cnt[k]:>8} {ms[k]:9.3f} {(gb or 0) / 1e9:8.3f} {share} {rate}")
        rows.append(dict(rows=n, case=name, wall_ms=wall, kernel_ms=kern, window_kernel_ms=win, by_label_ms=ms, launches=cnt, design_bytes=design))
        print("\n".join(lines[-(len(ms) + 2):]), flush=True)
    with open(os.path.join(a.out, "probe.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    with open(os.path.join(a.out, "probe.json"), "w") as f:
        json.dump(rows, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
