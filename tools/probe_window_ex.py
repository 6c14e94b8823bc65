#!/usr/bin/env python3
"""nqe_window_execute_ex on the device (csrc/window.hip, window_ex_kernels.hpp): what bounded ROWS BETWEEN frames and the value
functions cost beside the old ROWS frame, per launch label, on tools/probe_window.py's table.

  table   id Int64 0 … n-1, k = id % 1024 (Int64), v Float64 normal; `partition by k order by v`
  cases   old_sum_rows      sum(v) ROWS through nqe_window_execute — the yardstick
          sum_w7            sum(v) ROWS BETWEEN 3 PRECEDING AND 3 FOLLOWING          (measured twice: the second run is the narrow width's spread)
          sum_w100001       sum(v) ROWS BETWEEN 50000 PRECEDING AND 50000 FOLLOWING  (by construction the cost does not depend on the width)
          avg_min_max_w7    avg(v), min(v), max(v) over one (-6, 0): one gather, one reversal, two scans of four operators
          lag1              lag(v, 1)
  bytes by design, n rows (beyond tools/probe_window.py's formulas for win_bounds, win_pos_*, win_gather and win_scan_* — a bounded
  frame runs win_scan_reduce / win_scan_apply TWICE, over the column and over its reversal)
          win_flags         n / 8 partition-start bits read + 2 n / 8 written
          win_reverse       8 n read + 8 n written (+ 2 n / 8 with NULLs)
          win_frame_emit    4 n permutation + 8 n for the two position arrays + per function up to 2 x (8 n per f64 state, 4 n per count) read
                            through a computed index (neighbouring threads read neighbouring or equal words) + 8 n per column written (the scatter)
          win_inverse       4 n read + 4 n written (the scatter)
          win_value_emit    4 n positions + 8 n for the two position arrays (gathered: position order, not row order) + per function 4 n
                            permutation + 8 n value (both gathered) + 8 n written + n / 8 validity (coalesced)

Usage: python tools/probe_window_ex.py [--rows 100000000] [--reps K] [--out DIR]   (on a GPU machine; writes DIR/probe.txt and DIR/probe.json)
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from naive_query_engine_amd import Column, WindowFrame as F, WindowFrameEx as FX, WindowFunc as W, WindowFuncEx as WX, capi  # noqa: E402

PEAK = 8e12
LABELS = ("win_bounds", "win_pos_reduce", "win_pos_carry", "win_pos_apply", "win_gather", "win_reverse", "win_flags", "win_scan_reduce", "win_scan_carry", "win_scan_apply", "win_emit",
          "win_frame_emit", "win_inverse", "win_value_emit")


def between(func, start, end):
    return {"func": func, "column": 2, "frame": FX.RowsBetween, "start": start, "end": end}


CASES = [("old_sum_rows", None, [(W.Sum, 2, F.Rows)]),
         ("sum_w7", 1, [between(WX.Sum, -3, 3)]),
         ("sum_w7_again", 1, [between(WX.Sum, -3, 3)]),
         ("sum_w100001", 1, [between(WX.Sum, -50000, 50000)]),
         ("avg_min_max_w7", 3, [between(WX.Avg, -6, 0), between(WX.Min, -6, 0), between(WX.Max, -6, 0)]),
         ("lag1", 0, [{"func": WX.Lag, "column": 2, "param": 1}])]


def design_bytes(n, name, nkeys=2):
    b = {"win_bounds": 4 * n + 8 * n * nkeys + n // 4}
    if name == "old_sum_rows":
        b.update({"win_gather": 20 * n, "win_scan_reduce": 8 * n + n // 8, "win_scan_apply": 16 * n + n // 8, "win_emit": 4 * n + 8 * n + 8 * n})
        return b
    b.update({"win_pos_reduce": n // 4, "win_pos_apply": n // 4 + 8 * n})
    if name == "lag1":
        b.update({"win_inverse": 8 * n, "win_value_emit": 4 * n + 8 * n + 4 * n + 8 * n + 8 * n + n // 8})
        return b
    states = 8 if name.startswith("sum") else 8 + 4 + 8 + 8  # bytes per row of one scan's state arrays
    columns = 1 if name.startswith("sum") else 3
    b.update({"win_gather": 20 * n, "win_reverse": 16 * n, "win_flags": 3 * n // 8, "win_scan_reduce": 2 * (8 * n + n // 8), "win_scan_apply": 2 * (8 * n + n // 8 + states * n),
              "win_frame_emit": 4 * n + 8 * n + 2 * states * n + 8 * n * columns})
    return b


def measure(ctx, table, old, funcs, reps):
    walls, reports = [], []
    for rep in range(reps + 1):
        ctx.synchronize()
        ctx.timing_reset()
        t0 = time.perf_counter()
        out = ctx.window(table, [1], [2], funcs) if old else ctx.window_ex(table, [1], [2], funcs)
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "window_ex"))
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    n = a.rows
    rng = np.random.default_rng(1)
    ids = np.arange(n, dtype=np.int64)
    ctx = capi.Context(0)
    table = ctx.table_from_host([Column.from_numpy(ids), Column.from_numpy(ids % 1024), Column.from_numpy(rng.normal(0, 1, n))])
    ctx.timing_enable(True)
    rows = []
    lines = [f"{n} rows, partition by id % 1024 order by v; medians of {a.reps} repetitions after a warm-up; ms; GB = bytes by design (tools/probe_window_ex.py); share of 8 TB/s at the kernel time"]
    win_ms = {}
    for name, _, funcs in CASES:
        wall, ms, cnt = measure(ctx, table, name == "old_sum_rows", funcs, a.reps)
        design = design_bytes(n, name.replace("_again", ""))
        kern = sum(ms.values())
        win = sum(v for k, v in ms.items() if k.startswith("win_"))
        win_ms[name] = win
        lines.append(f"--- {name}: wall {wall:.3f}  all kernels {kern:.3f}  window kernels {win:.3f} ({win / kern:.3f} of the call)  sort and the rest {kern - win:.3f}")
        lines.append(f"{'label':>18} {'launches':>8} {'ms':>9} {'GB':>8} {'share':>6}")
        for k in sorted(ms, key=lambda k: (not k.startswith("win_"), LABELS.index(k) if k in LABELS else 0, k)):
            gb = design.get(k)
            share = f"{gb / (ms[k] * 1e-3) / PEAK:6.3f}" if gb and ms[k] > 0 else "      "
            lines.append(f"{k:>18} {cnt[k]:>8} {ms[k]:9.3f} {(gb or 0) / 1e9:8.3f} {share}")
        rows.append(dict(rows=n, case=name, wall_ms=wall, kernel_ms=kern, window_kernel_ms=win, by_label_ms=ms, launches=cnt, design_bytes=design))
        print("\n".join(lines[-(len(ms) + 2):]), flush=True)
    old, narrow, again, wide = (win_ms[k] for k in ("old_sum_rows", "sum_w7", "sum_w7_again", "sum_w100001"))
    lines.append(f"--- window kernels: sum w=7 {narrow:.3f} and again {again:.3f} (spread {abs(narrow - again):.3f}); w=100001 {wide:.3f} (difference to the first {wide - narrow:+.3f}); "
                 f"bounded / old ROWS {narrow / old:.3f}")
    print(lines[-1], flush=True)
    with open(os.path.join(a.out, "probe.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    with open(os.path.join(a.out, "probe.json"), "w") as f:
        json.dump(rows, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
