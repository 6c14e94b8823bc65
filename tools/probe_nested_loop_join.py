#!/usr/bin/env python3
"""NestedLoopJoin on the device (nqe_nested_loop_join_execute, csrc/nested_loop_join.hip): the compare rate of its count and emit
kernels, the split of a call over its launch labels, and the same inputs through nqe_hash_join_execute — the path a user has today.

  shapes   10^5 x 10^5, 10^6 x 10^4, 10^4 x 10^6 with unique Int64 keys (about min(L, R) matches), 10^5 x 10^5 with 1000 distinct keys
           (10^7 matches), and a size ladder n x n for the crossover with the hash join
  rate     L*R pairs / the HIP-event time of `nlj_count` (and of `nlj_emit`), as a share of the VALU issue bound the README derives
  split    nlj_count / scan / nlj_emit / take (every other label of the call is listed under `other`)

Usage: python tools/probe_nested_loop_join.py [--reps K] [--out DIR]   (on a GPU machine; writes DIR/probe.txt and DIR/probe.json)
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from naive_query_engine_amd import Column, capi  # noqa: E402

# the count loop issues two vector instructions per key pair (v_cmp_eq_u64 + v_cndmask / v_addc), a wave64 instruction takes a
# 32-lane SIMD two cycles: 64 pairs per 4 cycles per SIMD, 4 SIMDs on each of 256 CUs at 2.4 GHz (profiles/nested_loop_join/README.md)
ISSUE_BOUND = 64 / 4 * 4 * 256 * 2.4e9


def tables(ctx, L, R, distinct, seed):
    rng = np.random.default_rng(seed)
    if distinct is None:  # unique keys on both sides, the smaller side a subset of the larger
        big = rng.permutation(max(L, R)).astype(np.int64) * 7 - 12345
        lk, rk = big[:L].copy(), rng.permutation(big)[:R].copy() if R < L else big[rng.permutation(R)]
    else:
        lk, rk = rng.integers(0, distinct, L).astype(np.int64), rng.integers(0, distinct, R).astype(np.int64)
    mk = lambda k: ctx.table_from_host([Column.from_numpy(k), Column.from_numpy(np.arange(k.size, dtype=np.int64))])
    return mk(lk), mk(rk)


def timed(ctx, fn):
    ctx.synchronize()
    ctx.timing_reset()
    t0 = time.perf_counter()
    res = fn()
    ctx.synchronize()
    wall = (time.perf_counter() - t0) * 1e3
    return res, wall, ctx.timing_report()


def split(report):
    out = {"nlj_count": 0.0, "scan": 0.0, "nlj_emit": 0.0, "take": 0.0, "other": 0.0}
    for name, (ms, _) in report.items():
        key = next((k for k in ("nlj_count", "nlj_emit", "scan", "take") if name.startswith(k)), "other")
        out[key] += ms
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nested_loop_join"))
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    ctx = capi.Context(0)
    ctx.timing_enable(True)
    shapes = [(100_000, 100_000, None), (1_000_000, 10_000, None), (10_000, 1_000_000, None), (100_000, 100_000, 1000)]
    ladder = [(n, n, None) for n in (1000, 3000, 10_000, 30_000, 300_000)]
    rows, lines = [], []
    lines.append(f"issue bound {ISSUE_BOUND:.3e} pairs/s (2 vector instructions per pair); medians of {a.reps} repetitions after a warm-up; ms")
    lines.append(f"{'L':>8} {'R':>8} {'keys':>7} {'matches':>9} | {'count':>7} {'scan':>6} {'emit':>7} {'take':>6} {'other':>6} {'wall':>7} | {'count pairs/s':>13} {'share':>5} {'emit pairs/s':>12} {'share':>5} | {'hash ms':>8} {'nlj/hash':>8}")
    for L, R, distinct in shapes + ladder:
        lt, rt = tables(ctx, L, R, distinct, L + R)
        nl, hj = [], []
        for rep in range(a.reps + 1):
            t, wall, rep_n = timed(ctx, lambda: ctx.nested_loop_join(lt, rt, 0, 0))
            m = t.num_rows
            del t
            h, hwall, _ = timed(ctx, lambda: ctx.hash_join(lt, rt, 0, 0)) if distinct is None else (None, float("nan"), None)
            assert h is None or h.num_rows == m
            del h
            if rep:
                nl.append((wall, split(rep_n)))
                hj.append(hwall)
        med = lambda xs: float(np.median(xs))
        s = {k: med([x[1][k] for x in nl]) for k in nl[0][1]}
        wall, hwall = med([x[0] for x in nl]), med(hj)
        cr, er = L * R / (s["nlj_count"] * 1e-3), L * R / (s["nlj_emit"] * 1e-3)
        rows.append(dict(L=L, R=R, distinct=distinct, matches=m, split_ms=s, wall_ms=wall, count_pairs_per_s=cr, emit_pairs_per_s=er, count_share=cr / ISSUE_BOUND,
                         emit_share=er / ISSUE_BOUND, hash_join_wall_ms=hwall, nlj_over_hash=wall / hwall))
        lines.append(f"{L:>8} {R:>8} {('unique' if distinct is None else distinct):>7} {m:>9} | {s['nlj_count']:7.3f} {s['scan']:6.3f} {s['nlj_emit']:7.3f} {s['take']:6.3f} {s['other']:6.3f} {wall:7.3f} | "
                     f"{cr:13.3e} {cr / ISSUE_BOUND:5.2f} {er:12.3e} {er / ISSUE_BOUND:5.2f} | {hwall:8.3f} {wall / hwall:8.2f}")
        print(lines[-1], flush=True)
        del lt, rt
    with open(os.path.join(a.out, "probe.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    with open(os.path.join(a.out, "probe.json"), "w") as f:
        json.dump(rows, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
