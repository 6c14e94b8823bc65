#!/usr/bin/env python3
"""Outer hash joins on the device (nqe_hash_join_probe_outer / nqe_hash_join_unmatched_build, csrc/hash_join_outer_kernels.hpp): the
HIP-event kernel time of a call and its split over the launch labels, next to the inner nqe_hash_join_probe over the same tables.

  shapes  c4_dense    10^8 fact rows joined to a 10^6-row dimension on a gap-free primary key (bench.py's C4): every probe row matches once
          partial_90  the same with foreign keys drawn from [0, nb / 0.9): 90 % match
          dup4        every build key four times (nb / 4 distinct keys), foreign keys from [0, nb): a quarter matches, 4 rows each
  calls   inner (nqe_hash_join_probe: the fused tiers), outer with flags = 0 and no marks (the general path alone), outer with
          NQE_JOIN_KEEP_PROBE, outer with marks (fresh marks per repetition: every first hit pays its atomic), outer with both, and the
          unmatched-build pass after a marked probe
  ratio   each outer figure over the inner probe of the same tables (kernel time)

Usage: python tools/probe_outer_join.py [--rows 100000000] [--dim-rows 1000000] [--reps K] [--out DIR]   (on a GPU machine; writes
DIR/probe.txt and DIR/probe.json)
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from naive_query_engine_amd import DType, capi  # noqa: E402


def make_shape(torch, ctx, shape, rows, nb):
    """dim(id, attr) = build side, fact(key, val) = probe side, as bench.py's make_join_data; returns the tables and the tensors behind them"""
    dev = torch.device("cuda", 0)

    def synth(kind, seed, n, mod=1, dtype=torch.int64):
        torch.cuda.synchronize()
        t = torch.empty(n, dtype=dtype, device=dev)
        ctx.synth_fill(kind, seed, 0, n, mod, 0, t.data_ptr())
        ctx.synchronize()
        return t

    g = torch.Generator(device=dev).manual_seed(7)
    perm = torch.randperm(nb, device=dev, generator=g).to(torch.int64)
    attr = synth(1, 4, nb, 1 << 20)
    fdom = int(math.ceil(nb / 0.9)) if shape == "partial_90" else nb
    fkey = synth(1, 5, rows, fdom)
    dkey = (perm % (nb // 4)).contiguous() if shape == "dup4" else perm
    val = synth(2, 3, rows, dtype=torch.float64)
    torch.cuda.synchronize()
    dim = ctx.table_from_device([(DType.INT64, nb, dkey.data_ptr(), None), (DType.INT64, nb, attr.data_ptr(), None)])
    fact = ctx.table_from_device([(DType.INT64, rows, fkey.data_ptr(), None), (DType.FLOAT64, rows, val.data_ptr(), None)])
    return dim, fact, (dkey, attr, fkey, val)


def measure(ctx, call, reps, prepare=None):
    """medians over `reps` repetitions after a warm-up: wall ms, {label: ms}, {label: launches}, output rows"""
    walls, reports, rows = [], [], 0
    for rep in range(reps + 1):
        arg = prepare() if prepare else None
        ctx.synchronize()
        ctx.timing_reset()
        t0 = time.perf_counter()
        out = call(arg)
        ctx.synchronize()
        wall = (time.perf_counter() - t0) * 1e3
        rpt = ctx.timing_report()
        rows = out.num_rows
        del out
        if rep:
            walls.append(wall)
            reports.append(rpt)
    names = sorted({k for r in reports for k in r})
    med = {k: float(np.median([r.get(k, (0.0, 0))[0] for r in reports])) for k in names}
    cnt = {k: reports[-1].get(k, (0.0, 0))[1] for k in names}
    return float(np.median(walls)), med, cnt, rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10 ** 8)
    ap.add_argument("--dim-rows", type=int, default=10 ** 6)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--shapes", default="c4_dense,partial_90,dup4")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "outer_join"))
    a = ap.parse_args()
    import torch

    os.makedirs(a.out, exist_ok=True)
    ctx = capi.Context(0)
    ctx.timing_enable(True)
    records = []
    lines = [f"medians of {a.reps} repetitions after a warm-up; ms of HIP-event kernel time; ratio = kernel time over the inner probe of the same tables (tools/probe_outer_join.py)",
             f"{'shape':>11} {'call':>16} | {'out rows':>10} {'wall':>8} {'kernels':>8} {'ratio':>6} | per launch label"]
    for shape in a.shapes.split(","):
        dim, fact, keep = make_shape(torch, ctx, shape, a.rows, a.dim_rows)
        jt = ctx.hash_join_build(dim, 0)
        rt_dtypes = [DType.INT64, DType.FLOAT64]
        calls = [("inner", lambda m: ctx.hash_join_probe(jt, fact, 0), None),
                 ("outer_plain", lambda m: ctx.hash_join_probe_outer(jt, fact, 0), None),
                 ("outer_keep_probe", lambda m: ctx.hash_join_probe_outer(jt, fact, 0, keep_probe=True), None),
                 ("outer_marks", lambda m: ctx.hash_join_probe_outer(jt, fact, 0, marks=m), lambda: ctx.join_marks(jt)),
                 ("outer_both", lambda m: ctx.hash_join_probe_outer(jt, fact, 0, keep_probe=True, marks=m), lambda: ctx.join_marks(jt))]
        marked = ctx.join_marks(jt)
        del_me = ctx.hash_join_probe_outer(jt, fact, 0, marks=marked)
        del del_me
        calls.append(("unmatched_build", lambda m: ctx.hash_join_unmatched_build(jt, marked, rt_dtypes), None))
        inner_kern = None
        for name, call, prepare in calls:
            wall, ms, cnt, out_rows = measure(ctx, call, a.reps, prepare)
            kern = sum(ms.values())
            if name == "inner":
                inner_kern = kern
            ratio = kern / inner_kern
            records.append(dict(shape=shape, call=name, probe_rows=a.rows, build_rows=a.dim_rows, out_rows=out_rows, wall_ms=wall, kernel_ms=kern, ratio_to_inner=ratio,
                                by_label_ms=ms, launches=cnt))
            labels = " ".join(f"{k}={v:.3f}" for k, v in sorted(ms.items(), key=lambda kv: -kv[1]) if v >= 0.0005)
            lines.append(f"{shape:>11} {name:>16} | {out_rows:>10} {wall:8.3f} {kern:8.3f} {ratio:6.2f} | {labels}")
            print(lines[-1], flush=True)
        del jt, marked, dim, fact, keep
        with open(os.path.join(a.out, "probe.txt"), "w") as f:
            f.write("\n".join(lines) + "\n")
        with open(os.path.join(a.out, "probe.json"), "w") as f:
            json.dump(records, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
