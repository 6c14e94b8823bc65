#!/usr/bin/env python3
"""Semi and anti hash joins on the device (nqe_hash_join_probe_semi, csrc/hash_join_semi_kernels.hpp): the HIP-event kernel time of a
call and its split over the launch labels, next to what a caller had to do before and next to the floor.

  shapes  c4_100      10^8 fact rows against a 10^6-row dimension on a gap-free primary key (bench.py's C4): every probe row matches
          c4_50       the same with foreign keys drawn from [0, 2 nb): half of them match
          c4_sparse   bench.py's c4_sparse: unique build keys spread over a 2^20 x nb domain (a hashed table), every probe row matches
          dup4        every build key four times (nb / 4 distinct keys), foreign keys from [0, nb): a quarter matches
          c4_2keys    C4 joined on (k / 1000, k % 1000), half of the tuples match: the probe codes are packed first
  calls   semi / anti   nqe_hash_join_probe_semi without and with NQE_SEMI_ANTI
          inner         nqe_hash_join_probe_keys over the same tables: what a caller must do today (and then drop the build columns,
                        and — with duplicate build keys — deduplicate)
          semi_per_lane / anti_per_lane   (hashed tables only) the same with NQE_SEMI_NO_COOP=1: the per-lane probe_one lookup instead
                        of the wave-cooperative bucket read
          floor_semi / floor_anti   nqe_selection_execute with `key < c` over the same probe table, c chosen so that it keeps as many
                        rows as semi / anti do: the same keep mask and compaction without a lookup
  ratio   each figure over the inner probe of the same tables (kernel time)

Usage: python tools/probe_semi_join.py [--rows 100000000] [--dim-rows 1000000] [--reps K] [--shapes a,b] [--out DIR]   (on a GPU machine;
writes DIR/probe.txt and DIR/probe.json)
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from naive_query_engine_amd import DType, Operator, capi  # noqa: E402
from naive_query_engine_amd.expression import binop, col, lit_i64  # noqa: E402

SHAPES = ["c4_100", "c4_50", "c4_sparse", "dup4", "c4_2keys"]


def make_shape(torch, ctx, shape, rows, nb):
    """dim = build side, fact = probe side, as bench.py's make_join_data; returns (dim, build keys, fact, probe keys, the probe key tensor the
    floor's predicate reads, the tensors behind the tables)"""
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
    fdom = 2 * nb if shape in ("c4_50", "c4_2keys") else nb
    fidx = synth(1, 5, rows, fdom)
    val = synth(2, 3, rows, dtype=torch.float64)
    if shape == "c4_sparse":
        dom = (torch.arange(nb, device=dev, dtype=torch.int64) << 20) + synth(1, 11, nb, 1 << 20)
        dkey, fkey = dom[perm].contiguous(), dom[fidx].contiguous()
    elif shape == "dup4":
        dkey, fkey = (perm % (nb // 4)).contiguous(), fidx
    else:
        dkey, fkey = perm, fidx
    torch.cuda.synchronize()
    I, F = DType.INT64, DType.FLOAT64
    if shape == "c4_2keys":
        d1, d2 = (dkey // 1000).contiguous(), (dkey % 1000).contiguous()
        f1, f2 = (fkey // 1000).contiguous(), (fkey % 1000).contiguous()
        torch.cuda.synchronize()
        dim = ctx.table_from_device([(I, nb, d1.data_ptr(), None), (I, nb, d2.data_ptr(), None), (I, nb, attr.data_ptr(), None)])
        fact = ctx.table_from_device([(I, rows, f1.data_ptr(), None), (I, rows, f2.data_ptr(), None), (F, rows, val.data_ptr(), None)])
        return dim, [0, 1], fact, [0, 1], f1, (d1, d2, f1, f2, attr, val)
    dim = ctx.table_from_device([(I, nb, dkey.data_ptr(), None), (I, nb, attr.data_ptr(), None)])
    fact = ctx.table_from_device([(I, rows, fkey.data_ptr(), None), (F, rows, val.data_ptr(), None)])
    return dim, [0], fact, [0], fkey, (dkey, attr, fkey, val)


def threshold_for(torch, key, want):
    """c with count(key < c) as close to `want` as the key values allow (bisection over the key range)"""
    lo, hi = int(key.min().item()), int(key.max().item()) + 1
    while lo < hi:
        mid = (lo + hi) // 2
        if int((key < mid).sum().item()) < want:
            lo = mid + 1
        else:
            hi = mid
    return lo


def per_lane(call):
    """`call` with NQE_SEMI_NO_COOP=1 (read per call)"""
    def run():
        os.environ["NQE_SEMI_NO_COOP"] = "1"
        try:
            return call()
        finally:
            del os.environ["NQE_SEMI_NO_COOP"]
    return run


def measure(ctx, call, reps):
    """medians over `reps` repetitions after a warm-up: wall ms, {label: ms}, {label: launches}, output rows"""
    walls, reports, rows = [], [], 0
    for rep in range(reps + 1):
        ctx.synchronize()
        ctx.timing_reset()
        t0 = time.perf_counter()
        out = call()
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
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "semi_join"))
    a = ap.parse_args()
    import torch

    os.makedirs(a.out, exist_ok=True)
    ctx = capi.Context(0)
    ctx.timing_enable(True)
    records = []
    lines = [f"medians of {a.reps} repetitions after a warm-up; ms of HIP-event kernel time; ratio = kernel time over the inner probe of the same tables (tools/probe_semi_join.py)",
             f"{'shape':>10} {'call':>13} | {'out rows':>10} {'wall':>8} {'kernels':>8} {'ratio':>6} | per launch label"]
    fields = [type("F", (), {"name": "key"})()]
    for shape in a.shapes.split(","):
        dim, lkeys, fact, rkeys, fkey, keep = make_shape(torch, ctx, shape, a.rows, a.dim_rows)
        jt = ctx.hash_join_build_keys(dim, lkeys)
        semi_rows = ctx.hash_join_probe_semi(jt, fact, rkeys).num_rows
        preds = {}
        for name, want in (("floor_semi", semi_rows), ("floor_anti", a.rows - semi_rows)):
            c = threshold_for(torch, fkey, want)
            preds[name] = binop(col(0), Operator.Lt, lit_i64(c)).flatten(fields)
        torch.cuda.synchronize()
        calls = [("inner", lambda: ctx.hash_join_probe_keys(jt, fact, rkeys)),
                 ("semi", lambda: ctx.hash_join_probe_semi(jt, fact, rkeys)),
                 ("anti", lambda: ctx.hash_join_probe_semi(jt, fact, rkeys, anti=True)),
                 ("floor_semi", lambda: ctx.selection(fact, preds["floor_semi"])),
                 ("floor_anti", lambda: ctx.selection(fact, preds["floor_anti"]))]
        if shape == "c4_sparse":
            calls[3:3] = [("semi_per_lane", per_lane(calls[1][1])), ("anti_per_lane", per_lane(calls[2][1]))]
        inner_kern = None
        for name, call in calls:
            wall, ms, cnt, out_rows = measure(ctx, call, a.reps)
            kern = sum(ms.values())
            if name == "inner":
                inner_kern = kern
            ratio = kern / inner_kern
            records.append(dict(shape=shape, call=name, probe_rows=a.rows, build_rows=a.dim_rows, out_rows=out_rows, wall_ms=wall, kernel_ms=kern, ratio_to_inner=ratio,
                                by_label_ms=ms, launches=cnt))
            labels = " ".join(f"{k}={v:.3f}" for k, v in sorted(ms.items(), key=lambda kv: -kv[1]) if v >= 0.0005)
            lines.append(f"{shape:>10} {name:>13} | {out_rows:>10} {wall:8.3f} {kern:8.3f} {ratio:6.2f} | {labels}")
            print(lines[-1], flush=True)
        del jt, dim, fact, keep, fkey
        with open(os.path.join(a.out, "probe.txt"), "w") as f:
            f.write("\n".join(lines) + "\n")
        with open(os.path.join(a.out, "probe.json"), "w") as f:
            json.dump(records, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
