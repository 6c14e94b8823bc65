#!/usr/bin/env python
"""CrossJoin on the device (nqe_cross_join_execute, csrc/cross_join.hip) against the take-based composition it replaces, at about
10^8 output rows per shape, beside the card's fill rate measured by the same run (tools/stream_bench).

Per shape, in one process, alternating after a warm-up:
  kernel   nqe_cross_join_execute: the `cross_join_*` launches (HIP events, nqe_ctx_timing_query) and the call's host wall time
           (ending in a stream synchronisation), once with plain and once with non-temporal stores (NQE_CROSS_JOIN_STORES)
  take     iota -> `% L` / `% R` (nqe_expr_evaluate) -> nqe_take of each side: every launch of the composition (HIP events)
Output bytes = N x 8 per 8-byte column + (N + 1) x 4 + payload per Utf8 column.  The rate is output bytes over kernel time.

Usage: python tools/probe_cross_join.py [--reps K] [--out DIR]   (on a GPU machine; writes DIR/probe.txt and DIR/probe.json)
"""
import argparse
import json
import os
import re
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from naive_query_engine_amd import Column, DType, Operator, capi  # noqa: E402
from naive_query_engine_amd.expression import binop, col, lit_i64  # noqa: E402
from tests.helpers import fields  # noqa: E402


def fill_rate():
    """the best `copy read=0 write=4` (pure fill) line of tools/stream_bench, in GB/s"""
    exe = os.path.join(ROOT, "tools", "stream_bench")
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300).stdout
    lines = [ln for ln in out.splitlines() if "read=0 write=4" in ln]
    best = max(lines, key=lambda ln: float(re.search(r"= (\d+) GB/s", ln).group(1)))
    return float(re.search(r"= (\d+) GB/s", best).group(1)), best


def word_table(ctx, n, seed, keep):
    """two device-generated 8-byte columns (Int64 row ids, Float64 uniform) of n rows"""
    cols = []
    for kind, dt in ((0, DType.INT64), (2, DType.FLOAT64)):
        p = ctx.device_alloc(n * 8)
        keep.append(p)
        ctx.synth_fill(kind, seed, 0, n, 1, 0, p)
        cols.append((dt, n, p, None))
    return ctx.table_from_device(cols)


def utf8_words_table(ctx, n, seed):
    rng = np.random.default_rng(seed)
    words = ["", "a", "bc", "héllo", "naive", "query-engine", "日本語"]
    strs = [words[k] for k in rng.integers(0, len(words), n)]
    return ctx.table_from_host([Column.from_numpy(np.arange(n, dtype=np.int64)), Column.from_list(strs, DType.UTF8)])


def out_bytes(t):
    b = 0
    for i in range(t.num_columns):
        c = t.column_info(i)
        b += c.length * 8 if c.dtype != int(DType.UTF8) else (c.length + 1) * 4 + c.data_length
    return b


def take_composition(ctx, lt, rt, n, iota_ptr):
    """iota -> % -> take: the A/B baseline (8-byte index written, then read back once per column it gathers)"""
    L, R = lt.num_rows, rt.num_rows
    ctx.synth_fill(0, 0, 0, n, 1, 0, iota_ptr)
    iota = ctx.table_from_device([(DType.INT64, n, iota_ptr, None)])
    f = fields("j")
    il = ctx.expr_evaluate(iota, binop(col(0), Operator.Modulos, lit_i64(L)).flatten(f))
    ir = ctx.expr_evaluate(iota, binop(col(0), Operator.Modulos, lit_i64(R)).flatten(f))
    return ctx.take(lt, il), ctx.take(rt, ir)


def timed(ctx, fn):
    ctx.synchronize()
    ctx.timing_reset()
    t0 = time.perf_counter()
    res = fn()
    ctx.synchronize()
    wall = (time.perf_counter() - t0) * 1e3
    rep = ctx.timing_report()
    return res, wall, rep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cross_join"))
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    fill, fill_line = fill_rate()
    ctx = capi.Context(0)
    ctx.timing_enable(True)
    keep = []
    shapes = [("big x small", 25_000_000, 4, "words"), ("square", 10_000, 10_000, "words"), ("small x big", 4, 25_000_000, "words"),
              ("square, Int64 + Utf8 each side", 10_000, 10_000, "utf8")]
    iota = ctx.device_alloc(100_000_000 * 8)
    lines = [f"fill (tools/stream_bench, same call): {fill:.0f} GB/s   [{fill_line.strip()}]", ""]
    results = []
    for name, L, R, kind in shapes:
        n = L * R
        if kind == "words":
            lt, rt = word_table(ctx, L, 1, keep), word_table(ctx, R, 2, keep)
        else:
            lt, rt = utf8_words_table(ctx, L, 1), utf8_words_table(ctx, R, 2)
        # correctness of both forms on this shape (first and last rows)
        t = ctx.cross_join(lt, rt)
        tl, tr = take_composition(ctx, lt, rt, n, iota)
        for part in (0, n - 1000):
            a1 = [c.to_list() for c in ctx.slice(t, part, 1000).to_host()]
            b1 = [c.to_list() for c in ctx.slice(tl, part, 1000).to_host()] + [c.to_list() for c in ctx.slice(tr, part, 1000).to_host()]
            assert a1 == b1, f"{name}: the kernel and the take composition differ near row {part}"
        nbytes = out_bytes(t)
        del t, tl, tr
        rec = {"shape": name, "L": L, "R": R, "N": n, "output_bytes": nbytes, "plain": [], "nt": [], "take": []}
        for rep in range(a.reps + 1):  # rep 0: warm-up
            for mode in ("plain", "nt", "take"):
                if mode == "take":
                    res, wall, report = timed(ctx, lambda: take_composition(ctx, lt, rt, n, iota))
                    kern = sum(ms for k, (ms, _) in report.items())
                    launches = sum(c for k, (_, c) in report.items())
                else:
                    os.environ["NQE_CROSS_JOIN_STORES"] = mode
                    res, wall, report = timed(ctx, lambda: ctx.cross_join(lt, rt))
                    kern = sum(ms for k, (ms, _) in report.items() if k.startswith("cross_join"))
                    launches = sum(c for k, (_, c) in report.items() if k.startswith("cross_join"))
                del res
                if rep:
                    rec[mode].append({"kernel_ms": kern, "wall_ms": wall, "launches": launches})
        os.environ.pop("NQE_CROSS_JOIN_STORES", None)
        med = {m: float(np.median([x["kernel_ms"] for x in rec[m]])) for m in ("plain", "nt", "take")}
        wall = {m: float(np.median([x["wall_ms"] for x in rec[m]])) for m in ("plain", "nt", "take")}
        rec["median_kernel_ms"], rec["median_wall_ms"] = med, wall
        rec["fill_GBps"] = fill
        for m in ("plain", "nt"):
            rec[f"{m}_GBps"] = nbytes / med[m] / 1e6
            rec[f"{m}_frac_of_fill"] = rec[f"{m}_GBps"] / fill
        rec["speedup_over_take_plain"] = med["take"] / med["plain"]
        rec["speedup_over_take_nt"] = med["take"] / med["nt"]
        results.append(rec)
        lines.append(f"{name}: L={L} R={R} N={n} output {nbytes / 1e9:.3f} GB")
        for m in ("plain", "nt"):
            lines.append(f"  kernel {m:5s}: {med[m]:.3f} ms kernels ({rec[m][0]['launches']} launches), {wall[m]:.3f} ms wall, "
                         f"{rec[m + '_GBps']:.0f} GB/s = {rec[m + '_frac_of_fill']:.3f} of fill, {med['take'] / med[m]:.2f}x the take form")
        lines.append(f"  take        : {med['take']:.3f} ms kernels ({rec['take'][0]['launches']} launches), {wall['take']:.3f} ms wall")
        del lt, rt
        ctx.trim()
    txt = "\n".join(lines)
    print(txt)
    with open(os.path.join(a.out, "probe.txt"), "w") as f:
        f.write(txt + "\n")
    with open(os.path.join(a.out, "probe.json"), "w") as f:
        json.dump({"fill_GBps": fill, "fill_line": fill_line.strip(), "shapes": results}, f, indent=1)
    ctx.device_free(iota)
    for p in keep:
        ctx.device_free(p)


if __name__ == "__main__":
    main()
