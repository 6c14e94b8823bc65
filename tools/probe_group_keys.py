#!/usr/bin/env python3
"""GROUP BY on several keys on the device (nqe_group_aggregate_execute, csrc/group_keys.hip; quirk Q20): what the tuple → code passes
cost next to the aggregate they feed.  HIP-event kernel time per call and per launch label (nqe_ctx_timing_report), and the wall time of
the call, over `--steps` steps after a warm-up; count / sum / avg / min / max over one Float64 column throughout.

  packed       `group by a, b`, two Int64 keys of 32 values each, against the same grouping written by hand for the single-key operator
               (nqe_aggregate_execute with the key expression `a * 32 + b`) and against `group by c` with 1024 values: the difference is
               what group_keys_ranges and group_keys_pack cost
  dictionary   two full-range Int64 keys (the spans' product overflows), and a Utf8 + Int64 pair, with 1024 and 10^6 distinct tuples
  one key      num_keys == 1 against nqe_aggregate_execute (it forwards): a bare column and `id % 1024`

Bytes = what the form must move per row: 8 per distinct 8-byte column read or written by every pass (the Utf8 column: its 4-byte
offsets and its bytes); the share of 8 TB/s is bytes over kernel time.

Usage: python tools/probe_group_keys.py [--rows 100000000] [--steps K] [--warmup W] [--out DIR]   (on a GPU machine; writes DIR/README.md
and DIR/probe.json)
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from naive_query_engine_amd import AggregateFunc, Column, DType, Field, Operator, capi  # noqa: E402
from naive_query_engine_amd.arrow_host import node_column  # noqa: E402
from naive_query_engine_amd.expression import binop, col, lit_i64  # noqa: E402

PEAK = 8e12  # bytes per second
AGGS = [(AggregateFunc.Count, 0), (AggregateFunc.Sum, 0), (AggregateFunc.Avg, 0), (AggregateFunc.Min, 0), (AggregateFunc.Max, 0)]


def measure(ctx, call, steps, warmup):
    """per step: wall ms, {label: ms}; returns the lists and the output's row count"""
    walls, reports, rows = [], [], 0
    for step in range(warmup + steps):
        ctx.synchronize()
        ctx.timing_reset()
        t0 = time.perf_counter()
        out = call()
        ctx.synchronize()
        wall = (time.perf_counter() - t0) * 1e3
        rpt = ctx.timing_report()
        rows = (out[0] if isinstance(out, tuple) else out).num_rows
        del out
        if step >= warmup:
            walls.append(wall)
            reports.append({k: v[0] for k, v in rpt.items()})
    return walls, reports, rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10 ** 8)
    ap.add_argument("--utf8-rows", type=int, default=None, help="rows of the Utf8 + Int64 shape (default: --rows)")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "group_keys"))
    a = ap.parse_args()
    import torch

    n = a.rows
    nu = a.utf8_rows or n
    os.makedirs(a.out, exist_ok=True)
    dev = torch.device("cuda", 0)
    ctx = capi.Context(0)
    ctx.timing_enable(True)

    def synth(kind, seed, rows, mod=1, dtype=torch.int64):
        t = torch.empty(rows, dtype=dtype, device=dev)
        torch.cuda.synchronize()
        ctx.synth_fill(kind, seed, 0, rows, mod, 0, t.data_ptr())
        ctx.synchronize()
        return t

    v = synth(2, 3, n, dtype=torch.float64)
    records = []

    def run(group, name, call, bytes_per_row, rows):
        walls, reports, out_rows = measure(ctx, call, a.steps, a.warmup)
        kern = [sum(r.values()) for r in reports]
        labels = sorted({k for r in reports for k in r})
        by_label = {k: float(np.median([r.get(k, 0.0) for r in reports])) for k in labels}
        med = float(np.median(kern))
        rec = dict(group=group, call=name, rows=rows, out_rows=out_rows, kernel_ms_median=med, kernel_ms_min=min(kern), kernel_ms_max=max(kern),
                   wall_ms_median=float(np.median(walls)), wall_ms_min=min(walls), wall_ms_max=max(walls), bytes_per_row=bytes_per_row,
                   share_of_8TBps=bytes_per_row * rows / (med * 1e-3) / PEAK, by_label_ms=by_label)
        records.append(rec)
        print(f"{group:>10} {name:>34} | groups {out_rows:>8} kernels {med:8.3f} ms [{min(kern):.3f}, {max(kern):.3f}] wall {rec['wall_ms_median']:8.3f} | "
              + " ".join(f"{k}={x:.3f}" for k, x in sorted(by_label.items(), key=lambda kv: -kv[1]) if x >= 0.0005), flush=True)
        with open(os.path.join(a.out, "probe.json"), "w") as f:
            json.dump(records, f, indent=1)

    # ---- packed path
    ka, kb, kc = synth(1, 11, n, 32), synth(1, 12, n, 32), synth(1, 13, n, 1024)
    t = ctx.table_from_device([(DType.FLOAT64, n, v.data_ptr(), None), (DType.INT64, n, ka.data_ptr(), None), (DType.INT64, n, kb.data_ptr(), None),
                               (DType.INT64, n, kc.data_ptr(), None)])
    fl = [Field(f"c{i}", DType.INT64, False) for i in range(4)]
    by_hand = binop(binop(col(1), Operator.Multiply, lit_i64(32)), Operator.Plus, col(2)).flatten(fl)
    # ranges: reads a, b; pack: reads a, b, writes the code; aggregate: reads the code and v
    run("packed", "group by a, b (32 x 32)", lambda: ctx.group_aggregate(t, [[node_column(1)], [node_column(2)]], AGGS), 16 + 24 + 16, n)
    # the key expression is evaluated into a column (reads a, b, writes it), then read beside v
    run("packed", "aggregate by a * 32 + b", lambda: ctx.aggregate(t, AGGS, group_nodes=by_hand), 24 + 16, n)
    run("packed", "aggregate by c (1024)", lambda: ctx.aggregate(t, AGGS, group_nodes=[node_column(3)]), 16, n)

    # ---- one key: forwards
    ids = synth(0, 0, n)
    t1 = ctx.table_from_device([(DType.FLOAT64, n, v.data_ptr(), None), (DType.INT64, n, ids.data_ptr(), None), (DType.INT64, n, kc.data_ptr(), None)])
    mod = binop(col(1), Operator.Modulos, lit_i64(1024)).flatten(fl)
    for label, key in (("c (1024)", [node_column(2)]), ("id % 1024", mod)):
        run("one key", f"group by {label}", lambda: ctx.group_aggregate(t1, [key], AGGS), 16, n)
        run("one key", f"aggregate by {label}", lambda: ctx.aggregate(t1, AGGS, group_nodes=key), 16, n)
    del t, t1, ka, kb, ids

    # ---- dictionary path: two full-range Int64 keys with D distinct tuples
    for d in (1024, 10 ** 6):
        base = synth(1, 21, n, d)
        fa = base * 0x5851F42D4C957F2D + 0x14057B7EF767814F  # (wrapping: every value of `base` lands somewhere in the whole Int64 range)
        fb = (base ^ 0x2545F491) * 0x2127599BF4325C37
        torch.cuda.synchronize()
        t = ctx.table_from_device([(DType.FLOAT64, n, v.data_ptr(), None), (DType.INT64, n, fa.data_ptr(), None), (DType.INT64, n, fb.data_ptr(), None),
                                   (DType.INT64, n, base.data_ptr(), None)])
        # dictionary: reads a, b, writes the code (plus the table's random traffic, not counted); aggregate: reads the code and v
        run("dictionary", f"group by a, b full-range ({d})", lambda: ctx.group_aggregate(t, [[node_column(1)], [node_column(2)]], AGGS), 24 + 16, n)
        run("dictionary", f"aggregate by the dense id ({d})", lambda: ctx.aggregate(t, AGGS, group_nodes=[node_column(3)]), 16, n)
        del t, fa, fb, base
    del v

    # ---- dictionary path: Utf8 + Int64 (8-byte strings "k0000000"; D = strings x 4 integer values)
    rng = np.random.default_rng(5)
    for d in (1024, 10 ** 6):
        sid = rng.integers(0, d // 4, nu)
        data = np.empty((nu, 8), dtype=np.uint8)
        data[:, 0] = ord("k")
        rest = sid.copy()
        for p in range(7, 0, -1):
            data[:, p] = ord("0") + rest % 10
            rest //= 10
        s = Column(DType.UTF8, nu, (np.arange(nu + 1, dtype=np.int64) * 8).astype(np.int32), None, data.reshape(-1))
        t = ctx.table_from_host([Column.from_numpy(rng.random(nu) * 100.0), s, Column.from_numpy(rng.integers(0, 4, nu).astype(np.int64)),
                                 Column.from_numpy((sid * 4 + rng.integers(0, 4, nu)).astype(np.int64))])
        del data, rest, s, sid
        # dictionary: reads offsets (4), bytes (8), b (8), writes the code (8); aggregate: reads the code and v
        run("dictionary", f"group by s, b Utf8 + Int64 ({d})", lambda: ctx.group_aggregate(t, [[node_column(1)], [node_column(2)]], AGGS), 28 + 16, nu)
        run("dictionary", f"aggregate by a dense id ({d})", lambda: ctx.aggregate(t, AGGS, group_nodes=[node_column(3)]), 16, nu)
        del t

    props = torch.cuda.get_device_properties(0)
    lines = ["# GROUP BY on several keys: what the tuple → code passes cost (`tools/probe_group_keys.py`)", "",
             f"Measured on one {props.name} ({props.multi_processor_count} CUs), {n} rows ({nu} for the Utf8 shapes), "
             f"{a.steps} steps after {a.warmup} warm-up steps.  `kernels` is the sum of the HIP-event times of every launch of the call "
             "(`nqe_ctx_timing_report`), median [min, max] over the steps — the spread is the noise between repeated runs; `wall` is the host time of "
             "the call including its read-backs.  `share` is the bytes the form must move over the kernel time, as a fraction of 8 TB/s.", "",
             "| shape | call | groups | kernels ms | wall ms | B/row | share |", "|---|---|---|---|---|---|---|"]
    for r in records:
        lines.append(f"| {r['group']} | {r['call']} | {r['out_rows']} | {r['kernel_ms_median']:.3f} [{r['kernel_ms_min']:.3f}, {r['kernel_ms_max']:.3f}] | "
                     f"{r['wall_ms_median']:.3f} [{r['wall_ms_min']:.3f}, {r['wall_ms_max']:.3f}] | {r['bytes_per_row']} | {r['share_of_8TBps']:.3f} |")
    lines += ["", "## Per launch label (median ms)", ""]
    for r in records:
        lines.append(f"* {r['group']}, {r['call']}: " + ", ".join(f"`{k}` {x:.3f}" for k, x in sorted(r["by_label_ms"].items(), key=lambda kv: -kv[1]) if x >= 0.0005))
    with open(os.path.join(a.out, "README.md"), "w") as f:
        f.write("\n".join(lines) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
