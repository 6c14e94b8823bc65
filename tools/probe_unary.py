#!/usr/bin/env python
"""Kernel times of PhysicalUnaryExpr trees on one GPU (HIP events through nqe_ctx_timing_*): one process, warm-up, then the median
of --steps executions over --rows Float64 rows, for

    abs(v)                       projection          (against `v * 2.0`: the same 8 B in + 8 B out per row)
    sin(v)                       projection
    sin(v) * 2.0 > 0.5           selection predicate, projecting id
    cos(v) > 0.25                predicate of count / sum / min / max group by id % 7

each in the one-pass form (the stack machine or its run-time compiled kernel) and node-at-a-time (NQE_NO_EXPR_TREE=1).
Writes probe.json and probe.txt under --out (default profiles/unary)."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "unary"))
    a = ap.parse_args()
    from naive_query_engine_amd import AggregateFunc, Column, Operator, UnaryOperator, capi
    from naive_query_engine_amd.expression import binop, col, lit_f64, lit_i64, unop

    class F:
        def __init__(self, name):
            self.name = name

    f = [F("id"), F("v")]
    n = a.rows
    rng = np.random.default_rng(7)
    ctx = capi.Context(0)
    t = ctx.table_from_host([Column.from_numpy(np.arange(n, dtype=np.int64)), Column.from_numpy(rng.random(n) * 200.0 - 100.0)])
    v = col(1)
    sin_pred = binop(binop(unop(UnaryOperator.Sin, v), Operator.Multiply, lit_f64(2.0)), Operator.Gt, lit_f64(0.5)).flatten(f)
    cos_pred = binop(unop(UnaryOperator.Cos, v), Operator.Gt, lit_f64(0.25)).flatten(f)
    key = binop(col(0), Operator.Modulos, lit_i64(7)).flatten(f)
    aggs = [(AggregateFunc.Count, 1), (AggregateFunc.Sum, 1), (AggregateFunc.Min, 1), (AggregateFunc.Max, 1)]
    cases = {
        "v * 2.0": lambda: ctx.projection(t, [binop(v, Operator.Multiply, lit_f64(2.0)).flatten(f)]),
        "abs(v)": lambda: ctx.projection(t, [unop(UnaryOperator.Abs, v).flatten(f)]),
        "sin(v)": lambda: ctx.projection(t, [unop(UnaryOperator.Sin, v).flatten(f)]),
        "abs(v - 50.0)": lambda: ctx.projection(t, [unop(UnaryOperator.Abs, binop(v, Operator.Minus, lit_f64(50.0))).flatten(f)]),
        "select id where sin(v) * 2.0 > 0.5": lambda: ctx.selection_projection(t, sin_pred, [col(0).flatten(f)]),
        "count/sum/min/max(v) where cos(v) > 0.25 group by id % 7": lambda: ctx.aggregate(t, aggs, group_nodes=key, pred_nodes=cos_pred),
    }
    forms = {"one_pass": {"NQE_JIT_SYNC": "1"}, "node_at_a_time": {"NQE_NO_EXPR_TREE": "1"}}
    ctx.timing_enable(True)
    results = {}
    for name, run in cases.items():
        for form, env in forms.items():
            for k in ("NQE_JIT_SYNC", "NQE_NO_EXPR_TREE"):
                os.environ.pop(k, None)
            os.environ.update(env)
            times, kernels = [], {}
            for step in range(a.warmup + a.steps):
                ctx.timing_reset()
                out = run()
                ctx.synchronize()
                rep = ctx.timing_report()
                del out
                if step >= a.warmup:
                    times.append(sum(ms for ms, _ in rep.values()))
                    kernels = {k: round(ms, 4) for k, (ms, _) in rep.items()}
            med = statistics.median(times)
            results[f"{name} [{form}]"] = {"median_ms": round(med, 4), "min_ms": round(min(times), 4), "max_ms": round(max(times), 4),
                                           "gb_per_s_at_16_bytes_per_row": round(16.0 * n / med / 1e6, 1), "kernels_last_step_ms": kernels}
    os.makedirs(a.out, exist_ok=True)
    doc = {"rows": n, "steps": a.steps, "warmup": a.warmup, "results": results}
    with open(os.path.join(a.out, "probe.json"), "w") as fh:
        json.dump(doc, fh, indent=1)
    lines = [f"rows {n}, median of {a.steps} steps after {a.warmup} warm-up, HIP-event kernel times (ms); GB/s counts 16 B per row"]
    for k, r in results.items():
        lines.append(f"{k:78s} median {r['median_ms']:8.4f}  min {r['min_ms']:8.4f}  max {r['max_ms']:8.4f}  {r['gb_per_s_at_16_bytes_per_row']:8.1f} GB/s  {r['kernels_last_step_ms']}")
    with open(os.path.join(a.out, "probe.txt"), "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    ctx.close()


if __name__ == "__main__":
    main()
