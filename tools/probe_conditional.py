#!/usr/bin/env python
"""Kernel times of the conditional and NULL-handling functions (NQE_EXPR_CONDITIONAL, quirk Q28) on one GPU, from HIP events through
nqe_ctx_timing_*: one process, warm-up, then min / median / max of --steps executions of

    coalesce(v, 0.0)   if(b, v, w)   if(v > 50, 1, 0) (two nodes)   nullif(id, 0)        cond_words
    not(b)   is_null(v)                                                                  cond_bits

over --rows rows (v: Float64 with ~30 % NULLs, w: Float64, id: Int64, b: Boolean with NULLs, b2: Boolean), each next to a yardstick taken in
the same process over the same columns — the existing binary node of equal traffic: `v + w` for two word inputs, `v * 2.0` for one,
`b and b2` for the bit forms — which is executed 3 x --steps times so that its own run-to-run spread (max - min) is known; and of

    coalesce(s, 'unknown')   if(b, s, t)                                                 cond_str_lengths + scan + cond_str_copy

over --str-rows strings of 5-20 bytes and --long-rows strings of 200 bytes (s with ~30 % NULLs), next to an identity nqe_take of the
RESULT column (the same result bytes), the yardstick of the other string sections.  Bytes per row are what the algorithm has to move,
computed here from the shapes.  A form whose median differs from its yardstick's by more than that yardstick's spread is flagged; why, is
ANALYSIS.md's business (written by hand beside the output; the probe does not touch it).
Writes profiles/conditional/README.md and probe.json (--out)."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def timed(ctx, run, warmup, steps):
    times, kernels = [], {}
    for step in range(warmup + steps):
        ctx.timing_reset()
        out = run()
        ctx.synchronize()
        rep = ctx.timing_report()
        del out
        if step >= warmup:
            times.append(sum(ms for ms, _ in rep.values()))
            kernels = {k: round(ms, 4) for k, (ms, _) in rep.items()}
    return {"median_ms": round(statistics.median(times), 4), "min_ms": round(min(times), 4), "max_ms": round(max(times), 4), "kernels_last_step_ms": kernels}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--str-rows", type=int, default=10_000_000)
    ap.add_argument("--long-rows", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "conditional"))
    a = ap.parse_args()
    from probe_string_fn import make_column

    from naive_query_engine_amd import Column, Operator, capi
    from naive_query_engine_amd.arrow_host import pack_bits
    from naive_query_engine_amd.expression import binop, coalesce, col, if_else, is_null, lit_f64, lit_i64, lit_utf8, not_, nullif

    ctx = capi.Context(0)
    ctx.timing_enable(True)
    rng = np.random.default_rng(7)
    n = a.rows
    doc = {"steps": a.steps, "warmup": a.warmup, "yardstick_steps": 3 * a.steps, "workloads": []}
    lines = ["# Conditional and NULL-handling functions (NQE_EXPR_CONDITIONAL, quirk Q28): kernel times", "",
             f"`tools/probe_conditional.py`: one process, {a.warmup} warm-up executions, then min / median / max of {a.steps} ({3 * a.steps} for a yardstick); HIP-event kernel",
             "times from `nqe_ctx_timing_*` (the sum of a form's kernels).  Measured on one MI355X box.  Bytes per row: what the algorithm has to move.", ""]

    # ---- words and bits
    names = ["v", "w", "id", "b", "b2"]
    fields = [type("F", (), {"name": nm})() for nm in names]
    v = rng.random(n) * 100.0
    cols = [Column.from_numpy(v, rng.random(n) >= 0.3), Column.from_numpy(rng.random(n) * 100.0), Column.from_numpy(rng.integers(0, 4, n).astype(np.int64)),
            Column.from_numpy(rng.random(n) < 0.5, rng.random(n) >= 0.3), Column.from_numpy(rng.random(n) < 0.5)]
    del v
    t = ctx.table_from_host(cols)
    del cols
    V, W, ID, B, B2 = (col(i) for i in range(5))
    bit = 1.0 / 8.0
    yard = {"v + w": (binop(V, Operator.Plus, W), 8 + bit + 8 + 8 + bit), "v * 2.0": (binop(V, Operator.Multiply, lit_f64(2.0)), 8 + bit + 8 + bit),
            "b and b2": (binop(B, Operator.And, B2), 4 * bit + bit)}
    forms = [("coalesce(v, 0.0)", coalesce(V, lit_f64(0.0)), 8 + bit + 8, "v * 2.0"), ("if(b, v, w)", if_else(B, V, W), 2 * bit + 8 + bit + 8 + 8 + bit, "v + w"),
             ("if(v > 50, 1, 0)  (two nodes)", if_else(binop(V, Operator.Gt, lit_f64(50.0)), lit_i64(1), lit_i64(0)), (8 + bit + 2 * bit) + (2 * bit + 8), "v * 2.0"),
             ("nullif(id, 0)", nullif(ID, lit_i64(0)), 8 + 8 + bit, "v * 2.0"), ("not(b)", not_(B), 2 * bit + 2 * bit, "b and b2"), ("is_null(v)", is_null(V), bit + bit, "b and b2")]
    yard_rows = {}
    for name, (e, bpr) in yard.items():
        r = timed(ctx, lambda e=e: ctx.expr_evaluate(t, e.flatten(fields)), a.warmup, 3 * a.steps)
        r.update({"form": name, "bytes_per_row": round(bpr, 3), "spread_ms": round(r["max_ms"] - r["min_ms"], 4)})
        yard_rows[name] = r
    rows = []
    for name, e, bpr, yname in forms:
        r = timed(ctx, lambda e=e: ctx.expr_evaluate(t, e.flatten(fields)), a.warmup, a.steps)
        y = yard_rows[yname]
        r.update({"form": name, "bytes_per_row": round(bpr, 3), "yardstick": yname, "ratio": round(r["median_ms"] / y["median_ms"], 3),
                  "outside_yardstick_spread": bool(abs(r["median_ms"] - y["median_ms"]) > y["spread_ms"]), "gb_per_s": round(bpr * n / r["median_ms"] / 1e6, 1)})
        rows.append(r)
    doc["workloads"].append({"workload": f"{n} rows", "rows": n, "yardsticks": list(yard_rows.values()), "results": rows})
    lines += [f"## {n} rows: words and bits", "", "| yardstick (existing binary node) | bytes / row | median ms | min | max | spread (max - min) | kernels of the last step (ms) |", "|---|---|---|---|---|---|---|"]
    for y in yard_rows.values():
        ks = ", ".join(f"`{k}` {ms}" for k, ms in y["kernels_last_step_ms"].items())
        lines.append(f"| `{y['form']}` | {y['bytes_per_row']} | {y['median_ms']:.4f} | {y['min_ms']:.4f} | {y['max_ms']:.4f} | {y['spread_ms']:.4f} | {ks} |")
    lines += ["", "| form | bytes / row | median ms | min | max | GB/s | yardstick | ratio | outside the yardstick's spread | kernels of the last step (ms) |", "|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        ks = ", ".join(f"`{k}` {ms}" for k, ms in r["kernels_last_step_ms"].items())
        lines.append(f"| `{r['form']}` | {r['bytes_per_row']} | {r['median_ms']:.4f} | {r['min_ms']:.4f} | {r['max_ms']:.4f} | {r['gb_per_s']} | `{r['yardstick']}` | {r['ratio']:.3f} | "
                     f"{'yes' if r['outside_yardstick_spread'] else 'no'} | {ks} |")
    lines.append("")
    del t

    # ---- Utf8
    sfields = [type("F", (), {"name": nm})() for nm in ("s", "t", "b")]
    S, T, SB = col(0), col(1), col(2)
    for label, m, lo, hi in ((f"{a.str_rows} strings of 5-20 bytes", a.str_rows, 5, 20), (f"{a.long_rows} strings of 200 bytes", a.long_rows, 200, 200)):
        s_host, t_host = make_column(rng, m, lo, hi), make_column(rng, m, lo, hi)
        s_host.validity = pack_bits(rng.random(m) >= 0.3)
        st = ctx.table_from_host([s_host, t_host, Column.from_numpy(rng.random(m) < 0.5)])
        idx = ctx.table_from_host([Column.from_numpy(np.arange(m, dtype=np.int64))])
        rows = []
        for name, e in (("coalesce(s, 'unknown')", coalesce(S, lit_utf8("unknown"))), ("if(b, s, t)", if_else(SB, S, T))):
            result = ctx.expr_evaluate(st, e.flatten(sfields))
            out_bytes = int(result.column_info(0).data_length)
            r = timed(ctx, lambda e=e: ctx.expr_evaluate(st, e.flatten(sfields)), a.warmup, a.steps)
            y = timed(ctx, lambda: ctx.take(result, idx), a.warmup, 3 * a.steps)
            # per row: two offsets in, one source byte and one length out and in again, one offset out, the bytes in and out (validity bits aside)
            bpr = (4 + 4) + (1 + 4) + (1 + 4) + 4 + 2.0 * out_bytes / m
            r.update({"form": name, "result_bytes": out_bytes, "bytes_per_row": round(bpr, 2), "yardstick": "identity take of the result", "yardstick_median_ms": y["median_ms"],
                      "yardstick_min_ms": y["min_ms"], "yardstick_max_ms": y["max_ms"], "yardstick_spread_ms": round(y["max_ms"] - y["min_ms"], 4),
                      "yardstick_kernels_last_step_ms": y["kernels_last_step_ms"], "ratio": round(r["median_ms"] / y["median_ms"], 3),
                      "outside_yardstick_spread": bool(abs(r["median_ms"] - y["median_ms"]) > y["max_ms"] - y["min_ms"])})
            rows.append(r)
            del result
        doc["workloads"].append({"workload": label, "rows": m, "results": rows})
        lines += [f"## {label}", "", "| form | result bytes | bytes / row | median ms | min | max | identity take of the result: median ms | min | max | ratio | outside the yardstick's spread | kernels of the last step (ms) |",
                  "|---|---|---|---|---|---|---|---|---|---|---|---|"]
        for r in rows:
            ks = ", ".join(f"`{k}` {ms}" for k, ms in r["kernels_last_step_ms"].items())
            lines.append(f"| `{r['form']}` | {r['result_bytes']} | {r['bytes_per_row']} | {r['median_ms']:.4f} | {r['min_ms']:.4f} | {r['max_ms']:.4f} | {r['yardstick_median_ms']:.4f} | "
                         f"{r['yardstick_min_ms']:.4f} | {r['yardstick_max_ms']:.4f} | {r['ratio']:.3f} | {'yes' if r['outside_yardstick_spread'] else 'no'} | {ks} |")
        lines.append("")
        del st, idx
    lines += ["What these numbers say — every ratio outside its yardstick's spread explained from the bytes and the instruction mix — is in `ANALYSIS.md` beside this file (written by hand;",
              "the probe does not touch it).", ""]
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "probe.json"), "w") as fh:
        json.dump(doc, fh, indent=1)
    with open(os.path.join(a.out, "README.md"), "w") as fh:
        fh.write("\n".join(lines))
    print("\n".join(lines))
    ctx.close()


if __name__ == "__main__":
    main()
