#!/usr/bin/env python
"""Kernel times of the string functions with arguments (NQE_EXPR_STRING_ARGS, quirk Q26) on one GPU, from HIP events through
nqe_ctx_timing_*: one process, warm-up, then the median of --steps executions of

    substr(s, 1, 2)   substr(s, 3)   repeat(s, 3)
    replace(s, ' ', '_')  replace(s, ' ', '')  replace(s, ' ', '<sp>')      same length, shorter, longer
    replace(s, 'aa', 'b')  replace(s, 'ab', 'X')                            a bordered and a border-free pattern

through nqe_expr_evaluate over the two Utf8 columns of tools/probe_string_fn.py — --rows strings of 5-20 bytes and --long-rows strings of
200 bytes — and, in the same process over the same columns, of an identity nqe_take (row i -> row i): the Utf8 gather that exists
without this feature.  Where a form takes more than twice the take's time, the kernel that carries most of it is named.
Writes profiles/string_args/README.md and probe.json (--out)."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--long-rows", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "string_args"))
    a = ap.parse_args()
    from probe_string_fn import make_column

    from naive_query_engine_amd import Column, capi
    from naive_query_engine_amd.expression import col, repeat, replace, substr

    class F:
        name = "s"

    ctx = capi.Context(0)
    ctx.timing_enable(True)
    rng = np.random.default_rng(7)
    forms = [("substr(s, 1, 2)", substr(col(0), 1, 2)), ("substr(s, 3)", substr(col(0), 3)), ("repeat(s, 3)", repeat(col(0), 3)),
             ("replace(s, ' ', '_')  same length", replace(col(0), " ", "_")), ("replace(s, ' ', '')  shorter", replace(col(0), " ", "")),
             ("replace(s, ' ', '<sp>')  longer", replace(col(0), " ", "<sp>")), ("replace(s, 'aa', 'b')  bordered", replace(col(0), "aa", "b")),
             ("replace(s, 'ab', 'X')  border-free", replace(col(0), "ab", "X"))]
    doc = {"steps": a.steps, "warmup": a.warmup, "workloads": []}
    lines = ["# String functions with arguments (NQE_EXPR_STRING_ARGS, quirk Q26): kernel times", "",
             f"`tools/probe_string_args.py`: one process, {a.warmup} warm-up executions, then the median of {a.steps}; HIP-event kernel times from",
             "`nqe_ctx_timing_*` (the sum of a form's kernels, the scan's included), next to an identity `nqe_take` of the same column in the",
             "same process.  Measured on one MI355X box; the columns are those of `profiles/string_fn`.", ""]
    for label, n, lo, hi in ((f"{a.rows} rows of 5-20 bytes", a.rows, 5, 20), (f"{a.long_rows} rows of 200 bytes", a.long_rows, 200, 200)):
        host = make_column(rng, n, lo, hi)
        B = int(host.data.size)
        t = ctx.table_from_host([host])
        idx = ctx.table_from_host([Column.from_numpy(np.arange(n, dtype=np.int64))])
        cases = {name: (lambda e=e: ctx.expr_evaluate(t, e.flatten([F()]))) for name, e in forms}
        cases["identity take"] = lambda: ctx.take(t, idx)
        rows = []
        for name, run in cases.items():
            times, kernels, out_bytes = [], {}, 0
            for step in range(a.warmup + a.steps):
                ctx.timing_reset()
                out = run()
                ctx.synchronize()
                rep = ctx.timing_report()
                out_bytes = int(out.column_info(0).data_length)
                del out
                if step >= a.warmup:
                    times.append(sum(ms for ms, _ in rep.values()))
                    kernels = {k: round(ms, 4) for k, (ms, _) in rep.items()}
            rows.append({"form": name, "median_ms": round(statistics.median(times), 4), "min_ms": round(min(times), 4), "max_ms": round(max(times), 4), "result_bytes": out_bytes,
                         "kernels_last_step_ms": kernels})
        take_ms = rows[-1]["median_ms"]
        for r in rows:
            r["vs_identity_take"] = round(r["median_ms"] / take_ms, 3)
        doc["workloads"].append({"workload": label, "rows": n, "string_bytes": B, "results": rows})
        lines += [f"## {label} ({B} string bytes)", "", "| form | median ms | min | max | result MB | time / identity take | kernels of the last step (ms) |", "|---|---|---|---|---|---|---|"]
        for r in rows:
            ks = ", ".join(f"`{k}` {v}" for k, v in r["kernels_last_step_ms"].items())
            lines.append(f"| {r['form']} | {r['median_ms']:.4f} | {r['min_ms']:.4f} | {r['max_ms']:.4f} | {r['result_bytes'] / 1e6:.1f} | {r['vs_identity_take']:.3f} | {ks} |")
        lines.append("")
        slow = [r for r in rows if r["vs_identity_take"] > 2.0]
        for r in slow:
            k, ms = max(r["kernels_last_step_ms"].items(), key=lambda kv: kv[1])
            lines.append(f"* `{r['form'].split('  ')[0]}` takes {r['vs_identity_take']:.2f}x the take: `{k}` carries {ms:.4f} of its {r['median_ms']:.4f} ms.")
        if slow:
            lines.append("")
        del t, idx
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "probe.json"), "w") as fh:
        json.dump(doc, fh, indent=1)
    with open(os.path.join(a.out, "README.md"), "w") as fh:
        fh.write("\n".join(lines))
    print("\n".join(lines))
    ctx.close()


if __name__ == "__main__":
    main()
