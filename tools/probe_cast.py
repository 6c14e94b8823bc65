#!/usr/bin/env python
"""Kernel times of the cast node (NQE_EXPR_CAST, quirk Q29) on one GPU, from HIP events through nqe_ctx_timing_*: one process, warm-up,
then min / median / max of --steps executions, every family next to an existing node of equal traffic taken in the same process over
the same columns.  A form and its yardstick ALTERNATE step by step, so that both see the same clocks and the same neighbours; the
yardstick's own run-to-run spread (max - min over its steps) is the margin: a form whose median differs from its yardstick's by more
than that is flagged, and why is ANALYSIS.md's business (written by hand beside the output; the probe does not touch it).

    cast(id as double)   cast(v as bigint)                    beside  v * 2.0            (16 B/row each)              cast_fixed
    cast(b as bigint)    cast(v as boolean)                   beside  is_null(v), not(b)                               cast_fixed
    cast(id as double) * 1.5  (two passes)                    beside  v * 2.0            (the case for a one-pass cast)
    cast(s as bigint)    cast(s as double)                    beside  character_length(s) (the same bytes read once)
                                                              and     the CSV reader's parse of the same bytes as one column   cast_parse
    cast(id as varchar)                                       beside  an identity nqe_take of the result       cast_text_lengths + scan + cast_text_write

over --rows rows and --str-rows strings of 1-19 digits.  Writes README.md and probe.json to --out (default profiles/cast)."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def one(ctx, run):
    ctx.timing_reset()
    out = run()
    ctx.synchronize()
    rep = ctx.timing_report()
    del out
    return sum(ms for ms, _ in rep.values()), {k: round(ms, 4) for k, (ms, _) in rep.items()}


def alternating(ctx, runs, warmup, steps):
    """runs: {name: callable}; every step executes each once, in order"""
    times, kernels = {k: [] for k in runs}, {}
    for step in range(warmup + steps):
        for name, run in runs.items():
            ms, ks = one(ctx, run)
            if step >= warmup:
                times[name].append(ms)
                kernels[name] = ks
    return {name: {"form": name, "median_ms": round(statistics.median(t), 4), "min_ms": round(min(t), 4), "max_ms": round(max(t), 4), "spread_ms": round(max(t) - min(t), 4),
                   "kernels_last_step_ms": kernels[name]} for name, t in times.items()}


def table(lines, rows, yard_name):
    y = rows[yard_name]
    lines += ["| form | bytes / row | median ms | min | max | spread | ratio to the yardstick | outside the yardstick's spread | kernels of the last step (ms) |", "|---|---|---|---|---|---|---|---|---|"]
    for r in rows.values():
        r["ratio"] = round(r["median_ms"] / y["median_ms"], 3)
        r["outside_yardstick_spread"] = bool(abs(r["median_ms"] - y["median_ms"]) > y["spread_ms"])
        ks = ", ".join(f"`{k}` {ms}" for k, ms in r["kernels_last_step_ms"].items())
        mark = "(yardstick)" if r["form"] == yard_name else ("yes" if r["outside_yardstick_spread"] else "no")
        lines.append(f"| `{r['form']}` | {r.get('bytes_per_row', '')} | {r['median_ms']:.4f} | {r['min_ms']:.4f} | {r['max_ms']:.4f} | {r['spread_ms']:.4f} | {r['ratio']:.3f} | {mark} | {ks} |")
    lines.append("")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--str-rows", type=int, default=10_000_000)
    ap.add_argument("--steps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cast"))
    a = ap.parse_args()

    from naive_query_engine_amd import Column, DType, Operator, UnaryOperator, capi
    from naive_query_engine_amd.expression import PhysicalStringExpr, binop, cast, col, is_null, lit_f64, not_

    ctx = capi.Context(0)
    ctx.timing_enable(True)
    rng = np.random.default_rng(7)
    n = a.rows
    doc = {"steps": a.steps, "warmup": a.warmup, "alternating": True, "workloads": []}
    lines = ["# Casts (NQE_EXPR_CAST, quirk Q29): kernel times", "",
             f"`tools/probe_cast.py`: one process, {a.warmup} warm-up steps, then min / median / max of {a.steps} steps; within a step a form and its yardstick run one after the other",
             "(alternating), HIP-event kernel times from `nqe_ctx_timing_*` (the sum of a form's kernels).  Measured on one MI355X box.  Bytes per row: what the algorithm has to move.", ""]

    # ---- words and bits
    fields = [type("F", (), {"name": nm})() for nm in ("id", "v", "b")]
    cols = [Column.from_numpy(rng.integers(-(1 << 40), 1 << 40, n).astype(np.int64)), Column.from_numpy((rng.random(n) - 0.5) * 1e6), Column.from_numpy(rng.random(n) < 0.5, rng.random(n) >= 0.3)]
    t = ctx.table_from_host(cols)
    del cols
    ID, V, B = (col(i) for i in range(3))
    ev = lambda e: (lambda: ctx.expr_evaluate(t, e.flatten(fields)))  # noqa: E731
    bit = 1.0 / 8.0
    groups = [("16 B/row: word to word", "v * 2.0", {"v * 2.0": (binop(V, Operator.Multiply, lit_f64(2.0)), 16), "cast(id as double)": (cast(ID, DType.FLOAT64), 16),
                                                      "cast(v as bigint)": (cast(V, DType.INT64), 16 + bit), "cast(id as double) * 1.5  (two passes)": (binop(cast(ID, DType.FLOAT64), Operator.Multiply, lit_f64(1.5)), 32)}),
              ("the Boolean casts", "is_null(v)", {"is_null(v)": (is_null(V), bit), "not(b)": (not_(B), 4 * bit), "cast(b as bigint)": (cast(B, DType.INT64), 2 * bit + 8),
                                                   "cast(v as boolean)": (cast(V, DType.BOOLEAN), 8 + bit)})]
    for title, yname, forms in groups:
        rows = alternating(ctx, {k: ev(e) for k, (e, _) in forms.items()}, a.warmup, a.steps)
        for k, (_, bpr) in forms.items():
            rows[k]["bytes_per_row"] = round(bpr, 3)
            rows[k]["gb_per_s"] = round(bpr * n / rows[k]["median_ms"] / 1e6, 1)
        lines += [f"## {n} rows, {title} (yardstick `{yname}`)", ""]
        table(lines, rows, yname)
        doc["workloads"].append({"workload": f"{n} rows, {title}", "rows": n, "yardstick": yname, "results": list(rows.values())})
    del t

    # ---- Utf8 -> word: strings of 1-19 digits
    m = a.str_rows
    digits = rng.integers(1, 20, m)
    ints = (rng.random(m) * (10.0 ** digits)).astype(np.uint64) % np.uint64(1 << 63)
    texts = [b"%d" % int(x) for x in ints]
    offs = np.zeros(m + 1, dtype=np.int32)
    offs[1:] = np.cumsum([len(s) for s in texts])
    data = b"".join(texts)
    s_col = Column(DType.UTF8, m, offs, None, np.frombuffer(data, dtype=np.uint8).copy())
    st = ctx.table_from_host([s_col])
    sf = [type("F", (), {"name": "s"})()]
    S = col(0)
    csv_bytes = b"\n".join(texts) + b"\n"
    del texts
    sev = lambda e: (lambda: ctx.expr_evaluate(st, e.flatten(sf)))  # noqa: E731
    runs = {"character_length(s)": sev(PhysicalStringExpr.create(S, UnaryOperator.CharacterLength)), "cast(s as bigint)": sev(cast(S, DType.INT64)), "cast(s as double)": sev(cast(S, DType.FLOAT64)),
            "csv reader: the same bytes as one Int64 column": lambda: ctx.csv_read(csv_bytes, [DType.INT64], False, ",", m + 1),
            "csv reader: the same bytes as one Float64 column": lambda: ctx.csv_read(csv_bytes, [DType.FLOAT64], False, ",", m + 1)}
    rows = alternating(ctx, runs, a.warmup, a.steps)
    mean = len(data) / m
    for k in rows:
        rows[k]["bytes_per_row"] = round(8 + mean + (0 if k.startswith("csv") else 8) + (0 if "length" in k else 1.0 / 8), 2) if not k.startswith("csv") else round(mean + 1 + 8, 2)
    lines += [f"## {m} strings of 1-19 digits (mean {mean:.1f} bytes) to a word (yardstick `character_length(s)`: the same offsets and bytes read once, 8 bytes written)", ""]
    table(lines, rows, "character_length(s)")
    doc["workloads"].append({"workload": f"{m} strings of 1-19 digits", "rows": m, "mean_bytes": mean, "yardstick": "character_length(s)", "results": list(rows.values())})
    del st

    # ---- Int64 -> Utf8
    it = ctx.table_from_host([Column.from_numpy(ints.astype(np.int64) * np.where(rng.random(m) < 0.5, 1, -1))])
    idf = [type("F", (), {"name": "id"})()]
    result = ctx.expr_evaluate(it, cast(col(0), DType.UTF8).flatten(idf))
    out_bytes = int(result.column_info(0).data_length)
    idx = ctx.table_from_host([Column.from_numpy(np.arange(m, dtype=np.int64))])
    rows = alternating(ctx, {"identity take of the result": lambda: ctx.take(result, idx), "cast(id as varchar)": lambda: ctx.expr_evaluate(it, cast(col(0), DType.UTF8).flatten(idf))}, a.warmup, a.steps)
    rows["cast(id as varchar)"]["bytes_per_row"] = round(8 + 4 + 8 + 4 + 4 + out_bytes / m, 2)  # the word twice, a length out and in, an offset out and in, the bytes out
    rows["identity take of the result"]["bytes_per_row"] = round(8 + 8 + 4 + 4 + 4 + 2.0 * out_bytes / m, 2)
    lines += [f"## {m} Int64 rows to text ({out_bytes} result bytes; yardstick: an identity `nqe_take` of the result)", ""]
    table(lines, rows, "identity take of the result")
    doc["workloads"].append({"workload": f"{m} Int64 rows to text", "rows": m, "result_bytes": out_bytes, "yardstick": "identity take of the result", "results": list(rows.values())})

    lines += ["What these numbers say — every ratio outside its yardstick's spread explained — is in `ANALYSIS.md` beside this file (written by hand; the probe does not touch it).", ""]
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "probe.json"), "w") as fh:
        json.dump(doc, fh, indent=1)
    with open(os.path.join(a.out, "README.md"), "w") as fh:
        fh.write("\n".join(lines))
    print("\n".join(lines))
    ctx.close()


if __name__ == "__main__":
    main()
