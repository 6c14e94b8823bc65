#!/usr/bin/env python
"""Kernel times of string matching (NQE_EXPR_STRING_MATCH, quirk Q27) on one GPU, from HIP events through nqe_ctx_timing_*: one process,
warm-up, then the median of --steps executions of

    like 'ab%'   like '%ab'   like 'ab%yz'   like 'ab'          the anchored forms (str_match_anchor)
    like '%ab%'  like 'a_c%'  like '%a%b%c%'  ilike '%AB%'  strpos(s, 'ab')      the scanning forms (str_match_scan)
    substr(s, 1, 2) = 'ab'                                       the composition a user had before

through nqe_expr_evaluate over the two Utf8 columns of tools/probe_string_fn.py — --rows strings of 5-20 bytes and --long-rows strings of
200 bytes — and, in the same process over the same columns, of what exists without this feature: `s = 'ab'` (utf8_compare: a lane per
row, a Boolean out), character_length(s) (every byte read once by the lane groups) and an identity nqe_take.
Two comparisons are drawn: the anchored forms against utf8_compare (a time above it by more than the run-to-run spread — the min-max of
the steps — is flagged), and the scanning forms against character_length (above twice its time the kernel is named).
Writes profiles/string_match/README.md and probe.json (--out); the hand-written reading of the numbers, ANALYSIS.md beside them, is left alone."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

ANCHORED = ("like 'ab%'", "like '%ab'", "like 'ab%yz'", "like 'ab'")
SCANNING = ("like '%ab%'", "like 'a_c%'", "like '%a%b%c%'", "ilike '%AB%'", "strpos(s, 'ab')")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--long-rows", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "string_match"))
    a = ap.parse_args()
    from probe_string_fn import make_column

    from naive_query_engine_amd import Column, Operator, UnaryOperator, capi
    from naive_query_engine_amd.expression import binop, col, ilike, like, lit_utf8, strop, strpos, substr

    class F:
        name = "s"

    ctx = capi.Context(0)
    ctx.timing_enable(True)
    rng = np.random.default_rng(7)
    s = col(0)
    forms = [("like 'ab%'", like(s, "ab%")), ("like '%ab'", like(s, "%ab")), ("like 'ab%yz'", like(s, "ab%yz")), ("like 'ab'", like(s, "ab")), ("like '%ab%'", like(s, "%ab%")),
             ("like 'a_c%'", like(s, "a_c%")), ("like '%a%b%c%'", like(s, "%a%b%c%")), ("ilike '%AB%'", ilike(s, "%AB%")), ("strpos(s, 'ab')", strpos(s, "ab")),
             ("substr(s, 1, 2) = 'ab'", binop(substr(s, 1, 2), Operator.Eq, lit_utf8("ab"))), ("s = 'ab'  (utf8_compare)", binop(s, Operator.Eq, lit_utf8("ab"))),
             ("character_length(s)", strop(UnaryOperator.CharacterLength, s))]
    doc = {"steps": a.steps, "warmup": a.warmup, "workloads": []}
    lines = ["# String matching (NQE_EXPR_STRING_MATCH, quirk Q27): kernel times", "",
             f"`tools/probe_string_match.py`: one process, {a.warmup} warm-up executions, then the median of {a.steps}; HIP-event kernel times from",
             "`nqe_ctx_timing_*` (the sum of a form's kernels), next to `s = 'ab'` (`utf8_compare`), `character_length(s)` and an identity `nqe_take`",
             "of the same column in the same process.  Measured on one MI355X box; the columns are those of `profiles/string_fn`.", ""]
    for label, n, lo, hi in ((f"{a.rows} rows of 5-20 bytes", a.rows, 5, 20), (f"{a.long_rows} rows of 200 bytes", a.long_rows, 200, 200)):
        host = make_column(rng, n, lo, hi)
        B = int(host.data.size)
        t = ctx.table_from_host([host])
        idx = ctx.table_from_host([Column.from_numpy(np.arange(n, dtype=np.int64))])
        cases = {name: (lambda e=e: ctx.expr_evaluate(t, e.flatten([F()]))) for name, e in forms}
        cases["identity take"] = lambda: ctx.take(t, idx)
        rows = []
        for name, run in cases.items():
            times, kernels, hits = [], {}, None
            for step in range(a.warmup + a.steps):
                ctx.timing_reset()
                out = run()
                ctx.synchronize()
                rep = ctx.timing_report()
                if step == 0 and name != "identity take" and name != "character_length(s)":
                    got = out.to_host()[0].to_numpy()
                    hits = int((got != 0).sum())  # rows that match (strpos: rows with an occurrence)
                del out
                if step >= a.warmup:
                    times.append(sum(ms for ms, _ in rep.values()))
                    kernels = {k: round(ms, 4) for k, (ms, _) in rep.items()}
            rows.append({"form": name, "median_ms": round(statistics.median(times), 4), "min_ms": round(min(times), 4), "max_ms": round(max(times), 4), "matching_rows": hits,
                         "kernels_last_step_ms": kernels})
        by = {r["form"]: r for r in rows}
        cmp_r, len_r, take_r = by["s = 'ab'  (utf8_compare)"], by["character_length(s)"], by["identity take"]
        for r in rows:
            r["vs_utf8_compare"] = round(r["median_ms"] / cmp_r["median_ms"], 3)
            r["vs_character_length"] = round(r["median_ms"] / len_r["median_ms"], 3)
            r["vs_identity_take"] = round(r["median_ms"] / take_r["median_ms"], 3)
        doc["workloads"].append({"workload": label, "rows": n, "string_bytes": B, "results": rows})
        lines += [f"## {label} ({B} string bytes)", "", "| form | median ms | min | max | matching rows | / utf8_compare | / character_length | / identity take | kernels of the last step (ms) |",
                  "|---|---|---|---|---|---|---|---|---|"]
        for r in rows:
            ks = ", ".join(f"`{k}` {v}" for k, v in r["kernels_last_step_ms"].items())
            hits = "" if r["matching_rows"] is None else str(r["matching_rows"])
            lines.append(f"| {r['form']} | {r['median_ms']:.4f} | {r['min_ms']:.4f} | {r['max_ms']:.4f} | {hits} | {r['vs_utf8_compare']:.3f} | {r['vs_character_length']:.3f} | "
                         f"{r['vs_identity_take']:.3f} | {ks} |")
        lines.append("")
        # the anchored forms against utf8_compare: the same offsets, fewer bytes.  The spread is the widest min-max of the rows compared.
        spread = max(r["max_ms"] - r["min_ms"] for r in rows if r["form"] in ANCHORED or r is cmp_r)
        lines.append(f"Anchored forms against `utf8_compare` ({cmp_r['median_ms']:.4f} ms; run-to-run spread, the widest min-max of these rows: {spread:.4f} ms):")
        lines.append("")
        for name in ANCHORED:
            r = by[name]
            d = r["median_ms"] - cmp_r["median_ms"]
            verdict = "ABOVE utf8_compare by more than the spread" if d > spread else "within the spread of utf8_compare" if d >= -spread else "below utf8_compare"
            lines.append(f"* `{name}`: {r['median_ms']:.4f} ms, {d:+.4f} ms: {verdict}.")
        lines.append("")
        lines.append(f"Scanning forms against `character_length` ({len_r['median_ms']:.4f} ms: every byte read once):")
        lines.append("")
        for name in SCANNING:
            r = by[name]
            k, ms = max(r["kernels_last_step_ms"].items(), key=lambda kv: kv[1])
            tail = f" — more than twice: `{k}` carries {ms:.4f} of its {r['median_ms']:.4f} ms" if r["vs_character_length"] > 2.0 else ""
            lines.append(f"* `{name}`: {r['vs_character_length']:.2f}x{tail}.")
        lines.append("")
        del t, idx
    lines += ["What these numbers say — the two comparisons explained — is in `ANALYSIS.md` beside this file (written by hand; the probe does not touch it).", ""]
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "probe.json"), "w") as fh:
        json.dump(doc, fh, indent=1)
    with open(os.path.join(a.out, "README.md"), "w") as fh:
        fh.write("\n".join(lines))
    print("\n".join(lines))
    ctx.close()


if __name__ == "__main__":
    main()
