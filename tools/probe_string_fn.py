#!/usr/bin/env python
"""Kernel times of the string functions (NQE_EXPR_STRING, quirk Q25) on one GPU, from HIP events through nqe_ctx_timing_*: one
process, warm-up, then the median of --steps executions of

    trim(s)  ltrim(s)  rtrim(s)  character_length(s)  lower(s)  upper(s)  reverse(s)

through nqe_expr_evaluate over two Utf8 columns — --rows strings of 5-20 bytes (the shape of profiles/r04/probe_strings.txt) and
--long-rows strings of 200 bytes — and, in the same process over the same columns, of an identity nqe_take (row i -> row i): the Utf8
gather that exists without this feature and that every one of these functions has to be compared with.  Next to each time, the bytes
the function's kernels have to read and write once (offsets, string bytes, outputs; what a kernel re-reads from cache is not counted).
Writes profiles/string_fn/README.md and probe.json (--out)."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_column(rng, n, lo, hi):
    """n strings of lo..hi bytes over letters of both cases, digits and inner spaces; half of them start with a space, half end with one"""
    from naive_query_engine_amd import Column, DType

    lens = rng.integers(lo, hi + 1, n).astype(np.int64)
    offs = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(lens, out=offs[1:])
    alphabet = np.frombuffer(b"abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789 ", dtype=np.uint8)
    data = alphabet[rng.integers(0, len(alphabet), int(offs[-1]))]
    lead, trail = rng.random(n) < 0.5, rng.random(n) < 0.5
    data[offs[:-1][lead]] = 0x20
    data[(offs[1:] - 1)[trail]] = 0x20
    return Column(DType.UTF8, n, offs.astype(np.int32), None, data)


def kept_bytes(col, front, back):
    """bytes a trim keeps, counted exactly on the host copy"""
    offs = col.values.astype(np.int64)
    data = col.data
    first, end = offs[:-1].copy(), offs[1:].copy()
    if front:
        while True:
            step = (first < end) & (data[np.minimum(first, len(data) - 1)] == 0x20)
            if not step.any():
                break
            first[step] += 1
    if back:
        while True:
            step = (end > first) & (data[np.maximum(end - 1, 0)] == 0x20)
            if not step.any():
                break
            end[step] -= 1
    return int((end - first).sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--long-rows", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "string_fn"))
    a = ap.parse_args()
    from naive_query_engine_amd import Column, UnaryOperator, capi
    from naive_query_engine_amd.expression import col, strop

    class F:
        name = "s"

    ctx = capi.Context(0)
    ctx.timing_enable(True)
    rng = np.random.default_rng(7)
    funcs = [UnaryOperator.Trim, UnaryOperator.LTrim, UnaryOperator.RTrim, UnaryOperator.CharacterLength, UnaryOperator.Lower, UnaryOperator.Upper, UnaryOperator.Reverse]
    doc = {"steps": a.steps, "warmup": a.warmup, "workloads": []}
    lines = ["# String functions (NQE_EXPR_STRING, quirk Q25): kernel times", "",
             f"`tools/probe_string_fn.py`: one process, {a.warmup} warm-up executions, then the median of {a.steps}; HIP-event kernel times from",
             "`nqe_ctx_timing_*` (the sum of a function's kernels, the scan's included), next to an identity `nqe_take` of the same column in the",
             "same process.  Bytes: what the function's kernels must read and write once (offsets 4 B per row, string bytes, outputs); GB/s is",
             "their sum over the time.", ""]
    for label, n, lo, hi in ((f"{a.rows} rows of 5-20 bytes", a.rows, 5, 20), (f"{a.long_rows} rows of 200 bytes", a.long_rows, 200, 200)):
        host = make_column(rng, n, lo, hi)
        B = int(host.data.size)
        t = ctx.table_from_host([host])
        idx = ctx.table_from_host([Column.from_numpy(np.arange(n, dtype=np.int64))])
        off = 4 * (n + 1)
        kept = {UnaryOperator.Trim: kept_bytes(host, True, True), UnaryOperator.LTrim: kept_bytes(host, True, False), UnaryOperator.RTrim: kept_bytes(host, False, True)}

        def traffic(func):
            if func in (UnaryOperator.Lower, UnaryOperator.Upper):
                return B, B                                      # a byte stream: no offsets
            if func == UnaryOperator.Reverse:
                return off + B, B
            if func == UnaryOperator.CharacterLength:
                return off + B, 8 * n
            k = kept[func]                                       # bounds: offsets + the ends; scan: lengths in and out; copy: both offsets, starts, kept bytes
            return off + (B - k) + off + (off + off + 4 * n + k), 8 * n + off + k

        cases = {f.name: (lambda f=f: ctx.expr_evaluate(t, strop(f, col(0)).flatten([F()]))) for f in funcs}
        cases["identity take"] = lambda: ctx.take(t, idx)
        rows = []
        for name, run in cases.items():
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
            if name == "identity take":
                rd, wr = 8 * n + off + off + (off + 8 * n + off + B), off + off + B  # lengths (idx, offsets), scan, copy (idx, both offsets, bytes)
            else:
                rd, wr = traffic(UnaryOperator[name])
            med = statistics.median(times)
            rows.append({"function": name, "median_ms": round(med, 4), "min_ms": round(min(times), 4), "max_ms": round(max(times), 4), "bytes_read": rd, "bytes_written": wr,
                         "gb_per_s": round((rd + wr) / med / 1e6, 1), "kernels_last_step_ms": kernels})
        take_ms = rows[-1]["median_ms"]
        for r in rows:
            r["vs_identity_take"] = round(r["median_ms"] / take_ms, 3)
        doc["workloads"].append({"workload": label, "rows": n, "string_bytes": B, "results": rows})
        lines += [f"## {label} ({B} string bytes)", "", "| function | median ms | min | max | MB read | MB written | GB/s | time / identity take | kernels of the last step (ms) |",
                  "|---|---|---|---|---|---|---|---|---|"]
        for r in rows:
            ks = ", ".join(f"`{k}` {v}" for k, v in r["kernels_last_step_ms"].items())
            lines.append(f"| {r['function']} | {r['median_ms']:.4f} | {r['min_ms']:.4f} | {r['max_ms']:.4f} | {r['bytes_read'] / 1e6:.1f} | {r['bytes_written'] / 1e6:.1f} | {r['gb_per_s']:.1f} | "
                         f"{r['vs_identity_take']:.3f} | {ks} |")
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
