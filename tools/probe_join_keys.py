#!/usr/bin/env python3
"""The hash join on several keys on the device (nqe_hash_join_build_keys / _probe_keys, csrc/join_keys.hip; quirk Q21): what the
tuple → code passes cost next to the join they feed.  HIP-event kernel time per call and per launch label (nqe_ctx_timing_report) and
the wall time of the call, over `--steps` steps after a warm-up.  The shape is the benchmark's C4: `--rows` probe rows against
`--build-rows` build rows, dense primary key / foreign key, one payload column on each side.

  two keys, packed      joined on (k / 1000, k % 1000): build = group_keys_ranges + group_keys_pack + the join's build,
                        probe = join_keys_pack_probe + the join's probe
  one key, by hand      the same join on the precomputed single key k (nqe_hash_join_build / _probe): the figure to compare against
  two keys, dictionary  the same two keys with NQE_JOIN_KEYS_FORCE_DICT=1: group_keys_dict / join_keys_lookup
  Utf8 + Int64          (8-byte string of k / 1000, k % 1000): the dictionary path with a string compare
  group by               nqe_group_aggregate_execute over the probe side's two key columns: group_keys_pack on the same memory, beside
                        join_keys_pack_probe
  execute                nqe_hash_join_execute_keys (build + probe per call) with every probe tuple inside the build's box, and with one
                        outside: what the abandoned all-match attempt costs

Bytes per row of the two new probe-side kernels: join_keys_pack_probe reads 8 K and writes 8; join_keys_lookup reads the key columns
(a Utf8 column: 4 bytes of offsets and its bytes) and writes 8, its table traffic not counted.  The share of 8 TB/s is those bytes over
the kernel's time.

Usage: python tools/probe_join_keys.py [--rows 100000000] [--build-rows 1000000] [--utf8-rows N] [--steps K] [--warmup W] [--out DIR]
(on a GPU machine; writes DIR/README.md and DIR/probe.json)
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from naive_query_engine_amd import AggregateFunc, Column, DType, capi  # noqa: E402
from naive_query_engine_amd.arrow_host import node_column  # noqa: E402

PEAK = 8e12  # bytes per second


def measure(ctx, call, steps, warmup):
    walls, reports, rows = [], [], 0
    for step in range(warmup + steps):
        ctx.synchronize()
        ctx.timing_reset()
        t0 = time.perf_counter()
        out = call()
        ctx.synchronize()
        wall = (time.perf_counter() - t0) * 1e3
        rpt = ctx.timing_report()
        rows = getattr(out[0] if isinstance(out, tuple) else out, "num_rows", 0)
        del out
        if step >= warmup:
            walls.append(wall)
            reports.append({k: v[0] for k, v in rpt.items()})
    return walls, reports, rows


def utf8_of(ids):
    """8-byte strings "k0000000" of the ids"""
    n = ids.size
    data = np.empty((n, 8), dtype=np.uint8)
    data[:, 0] = ord("k")
    rest = ids.copy()
    for p in range(7, 0, -1):
        data[:, p] = ord("0") + rest % 10
        rest //= 10
    return Column(DType.UTF8, n, (np.arange(n + 1, dtype=np.int64) * 8).astype(np.int32), None, data.reshape(-1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10 ** 8)
    ap.add_argument("--build-rows", type=int, default=10 ** 6)
    ap.add_argument("--utf8-rows", type=int, default=None, help="probe rows of the Utf8 + Int64 shape (default: --rows)")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "join_keys"))
    a = ap.parse_args()
    n, nb, nu = a.rows, a.build_rows, a.utf8_rows or a.rows
    os.makedirs(a.out, exist_ok=True)
    ctx = capi.Context(0)
    ctx.timing_enable(True)
    rng = np.random.default_rng(4)
    records = []

    def run(form, name, call, rows, kernel_bytes):
        walls, reports, out_rows = measure(ctx, call, a.steps, a.warmup)
        kern = [sum(r.values()) for r in reports]
        labels = sorted({k for r in reports for k in r})
        by_label = {k: float(np.median([r.get(k, 0.0) for r in reports])) for k in labels}
        shares = {k: b * rows / (by_label[k] * 1e-3) / PEAK for k, b in kernel_bytes.items() if by_label.get(k)}
        rec = dict(form=form, call=name, rows=rows, out_rows=out_rows, kernel_ms_median=float(np.median(kern)), kernel_ms_min=min(kern), kernel_ms_max=max(kern),
                   wall_ms_median=float(np.median(walls)), by_label_ms=by_label, bytes_per_row=kernel_bytes, share_of_8TBps=shares)
        records.append(rec)
        print(f"{form:>22} {name:>26} | out {out_rows:>10} kernels {rec['kernel_ms_median']:8.3f} ms [{min(kern):.3f}, {max(kern):.3f}] wall {rec['wall_ms_median']:8.3f} | "
              + " ".join(f"{k}={x:.3f}" for k, x in sorted(by_label.items(), key=lambda kv: -kv[1]) if x >= 0.0005)
              + " | " + " ".join(f"{k}: {s:.2f} of 8 TB/s" for k, s in shares.items()), flush=True)
        with open(os.path.join(a.out, "probe.json"), "w") as f:
            json.dump(records, f, indent=1)

    pk = rng.permutation(nb).astype(np.int64)
    fk = rng.integers(0, nb, n).astype(np.int64)
    i64 = Column.from_numpy
    left1 = ctx.table_from_host([i64(pk), i64(pk * 7)])
    right1 = ctx.table_from_host([i64(fk), i64(np.arange(n, dtype=np.int64))])
    left2 = ctx.table_from_host([i64(pk // 1000), i64(pk % 1000), i64(pk * 7)])
    right2 = ctx.table_from_host([i64(fk // 1000), i64(fk % 1000), i64(np.arange(n, dtype=np.int64))])

    run("one key, by hand", "build", lambda: ctx.hash_join_build(left1, 0), nb, {})
    jt = ctx.hash_join_build(left1, 0)
    run("one key, by hand", "probe", lambda: ctx.hash_join_probe(jt, right1, 0), n, {})
    del jt
    for form, env in (("two keys, packed", None), ("two keys, dictionary", "1")):
        if env:
            os.environ["NQE_JOIN_KEYS_FORCE_DICT"] = env
        try:
            run(form, "build", lambda: ctx.hash_join_build_keys(left2, [0, 1]), nb, {"group_keys_pack": 24, "group_keys_dict": 24})
            jt = ctx.hash_join_build_keys(left2, [0, 1])
        finally:
            os.environ.pop("NQE_JOIN_KEYS_FORCE_DICT", None)
        run(form, "probe", lambda: ctx.hash_join_probe_keys(jt, right2, [0, 1]), n, {"join_keys_pack_probe": 24, "join_keys_lookup": 24})
        del jt
    # group_keys_pack over the very same probe key columns: the stream join_keys_pack_probe is shaped after, on the same memory
    run("group by the probe keys", "group_aggregate", lambda: ctx.group_aggregate(right2, [[node_column(0)], [node_column(1)]], [(AggregateFunc.Count, 2)]), n,
        {"group_keys_pack": 24, "group_keys_ranges": 16})
    # the one-call inner form builds per call: the build side's codes fill their box without gaps, so its probe starts with the
    # optimistic all-match form; ONE probe tuple outside the box makes every call pay the abandoned attempt (no hint is kept for a
    # tuple table)
    run("two keys, packed", "execute, all inside", lambda: ctx.hash_join_keys(left2, right2, [0, 1], [0, 1]), n, {"join_keys_pack_probe": 24})
    a0, a1 = fk // 1000, fk % 1000
    a0[n - 1], a1[n - 1] = nb // 1000 + 1, 0
    right2_out = ctx.table_from_host([i64(a0), i64(a1), i64(np.arange(n, dtype=np.int64))])
    del a0, a1
    run("two keys, packed", "execute, one tuple outside", lambda: ctx.hash_join_keys(left2, right2_out, [0, 1], [0, 1]), n, {"join_keys_pack_probe": 24})
    del right2_out
    del left1, right1, left2, right2

    fku = fk[:nu]
    lefts = ctx.table_from_host([utf8_of(pk // 1000), i64(pk % 1000), i64(pk * 7)])
    rights = ctx.table_from_host([utf8_of(fku // 1000), i64(fku % 1000), i64(np.arange(nu, dtype=np.int64))])
    run("Utf8 (8 bytes) + Int64", "build", lambda: ctx.hash_join_build_keys(lefts, [0, 1]), nb, {"group_keys_dict": 28})
    jt = ctx.hash_join_build_keys(lefts, [0, 1])
    run("Utf8 (8 bytes) + Int64", "probe", lambda: ctx.hash_join_probe_keys(jt, rights, [0, 1]), nu, {"join_keys_lookup": 28})
    del jt, lefts, rights

    lines = ["# Join on several keys: what the tuple → code passes cost (`tools/probe_join_keys.py`)", "",
             f"One GPU, {n} probe rows ({nu} for the Utf8 shape) against {nb} build rows, dense primary key / foreign key; {a.steps} steps after {a.warmup} "
             "warm-up steps.  `kernels` is the sum of the HIP-event times of every launch of the call, median [min, max] over the steps.", "",
             "| form | call | output rows | kernels ms | wall ms | per launch label (median ms) | share of 8 TB/s |", "|---|---|---|---|---|---|---|"]
    for r in records:
        lines.append(f"| {r['form']} | {r['call']} | {r['out_rows']} | {r['kernel_ms_median']:.3f} [{r['kernel_ms_min']:.3f}, {r['kernel_ms_max']:.3f}] | {r['wall_ms_median']:.3f} | "
                     + ", ".join(f"`{k}` {x:.3f}" for k, x in sorted(r["by_label_ms"].items(), key=lambda kv: -kv[1]) if x >= 0.0005) + " | "
                     + ", ".join(f"`{k}` {s:.2f} ({r['bytes_per_row'][k]} B/row)" for k, s in r["share_of_8TBps"].items()) + " |")
    with open(os.path.join(a.out, "README.md"), "w") as f:
        f.write("\n".join(lines) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
