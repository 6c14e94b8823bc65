#!/usr/bin/env python3
"""DISTINCT and the set operators on the device (nqe_distinct_execute / nqe_set_op_execute, csrc/set_ops.hip): the kernel time of a
call and its split over the launch labels, read from nqe_ctx_timing_*, and beside every shape, in the same process on the same box:

  window route   the existing device route to the same rows: row_number() over (partition by the key columns), then a selection of
                 `row_number = 1` (DISTINCT shapes only)
  floor          a plain selection `id < kept` over the same table: the same number of rows kept, the same columns compacted

  DISTINCT shapes (every table also carries the row number `id` as a payload column)
    i64_1e3 / i64_1e6 / i64_all   one Int64 key with 10^3 / 10^6 / n different values
    i64_one                        one Int64 key with ONE value: every row lowers the same `first` (the contention case).  Without the
                                   read before the atomicMin: a variant build, and this tool against it —
                                     NQE_VARIANT_UNITS=set_ops tools/build_variant.sh noskip -DNQE_SET_NO_FIRST_SKIP
                                     NQE_LIB_PATH=naive_query_engine_amd/libnqe_hip_noskip.so python tools/probe_set_ops.py --shapes i64_one --out DIR
    two_i64                        two Int64 keys, 10^3 x 10^3 tuples
    utf8_1e6                       one Utf8 key of 8 bytes, 10^6 different strings
    five_dtypes                    Int64, UInt64, Float64, Boolean, Utf8, each with 10 % NULLs
  set-op shape: INTERSECT and EXCEPT of n left rows (one Int64 column, 2 x 10^6 different values) against 10^6 right rows (half of them)

Usage: python tools/probe_set_ops.py [--rows 100000000] [--reps K] [--shapes a,b] [--out DIR]   (on a GPU machine; writes DIR/probe.txt and DIR/probe.json)
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from naive_query_engine_amd import (Column, ColumnExpr, DType, Field, Operator, PhysicalBinaryExpr, PhysicalLiteralExpr, ScalarValue, SetOp, WindowFunc as W,  # noqa: E402
                                    capi)
from naive_query_engine_amd.arrow_host import pack_bits  # noqa: E402

SET_LABELS = ("set_table_init", "set_insert", "set_find", "set_keep", "set_null_count")
MIX = 0x9E3779B1


def hex8_column(values, mask=None):
    """a Utf8 column of 8 hexadecimal digits per row (built in chunks: the digit matrix of 10^8 rows at once would be 6 GB)"""
    n = values.size
    data = np.empty(n * 8, dtype=np.uint8)
    digits = np.frombuffer(b"0123456789abcdef", dtype=np.uint8)
    shifts = np.arange(28, -4, -4, dtype=np.uint64)
    for a in range(0, n, 1 << 24):
        v = values[a:a + (1 << 24)].astype(np.uint64)
        data[a * 8:(a + v.size) * 8] = digits[((v[:, None] >> shifts[None, :]) & np.uint64(15)).astype(np.intp)].ravel()
    col = Column(DType.UTF8, n, np.arange(0, 8 * n + 1, 8, dtype=np.int32), None, data)
    if mask is not None:
        col.validity = pack_bits(mask)
    return col


def shapes(n, rng):
    ids = np.arange(n, dtype=np.int64)
    mixed = (ids * MIX) & 0xFFFFFFFF
    i = Column.from_numpy
    yield "i64_1e3", lambda: [i(mixed % 1000)]
    yield "i64_1e6", lambda: [i(mixed % 1_000_000)]
    yield "i64_all", lambda: [i(ids * 0x9E3779B97F4A7C1)]
    yield "i64_one", lambda: [i(np.full(n, 42, dtype=np.int64))]
    yield "two_i64", lambda: [i(mixed % 1000), i(mixed // 1000 % 1000)]
    yield "utf8_1e6", lambda: [hex8_column(mixed % 1_000_000)]
    nulls = lambda: rng.random(n) > 0.1
    f = np.array([0.0, -0.0, np.nan, 1.5, -2.5, np.inf, 7.0], dtype=np.float64)
    yield "five_dtypes", lambda: [i(mixed % 100, nulls()), i((mixed // 100 % 100).astype(np.uint64), nulls()), i(f[mixed % 7], nulls()), i(mixed % 2 == 0, nulls()),
                                  hex8_column(mixed // 7 % 50, nulls())]


def timed(ctx, fn, reps):
    """(median wall ms, {label: median ms}, {label: launches}, the last result) over `reps` runs after a warm-up"""
    walls, reports, out = [], [], None
    for rep in range(reps + 1):
        out = None
        ctx.synchronize()
        ctx.timing_reset()
        t0 = time.perf_counter()
        out = fn()
        ctx.synchronize()
        wall = (time.perf_counter() - t0) * 1e3
        if rep:
            walls.append(wall)
            reports.append(ctx.timing_report())
    names = sorted({k for r in reports for k in r})
    med = {k: float(np.median([r.get(k, (0.0, 0))[0] for r in reports])) for k in names}
    cnt = {k: reports[-1].get(k, (0.0, 0))[1] for k in names}
    return float(np.median(walls)), med, cnt, out


def run(ctx, n, reps, say, only):
    rng = np.random.default_rng(1)
    rows = []
    ids = Column.from_numpy(np.arange(n, dtype=np.int64))

    def floor_of(table, id_col, kept, ncols):
        fields = [Field(f"c{j}", DType.INT64, True) for j in range(ncols)]
        pred = PhysicalBinaryExpr.create(ColumnExpr.try_create(None, id_col), Operator.Lt, PhysicalLiteralExpr.create(ScalarValue.Int64(kept)))
        return timed(ctx, lambda: ctx.selection(table, pred.flatten(fields)), reps)

    for name, make in shapes(n, rng):
        if only and name not in only:
            continue
        keys = make()
        nk = len(keys)
        table = ctx.table_from_host(keys + [ids])
        cols = list(range(nk))
        wall, ms, cnt, out = timed(ctx, lambda: ctx.distinct(table, cols), reps)
        kept = out.num_rows
        rec = dict(rows=n, shape=name, kept=kept, wall_ms=wall, kernel_ms=sum(ms.values()), set_kernel_ms=sum(v for k, v in ms.items() if k in SET_LABELS), by_label_ms=ms, launches=cnt)

        def window_route():
            rn = ctx.window(table, cols, [], [(W.RowNumber,)])
            beside = ctx.append_columns(table, [rn])
            fields = [Field(f"c{j}", DType.INT64, True) for j in range(nk + 2)]
            pred = PhysicalBinaryExpr.create(ColumnExpr.try_create(None, nk + 1), Operator.Eq, PhysicalLiteralExpr.create(ScalarValue.UInt64(1)))
            return ctx.project(ctx.selection(beside, pred.flatten(fields)), list(range(nk + 1)))

        wwall, wms, _, wout = timed(ctx, window_route, reps)
        assert wout.num_rows == kept, (name, wout.num_rows, kept)
        fwall, fms, _, fout = floor_of(table, nk, kept, nk + 1)
        assert fout.num_rows == kept
        rec.update(window_route_wall_ms=wwall, window_route_kernel_ms=sum(wms.values()), floor_wall_ms=fwall, floor_kernel_ms=sum(fms.values()))
        rec["ratio_to_window_route"] = rec["kernel_ms"] / rec["window_route_kernel_ms"]
        rec["ratio_to_floor"] = rec["kernel_ms"] / rec["floor_kernel_ms"]
        rows.append(rec)
        say(f"--- distinct {name}: {kept} of {n} rows kept; wall {wall:.3f}  kernels {rec['kernel_ms']:.3f} (set table {rec['set_kernel_ms']:.3f})"
            f"  | window route kernels {rec['window_route_kernel_ms']:.3f} (x{1 / rec['ratio_to_window_route']:.2f})  | selection floor kernels {rec['floor_kernel_ms']:.3f} (x{rec['ratio_to_floor']:.2f} of it)")
        for k in sorted(ms, key=lambda k: (k not in SET_LABELS, SET_LABELS.index(k) if k in SET_LABELS else 0, k)):
            say(f"{k:>22} {cnt[k]:>4} {ms[k]:9.3f}")
        del table, out, wout, fout

    if only and "set_ops" not in only:
        return rows
    m = min(n, 1_000_000)
    left_vals = (np.arange(n, dtype=np.int64) * MIX & 0xFFFFFFFF) % (2 * m)
    lt = ctx.table_from_host([Column.from_numpy(left_vals)])
    rt = ctx.table_from_host([Column.from_numpy(np.arange(m, dtype=np.int64) * 2)])
    both = ctx.table_from_host([Column.from_numpy(left_vals), ids])
    for op in (SetOp.Intersect, SetOp.Except):
        wall, ms, cnt, out = timed(ctx, lambda: ctx.set_op(lt, rt, op), reps)
        kept = out.num_rows
        fwall, fms, _, fout = floor_of(both, 1, kept, 2)
        rec = dict(rows=n, shape=f"{op.name.lower()}_{m}_right_rows", kept=kept, wall_ms=wall, kernel_ms=sum(ms.values()), set_kernel_ms=sum(v for k, v in ms.items() if k in SET_LABELS),
                   by_label_ms=ms, launches=cnt, floor_wall_ms=fwall, floor_kernel_ms=sum(fms.values()))
        rec["ratio_to_floor"] = rec["kernel_ms"] / rec["floor_kernel_ms"]
        rows.append(rec)
        say(f"--- {op.name.lower()} of {n} left rows against {m} right rows: {kept} rows kept; wall {wall:.3f}  kernels {rec['kernel_ms']:.3f} (set table {rec['set_kernel_ms']:.3f})"
            f"  | selection floor kernels {rec['floor_kernel_ms']:.3f} (x{rec['ratio_to_floor']:.2f} of it)")
        for k in sorted(ms, key=lambda k: (k not in SET_LABELS, SET_LABELS.index(k) if k in SET_LABELS else 0, k)):
            say(f"{k:>22} {cnt[k]:>4} {ms[k]:9.3f}")
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--shapes", default="", help="comma-separated shape names, `set_ops` for the INTERSECT / EXCEPT pair (default: all)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "set_ops"))
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    ctx = capi.Context(0)
    ctx.timing_enable(True)
    lines = [f"library {os.path.basename(capi.LIB_PATH)}; {a.rows} rows; medians of {a.reps} repetitions after a warm-up; ms of kernel time from nqe_ctx_timing_* unless it says wall; label, launches, ms"]

    def say(s):
        lines.append(s)
        print(s, flush=True)

    rows = run(ctx, a.rows, a.reps, say, [s for s in a.shapes.split(",") if s])
    with open(os.path.join(a.out, "probe.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    with open(os.path.join(a.out, "probe.json"), "w") as f:
        json.dump(rows, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
