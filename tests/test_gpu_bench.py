"""bench.py's plain run on the GPU: the contract's line and nothing that only --full measures, and --dump-outputs writing what the
timed path computed in its last step — checked against the oracle on the same generated rows."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["count_v", "sum_v", "avg_v", "min_v", "max_v"]


def run_bench(args, **env_extra):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    env.update(env_extra)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True, timeout=500, env=env)
    assert out.returncode == 0, out.stderr[-3000:]
    return json.loads(out.stdout.strip().splitlines()[-1])


def oracle_headline(total):
    """the headline over rows [0, total) of the generators, rows sorted: (count, sum, avg, min, max) per group"""
    from naive_query_engine_amd import AggregateFunc as A, Column, Operator
    from naive_query_engine_amd.expression import binop, col, lit_i64
    from oracle import oracle as orc
    from tests.helpers import fields

    ids = orc.synth_fill(0, 0, 0, total).view(np.int64)
    v = orc.synth_fill(2, 3, 0, total).view(np.float64)
    f = fields("id", "v")
    ref = orc.aggregate([[Column.from_numpy(ids), Column.from_numpy(v)]], [(A.Count, 1), (A.Sum, 1), (A.Avg, 1), (A.Min, 1), (A.Max, 1)],
                        group_nodes=binop(col(0), Operator.Modulos, lit_i64(1024)).flatten(f), pred_nodes=binop(col(0), Operator.Lt, lit_i64(total // 2)).flatten(f))
    exp = np.stack([c.to_numpy().astype(np.float64) for c in ref[0]], axis=1)
    return exp[np.lexsort(exp.T[::-1])]


def assert_matches_oracle(got, total):
    assert got.dtype == np.float64 and got.shape == (1024, 5)
    got, exp = got[np.lexsort(got.T[::-1])], oracle_headline(total)
    assert (got[:, [0, 3, 4]] == exp[:, [0, 3, 4]]).all(), "counts / min / max differ"
    assert np.allclose(got, exp, rtol=1e-9, atol=0), "sum / avg differ"


@pytest.mark.timeout(600)
def test_plain_headline_run_dumps_its_last_step(tmp_path):
    n, d = 1 << 21, tmp_path / "outputs"
    line = run_bench(["--gpus", "1", "--rows", str(n), "--steps", "3", "--warmup", "1", "--reserve-gb", "1", "--dump-outputs", str(d)])
    assert line["metric"] == "filter_hash_aggregate_rows_per_s" and line["unit"] == "rows/s" and line["higher_is_better"] is True
    assert line["dtype"] == "f64" and line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0
    assert abs(line["value"] - n / (line["ms_per_step"] * 1e-3)) <= 1e-9 * line["value"]
    for k in ("configs", "parity_checked", "cpu_baseline", "cpu_optimised_multicore", "cold_ms", "upload", "result_check"):
        assert k not in line, k
    assert sorted(os.listdir(d)) == sorted(f"{x}.npy" for x in NAMES)
    assert_matches_oracle(np.stack([np.load(d / f"{x}.npy") for x in NAMES], axis=1), n)


@pytest.mark.timeout(600)
def test_plain_two_rank_run_dumps_the_sharded_result(tmp_path):
    """`--gpus 2` over the host-staged transport (both ranks on one device): rank 0 writes the merged result and its group keys"""
    n, d = 1 << 20, tmp_path / "outputs"
    line = run_bench(["--gpus", "2", "--rows", str(n), "--steps", "2", "--warmup", "1", "--dump-outputs", str(d)], NQE_BENCH_TRANSPORT="host")
    assert line["n_gpus"] == 2 and line["ranks"] == 2 and line["steps"] == 2 and line["ms_per_step"] > 0
    assert "configs" not in line and "result_check" not in line and "preflight" not in line
    assert sorted(os.listdir(d)) == sorted(f"{x}.npy" for x in NAMES + ["group_key"])
    assert sorted(np.load(d / "group_key.npy").tolist()) == list(range(1024))
    assert_matches_oracle(np.stack([np.load(d / f"{x}.npy") for x in NAMES], axis=1), 2 * n)
