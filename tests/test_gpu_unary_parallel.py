"""GPU: the sharded selection + projection and the sharded aggregate with unary nodes in their predicates — two ranks sharing
cuda:0 through the host-staged transport, as tests/test_gpu_parallel.py does for the binary-only trees: the nqe_sharded_* entry
points take the same node arrays, and every rank must see what a single GPU computes."""
import os
import socket

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 120_001


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def make_data():
    rng = np.random.default_rng(21)
    return np.arange(N, dtype=np.int64), rng.random(N) * 200.0 - 100.0


def plans():
    from naive_query_engine_amd import AggregateFunc, Operator, UnaryOperator
    from naive_query_engine_amd.expression import binop, col, lit_f64, lit_i64, unop
    from tests.helpers import fields

    f = fields("id", "v")
    sel = binop(unop(UnaryOperator.Abs, binop(col(1), Operator.Minus, lit_f64(50.0))), Operator.Lt, lit_f64(10.0)).flatten(f)  # abs(v - 50.0) < 10.0
    proj = [col(0).flatten(f), binop(unop(UnaryOperator.Sin, col(1)), Operator.Multiply, lit_f64(2.0)).flatten(f)]             # id, sin(v) * 2.0
    pred = binop(unop(UnaryOperator.Cos, col(1)), Operator.Gt, lit_f64(0.25)).flatten(f)                                      # cos(v) > 0.25
    key = binop(col(0), Operator.Modulos, lit_i64(7)).flatten(f)
    aggs = [(AggregateFunc.Count, 1), (AggregateFunc.Sum, 1), (AggregateFunc.Min, 1), (AggregateFunc.Max, 1)]
    return sel, proj, pred, key, aggs


def worker(rank, world, port, q):
    import torch
    import torch.distributed as dist

    from naive_query_engine_amd import Column, capi
    from naive_query_engine_amd.parallel import make_staged_comm, shard_range, sharded_aggregate, sharded_selection_projection

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.cuda.set_device(0)
        ctx = capi.Context(0)
        ids, v = make_data()
        lo, hi = shard_range(N, rank, world)
        t = ctx.table_from_host([Column.from_numpy(ids[lo:hi]), Column.from_numpy(v[lo:hi])])
        sel, proj, pred, key, aggs = plans()
        comm = make_staged_comm(ctx)
        sp = sharded_selection_projection(comm, t, sel, proj, gather=True).to_host()
        out, keys = sharded_aggregate(comm, t, aggs, group_nodes=key, pred_nodes=pred)
        res = np.stack([c.to_numpy().astype(np.float64) for c in out.to_host()], axis=1)
        q.put((rank, sp[0].to_numpy().tolist(), sp[1].to_numpy().view(np.uint64).tolist(), keys.to_host()[0].to_numpy().tolist(), res.tolist()))
        ctx.close()
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_sharded_operators_with_unary_predicates_two_ranks_one_gpu():
    import torch.multiprocessing as mp

    from naive_query_engine_amd import Column, capi
    from tests.unary_util import TRIG_ULPS, assert_clear_of_threshold, ulp_distance

    ids, v = make_data()
    assert_clear_of_threshold(np.abs(v - 50.0), 10.0, "abs(v - 50.0) < 10.0")
    assert_clear_of_threshold(np.cos(v), 0.25, "cos(v) > 0.25")
    mpc = mp.get_context("spawn")
    q = mpc.Queue()
    port = free_port()
    procs = [mpc.Process(target=worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    results = [q.get(timeout=240) for _ in range(2)]
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    sel, proj, pred, key, aggs = plans()
    ctx = capi.Context(0)
    t = ctx.table_from_host([Column.from_numpy(ids), Column.from_numpy(v)])
    one = ctx.selection_projection(t, sel, proj).to_host()
    single = np.stack([c.to_numpy().astype(np.float64) for c in ctx.aggregate(t, aggs, group_nodes=key, pred_nodes=pred).to_host()], axis=1)
    keep = np.abs(v - 50.0) < 10.0
    passed = np.cos(v) > 0.25
    for rank, sp_ids, sp_bits, keys, res in results:
        assert sp_ids == ids[keep].tolist() == one[0].to_numpy().tolist()                       # exactly numpy's rows, in order
        assert sp_bits == one[1].to_numpy().view(np.uint64).tolist()                             # the same bits as a single GPU
        assert ulp_distance(np.array(sp_bits, dtype=np.uint64).view(np.float64), (np.sin(v) * 2.0)[keep]).max() <= TRIG_ULPS
        assert keys == list(range(7))
        got = np.array(res)
        assert (got[:, [0, 2, 3]] == single[:, [0, 2, 3]]).all() and np.allclose(got[:, 1], single[:, 1], rtol=1e-9, atol=0)
        for k in range(7):
            rows = passed & (ids % 7 == k)
            assert got[k, 0] == rows.sum() and got[k, 2] == v[rows].min() and got[k, 3] == v[rows].max()
            assert np.isclose(got[k, 1], v[rows].sum(), rtol=1e-9, atol=0)
    ctx.close()
