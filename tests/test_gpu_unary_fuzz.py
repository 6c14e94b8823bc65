"""GPU differential test: random expression trees over Float64 columns mixing abs / sin / cos / tan with + - * and compares,
against numpy in float64 (fixed seeds).  Arithmetic below a sin / cos node, and whole trees without one, are compared bit for bit;
a tree with a transcendental has at most two operators above it and is compared within the tolerance carried through them.  Each
tree runs interpreted, run-time compiled and node-at-a-time, and the three results are bit-identical (so `a * b + c` rounds twice in
every form: no contraction)."""
import numpy as np
import pytest

from tests.helpers import fields
from tests.unary_util import FORMS, TRIG_ULPS, bits, environment, ulp_distance

pytestmark = pytest.mark.gpu

N = 20_011
EPS = 2.0 ** -53


def exact_tree(rng, depth, cols, data):
    """a tree of + - * abs over columns and literals: (expr, numpy value) — IEEE, so bit-identical on the device"""
    from naive_query_engine_amd import Operator, UnaryOperator
    from naive_query_engine_amd.expression import binop, col, lit_f64, unop

    if depth == 0 or rng.random() < 0.25:
        k = int(rng.integers(0, len(cols)))
        return col(cols[k]), data[k]
    if rng.random() < 0.3:
        e, v = exact_tree(rng, depth - 1, cols, data)
        return unop(UnaryOperator.Abs, e), np.abs(v)
    op = [Operator.Plus, Operator.Minus, Operator.Multiply][int(rng.integers(0, 3))]
    l, lv = exact_tree(rng, depth - 1, cols, data)
    if rng.random() < 0.5:
        c = float(np.round(rng.random() * 8.0 - 4.0, 2))
        r, rv = lit_f64(c), np.full(N, c)
    else:
        r, rv = exact_tree(rng, depth - 1, cols, data)
    with np.errstate(all="ignore"):
        val = lv + rv if op == Operator.Plus else lv - rv if op == Operator.Minus else lv * rv
    return binop(l, op, r), val


def trig_tree(rng, cols, data):
    """f(exact tree) with f in sin / cos / tan, then up to two of: * literal, + exact tree, abs.  Returns (expr, value, absolute bound);
    the bound is None when nothing stands above the transcendental: then the result itself is held to TRIG_ULPS ulps"""
    from naive_query_engine_amd import Operator, UnaryOperator
    from naive_query_engine_amd.expression import binop, lit_f64, unop

    inner, iv = exact_tree(rng, 2, cols, data)
    func = [UnaryOperator.Sin, UnaryOperator.Cos, UnaryOperator.Tan][int(rng.integers(0, 3))]
    val = np.sin(iv) if func == UnaryOperator.Sin else np.cos(iv)  # Tan is the cosine (quirk Q16)
    e = unop(func, inner)
    err = TRIG_ULPS * np.spacing(np.abs(val))  # 5 ulp of the expected value
    above = int(rng.integers(0, 3))
    for _ in range(above):
        kind = int(rng.integers(0, 3))
        if kind == 0:
            c = float(np.round(rng.random() * 6.0 - 3.0, 2)) or 1.5
            e, val, err = binop(e, Operator.Multiply, lit_f64(c)), val * c, err * abs(c)
        elif kind == 1:
            o, ov = exact_tree(rng, 1, cols, data)
            e, val = binop(e, Operator.Plus, o), val + ov
        else:
            e, val = unop(UnaryOperator.Abs, e), np.abs(val)
        err = err + np.spacing(np.abs(val))  # the step's own rounding: half an ulp on either side, which may round a different way
    return e, val, (err if above else "ulps")


@pytest.mark.parametrize("seed", range(12))
def test_random_unary_trees_against_numpy(seed):
    from naive_query_engine_amd import Column, Operator, capi
    from naive_query_engine_amd.expression import binop, lit_f64

    rng = np.random.default_rng(1000 + seed)
    ctx = capi.Context(0)
    try:
        data = [rng.random(N) * 20.0 - 10.0, rng.random(N) * 2.0, np.round(rng.random(N) * 100.0 - 50.0, 1)]
        masks = [None, rng.random(N) > 0.15, None] if seed % 2 else [None, None, None]
        t = ctx.table_from_host([Column.from_numpy(d, m) for d, m in zip(data, masks)])
        f = fields("a", "b", "c")
        cases = []
        for _ in range(6):
            e, v = exact_tree(rng, 3, [0, 1, 2], data)
            cases.append((e, v, None))
            thr = float(np.round(np.nanmedian(v), 3))
            cases.append((binop(e, Operator.Lt, lit_f64(thr)), v < thr, None))  # an exact value against a literal: the same rows, always
        for _ in range(6):
            cases.append(trig_tree(rng, [0, 1, 2], data))
        for k, (e, val, err) in enumerate(cases):
            nodes = e.flatten(f)
            valid = np.ones(N, dtype=bool)
            for nd in nodes:
                if nd.kind == 0 and masks[nd.column] is not None:
                    valid &= masks[nd.column]
            res = {}
            for form, env in FORMS.items():
                with environment(**env):
                    c = ctx.expr_evaluate(t, nodes).to_host()[0]
                res[form] = (c.to_numpy(), c.valid_mask())
            base, bvalid = res["interpreter"]
            assert (bvalid == valid).all(), (seed, k)
            for form, (g, gv) in res.items():
                assert (gv == bvalid).all(), (seed, k, form)
                same = (g[valid] == base[valid]) if g.dtype == bool else (bits(g[valid]) == bits(base[valid]))
                assert same.all(), (seed, k, form, repr(e))
            if isinstance(err, str):  # a bare transcendental over an exact tree: the issue's bound, in ulps of the expected value
                d = ulp_distance(base[valid], val[valid])
                assert d.max() <= TRIG_ULPS, (seed, k, repr(e), d.max())
            elif err is None:
                ok = (base[valid] == val[valid]) if base.dtype == bool else ((bits(base[valid]) == bits(val[valid])) | (np.isnan(base[valid]) & np.isnan(val[valid])))
                assert ok.all(), (seed, k, repr(e))
            else:
                with np.errstate(all="ignore"):
                    diff = np.abs(base[valid] - val[valid])
                fin = np.isfinite(val[valid])
                assert (diff[fin] <= err[valid][fin]).all(), (seed, k, repr(e), float(np.nanmax(diff[fin] / err[valid][fin])))
    finally:
        ctx.close()
