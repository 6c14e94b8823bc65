"""Helpers of the PhysicalUnaryExpr GPU tests: ulp distance, the three evaluation forms, the CPU-side threshold guard."""
import contextlib
import os

import numpy as np

# The allowed distance between the device's sin / cos and numpy's (glibc), in ulps of the expected value: the device math
# library implements the OpenCL math functions, whose full-profile bound for double-precision sin and cos is 4 ulp, plus 1 ulp
# for the host library's own error.  It does not come from what the kernels produce.
TRIG_ULPS = 5

# the three forms every tree is run through: the interpreting stack machine, the run-time compiled kernels
# (compiled before the first execution, from the first row), one kernel per node
FORMS = {
    "interpreter": {"NQE_NO_JIT": "1"},
    "compiled": {"NQE_JIT_SYNC": "1", "NQE_JIT_MIN_ROWS": "1"},
    "node_at_a_time": {"NQE_NO_EXPR_TREE": "1"},
}


@contextlib.contextmanager
def environment(**kw):
    keys = ("NQE_NO_JIT", "NQE_JIT_SYNC", "NQE_JIT_MIN_ROWS", "NQE_NO_EXPR_TREE")
    saved = {k: os.environ.get(k) for k in keys}
    try:
        for k in keys:
            os.environ.pop(k, None)
        os.environ.update(kw)
        yield
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def ordered(x):
    """float64 -> uint64 that orders like the doubles (adjacent doubles differ by 1, -0.0 and +0.0 coincide); subnormals included"""
    u = np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)
    top = np.uint64(1 << 63)
    return np.where(u >= top, top - (u - top), top + u)  # negative doubles mirrored below 2^63, positive ones above


def ulp_distance(got, exp):
    """distance between the ordered bit patterns; NaN against NaN is 0, NaN against a number is 'infinite'"""
    got, exp = np.asarray(got, dtype=np.float64), np.asarray(exp, dtype=np.float64)
    a, b = ordered(got), ordered(exp)
    d = (np.maximum(a, b) - np.minimum(a, b)).astype(np.float64)  # exact in uint64; small distances convert exactly
    both_nan = np.isnan(got) & np.isnan(exp)
    one_nan = np.isnan(got) ^ np.isnan(exp)
    return np.where(both_nan, 0.0, np.where(one_nan, np.inf, d))


def assert_clear_of_threshold(values, literal, what):
    """CPU-side guard of a predicate test: NO row's numpy value lies within 16 ulp of the literal it is compared with, so the device
    (within TRIG_ULPS of numpy) must select exactly numpy's rows — nothing is dropped from the comparison afterwards"""
    d = ulp_distance(values, np.full(len(values), literal))
    assert d.min() > 16, f"{what}: a row lies {d.min()} ulp from the literal {literal}; choose another seed or literal"


def bits(a):
    return np.asarray(a, dtype=np.float64).view(np.uint64)
