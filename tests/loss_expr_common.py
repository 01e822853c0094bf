"""Shared by tests/test_loss_expr.py and tests/test_gpu_loss_expr.py: the built-in distance and margin
losses of srhip/losses.py restated as loss expressions (Node trees over prediction = feature 1, target =
feature 2, weight = feature 3), and small helpers over the C ABI.

The piecewise losses select with `greater` and `cond`: cond(g, v) is v where g > 0 and a signed zero
elsewhere (whatever v is there), so `cond(1 - g, A) + cond(g, B)` is numpy's where(g, B, A) up to the sign
of a zero result.  Constants are written as the numpy forms compute them, operation by operation in T
(`0.5 / gamma`, `2 * pi`), so that the exact class stays bit for bit.
"""
import ctypes

import numpy as np

import srhip
from srhip import _lib
from srhip import losses as L

BINARY = ("+", "-", "*", "/", "^", "greater", "cond", "max")
UNARY = ("abs", "square", "neg", "exp", "log", "log1p", "cos", "tanh", "cosh", "relu", "sqrt")


def options():
    return srhip.Options(binary_operators=BINARY, unary_operators=UNARY)


def N(op, *args):
    return srhip.Node(op, *args)


def C(v):
    return srhip.Node(val=float(v))


def P():
    return srhip.Node(feature=1)


def T_():
    return srhip.Node(feature=2)


def W():
    return srhip.Node(feature=3)


def diff():
    return P() - T_()


def agree():  # LossFunctions' margin agreement: target * output
    return T_() * P()


def where(g, b, a):
    """b where g (a 0/1 value) is 1, a where it is 0."""
    return N("cond", C(1.0) - g(), a) + N("cond", g(), b)


def _huber(d):
    g = lambda: N("greater", N("abs", diff()), C(d))
    return where(g, C(d) * (N("abs", diff()) - C(0.5) * C(d)), C(0.5) * N("square", diff()))


def _smoothed_l1_hinge(gm):
    g = lambda: N("greater", C(1.0) - C(gm), agree())  # a < 1 - gamma
    h = lambda: N("max", C(0.0), C(1.0) - agree())
    return where(g, (C(1.0) - C(gm) / C(2.0)) - agree(), (C(0.5) / C(gm)) * N("square", h()))


def _modified_huber():
    g = lambda: N("greater", C(-1.0), agree())  # a < -1
    h = lambda: N("max", C(0.0), C(1.0) - agree())
    return where(g, C(-4.0) * agree(), N("square", h()))


def _dwd(q):
    g = lambda: N("greater", agree(), C(q) / (C(q) + C(1.0)))  # a > q / (q + 1)
    far = ((C(q) ** C(q)) / ((C(q) + C(1.0)) ** (C(q) + C(1.0)))) / (agree() ** C(q))
    return where(g, far, C(1.0) - agree())


def _logit_dist():
    er = lambda: N("exp", diff())
    den = lambda: C(1.0) + er()
    return N("neg", N("log", (C(4.0) * er()) / (den() * den())))


# (name, losses.py instance, expression, exact class of DESIGN.md 4, input family)
#   families: "dist" / "margin": general inputs, every branch of the piecewise losses is taken;
#   "*_cond": inputs on which the loss is well conditioned, for the losses whose last operation cancels
#   (-log(x) near x = 1, 1 - cos near 0, 1 - tanh near 1): there a one-ulp difference between two correct
#   libms in the inner function is a large relative difference of the loss, which no relative bar on the
#   loss can hold.
CASES = [
    ("L2DistLoss", L.L2DistLoss(), lambda: N("square", diff()), True, "dist"),
    ("L1DistLoss", L.L1DistLoss(), lambda: N("abs", diff()), True, "dist"),
    ("LPDistLoss(2.5)", L.LPDistLoss(2.5), lambda: N("abs", diff()) ** C(2.5), False, "dist"),
    ("HuberLoss(1)", L.HuberLoss(1.0), lambda: _huber(1.0), True, "dist"),
    ("L1EpsilonInsLoss(0.5)", L.L1EpsilonInsLoss(0.5), lambda: N("max", C(0.0), N("abs", diff()) - C(0.5)), True, "dist"),
    ("L2EpsilonInsLoss(0.5)", L.L2EpsilonInsLoss(0.5),
     lambda: N("square", N("max", C(0.0), N("abs", diff()) - C(0.5))), True, "dist"),
    ("LogitDistLoss", L.LogitDistLoss(), _logit_dist, False, "dist_cond"),
    ("PeriodicLoss(16)", L.PeriodicLoss(16.0),
     lambda: C(1.0) - N("cos", (diff() * (C(2.0) * C(np.pi))) / C(16.0)), False, "dist_cond"),
    ("QuantileLoss(0.3)", L.QuantileLoss(0.3), lambda: diff() * (C(0.3) - N("greater", C(0.0), diff())), True, "dist"),
    ("ZeroOneLoss", L.ZeroOneLoss(), lambda: N("greater", C(0.0), agree()), True, "margin"),
    ("PerceptronLoss", L.PerceptronLoss(), lambda: N("max", C(0.0), N("neg", agree())), True, "margin"),
    ("LogitMarginLoss", L.LogitMarginLoss(), lambda: N("log1p", N("exp", N("neg", agree()))), False, "margin_cond"),
    ("L1HingeLoss", L.L1HingeLoss(), lambda: N("max", C(0.0), C(1.0) - agree()), True, "margin"),
    ("L2HingeLoss", L.L2HingeLoss(), lambda: N("square", N("relu", C(1.0) - agree())), True, "margin"),
    ("SmoothedL1HingeLoss(0.5)", L.SmoothedL1HingeLoss(0.5), lambda: _smoothed_l1_hinge(0.5), True, "margin"),
    ("ModifiedHuberLoss", L.ModifiedHuberLoss(), _modified_huber, True, "margin"),
    ("L2MarginLoss", L.L2MarginLoss(), lambda: N("square", C(1.0) - agree()), True, "margin"),
    ("ExpLoss", L.ExpLoss(), lambda: N("exp", N("neg", agree())), False, "margin_cond"),
    ("SigmoidLoss", L.SigmoidLoss(), lambda: C(1.0) - N("tanh", agree()), False, "margin_cond"),
    ("DWDMarginLoss(1)", L.DWDMarginLoss(1.0), lambda: _dwd(1.0), False, "margin_cond"),
]
CASE_IDS = [c[0] for c in CASES]

NROWS = 191


def inputs(family, dtype):
    """(pred, y, w), NROWS finite rows each, every intermediate of the family's losses finite."""
    rng = np.random.default_rng({"dist": 1, "dist_cond": 2, "margin": 3, "margin_cond": 4}[family])
    n = NROWS
    w = rng.uniform(0.25, 4.0, n)
    if family == "dist":
        y = rng.uniform(-2, 2, n)
        pred = y + rng.uniform(-3, 3, n)  # |d| on both sides of Huber's 1 and the insensitive 0.5
    elif family == "dist_cond":
        # 2 <= |d| <= 6: LogitDist's log argument 4 e^d / (1 + e^d)^2 is at most 0.42, PeriodicLoss(16)'s angle
        # 2 pi d / 16 lies in [pi/4, 3 pi/4], where 1 - cos >= 0.29
        y = rng.uniform(-2, 2, n)
        pred = y + rng.uniform(2, 6, n) * rng.choice([-1.0, 1.0], n)
    elif family == "margin":
        y = rng.choice([-1.0, 1.0], n)
        pred = rng.uniform(-3, 3, n)  # a = y pred on both sides of -1, 0, 0.5 and 1
    else:
        # |a| <= 1.25: SigmoidLoss's 1 - tanh(a) >= 0.15; away from 0 for DWD's 1 / a^q
        y = rng.choice([-1.0, 1.0], n)
        pred = rng.uniform(0.05, 1.25, n) * rng.choice([-1.0, 1.0], n)
    return pred.astype(dtype), y.astype(dtype), w.astype(dtype)


# ---- the C ABI ----------------------------------------------------------------------------------
def node_table(rows):
    """srhip_node records from (degree, constant, op, feature, l, r, val) tuples."""
    arr = np.zeros(len(rows), dtype=_lib.NODE_DTYPE)
    for i, (deg, const, op, feat, l, r, val) in enumerate(rows):
        arr[i] = (deg, const, op, feat, 0, l, r, val)
    return arr


def create_raw(dtype_code, nodes, opts, nargs, nnodes=None):
    """srhip_loss_expr_create -> (status, handle, message)."""
    lib = _lib.load()
    h = ctypes.c_void_p()
    ops = opts.c_operators()
    rc = lib.srhip_loss_expr_create(dtype_code, _lib.ptr(nodes), len(nodes) if nnodes is None else nnodes,
                                    ctypes.byref(ops), nargs, ctypes.byref(h))
    return rc, h, lib.srhip_last_error().decode() if rc else ""


def destroy(h):
    _lib.load().srhip_loss_expr_destroy(h)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)
