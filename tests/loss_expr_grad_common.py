"""Shared by tests/test_gpu_loss_expr_grad.py and tests/test_loss_expr_grad_api.py: small populations, data
and comparisons for the gradient and the constant optimiser under a loss given as an expression."""
import math

import numpy as np

import srhip

import loss_expr_common as X

F32_REL = 1e-6   # the project's standing bars (tests/test_gpu_parity.py)
F64_REL = 1e-12
DTYPES = [np.float32, np.float64]
DT_IDS = ["f32", "f64"]
TREE_OPS = dict(binary_operators=("+", "-", "*", "/"), unary_operators=("cos", "exp"))


def rel_bar(dtype):
    return F32_REL if np.dtype(dtype) == np.float32 else F64_REL


def x(i):
    return srhip.Node(feature=i)


def tree_options():
    return srhip.Options(**TREE_OPS)


def program(ctx, trees, dtype, opts=None):
    opts = opts or tree_options()
    nodes, offs = srhip.flatten(trees, opts, dtype)
    return srhip.Program(ctx, nodes, offs, opts, dtype)


def bits(v):
    return np.ascontiguousarray(np.asarray(v, dtype=np.float64)).view(np.uint64)


def flat(grads):
    return np.concatenate([np.asarray(g, dtype=np.float64).ravel() for g in grads]) if len(grads) else np.zeros(0)


def same_bits(a, b):
    """(loss, grads, ok) triples equal bit for bit."""
    return (np.array_equal(np.asarray(a[2]), np.asarray(b[2])) and np.array_equal(bits(a[0]), bits(b[0]))
            and np.array_equal(bits(flat(a[1])), bits(flat(b[1]))))


def l2_expr(weighted=False):
    e = X.N("square", X.diff())
    return srhip.ExprLoss(X.W() * e if weighted else e, X.options())


def lp_expr():
    return srhip.ExprLoss(X.N("abs", X.diff()) ** X.C(2.5), X.options())


def nine_constants():
    """9 constants: chunks at c0 = 0, 8 (8 tangents) or 0, 4, 8 (4 tangents)."""
    a = (x(1) * 0.5 + 0.25) * (x(2) * -1.5 + 0.75)
    b = (x(3) * 1.25 + -0.5) * 0.3
    return a + b + x(1) * 2.0 + -0.125


def row_failing():
    return x(1) / (x(2) - x(2))


def static_failing():
    return x(1) + srhip.Node(val=np.inf)


def edge_population(with_cos):
    trees = [x(1) + x(2), nine_constants(), static_failing(), row_failing(), x(2) * 1.5 + x(3) * -0.5 + 0.1]
    if with_cos:
        trees.append(srhip.Node("cos", x(1)) * 0.7 + 0.2)
    return trees


def edge_data(dtype, m, seed=0):
    rng = np.random.default_rng(100 + seed + m)
    Xd = rng.standard_normal((3, m)).astype(dtype)
    y = (2 * np.cos(Xd[1]) + Xd[0] ** 2 - 2).astype(dtype)
    w = rng.uniform(0.25, 4.0, m).astype(dtype)
    idx = rng.integers(0, m, size=max(1, (2 * m) // 3))
    idx[-1] = idx[0]
    return Xd, y, w, idx


def scale(wabs, dl_abs, g, den):
    """S_k = sum_i |w_i| |dl_i| |g_ik| / den for every constant k (g: [nconst, m])."""
    g = np.abs(np.asarray(g, dtype=np.float64))
    return np.array([math.fsum(wabs * dl_abs * g[k]) / den for k in range(g.shape[0])])


def host_dloss_abs(loss, pred, y, h=1e-6):
    """|d l / d prediction| by a Float64 central difference of the ExprLoss's host callable (a scale only)."""
    p = np.asarray(pred, dtype=np.float64)
    t = np.asarray(y, dtype=np.float64)
    return np.abs((loss(p + h, t) - loss(p - h, t)) / (2 * h))


class Member:
    def __init__(self, tree):
        self.tree, self.loss, self.score, self.birth = tree, np.float64(0), np.float64(0), -1
