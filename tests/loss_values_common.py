"""Shared by tests/test_loss_values_table.py (no device) and tests/test_gpu_loss_values.py: the golden table of
exact loss values (tests/golden/make_loss_values.py), the datasets that put every tabulated residual or
agreement in front of the loss epilogue unchanged, and the bars.  Not a test module.

Data.  The prediction tree is the single leaf x1, so the prediction is bit for bit the column.
Distance losses see d = x1 - y: general rows have x1 a multiple of 1/8 in [-1, 1] and y = x1 - d (every
fourth row: y = 0, x1 = d); kink and extreme rows have y = 0.  Margin losses see a = y * x1 with y cycling
through -1, +1, -2, +2 and x1 = a / y: the rows at +-2 tell the product from the sign.  Both identities are
asserted exactly in T where the data is built.

Bars (eps = eps(T), tiny = the smallest normal of T; no bar comes from what a device returns).

  per row:   |got - exact| <= B_k eps max(|exact|, floor_k(x)) + tiny
  a mean:    |got - fsum(w l) / fold(w)| <= B_k eps fsum(w max(|l|, floor_k)) / fsum(w) + tiny

The denominator of a weighted mean is a rule of the library, not rounding noise of the loss: sum(w) is the
weights added one by one in Float64 in position order (a view's order for idx= and row sets), the same bits on
every path.  For Float32 weights that fold is exact to n 2^-53.  For Float64 weights it is
not: over the 775 weights of the tiled shape it is 3.7 eps from fsum(w), which alone nearly spends B_k = 4.
So the expected mean is fsum(w l_exact) / fold(w), with fold(w) restated here (np.cumsum): the numerator
stays held to exact math, and the denominator to the documented order.

B_k = 4 for the 13 kinds built only from + - * max and comparisons.  Each correctly rounded operation adds a
relative error of at most eps / 2 and no rounded quantity is cancelled (the build has -ffp-contract=off), so
n operations stay within about n eps / 2.  Operations that round, per formula (inputs and T(p0) are exact; a
product with 0.5, 2 or 4 and abs, max, negation and selection do not round):

  L2                d d                                          1
  L1                |d|                                          0
  Huber             0.5 (d d)  |  p0 (|d| - 0.5 p0)              1 | 2
  L1EpsilonIns      max(0, |d| - p0)                             1
  L2EpsilonIns      e = |d| - p0; e e                            2  (3 half-eps: e's error counts twice)
  Quantile          d (p0 - [d < 0])                             2
  ZeroOne           [a < 0]                                      0
  Perceptron        max(0, -a)                                   0
  L1Hinge           max(0, 1 - a)                                1
  L2Hinge           h = 1 - a; h h                               2  (3 half-eps)
  SmoothedL1Hinge   (0.5 / g) (h h), h = 1 - a  |  (1 - g / 2) - a     4 (5 half-eps) | 2
  ModifiedHuber     h h, h = 1 - a  |  -4 a                      2 (3 half-eps) | 0
  L2Margin          h h, h = 1 - a                               2  (3 half-eps)

The worst, SmoothedL1Hinge's quadratic branch, is 2.5 eps; its linear branch subtracts a from the rounded
1 - g / 2, and with a < 1 - g the result is at least g / 2, so its error is at most (1 - g / 2) / (g / 2) + 1
half-eps = 3.3 half-eps at g = 0.6.  A weighted mean multiplies by w once more (one half-eps), and Float32's
unweighted in-lane sum of four rows adds two roundings to every row (two half-eps): 3.5 eps at the worst, inside 4.

L1, L1EpsilonIns, ZeroOne, Perceptron and L1Hinge make at most one rounding: per row they must equal the
exact value rounded to T, bit for value (EXACT_KINDS).  On the general rows (multiples of 2^-20 / 2^-48
below 2.5) that is the exact value itself; beside a kink 1 - a or |d| - p0 need not be representable.

B_k = derivative_rules_common.BAR (128) for the 7 transcendental kinds.

floor_k is 0 except where the published formula itself cancels: 1 for LogitDist (the log of a number near 1)
and Sigmoid (1 - tanh), 1 + |2 pi d / c| for Periodic (1 - cos, plus the rounding of the argument in T).
LogitDist's floor grows where e^d is subnormal (d < -87.3 in Float32; only the extreme block goes there): e^d
then carries an absolute error of up to eps tiny / 2, which -log(4 e^d / ..) turns into eps tiny / (2 e^d) --
0.019 at Float32's d = -100; the CPU restatement is 0.017 off there.  The allowance for it is 4 eps tiny / e^d
(the floor term is (4 / B_k) tiny / e^d), eight times the analysis and not B_k = 128 times.

The parameter block (PAR_KIND = L1EpsilonIns at 0.3, which Float32 does not hold, at |d| = prev, T(0.3), next)
tells T(p0) from the decimal: max(0, |d| - p0) rounds at most once, the tests demand equality, and with the
decimal 0.3 the value at |d| = T(0.3) is 1.2e-8 where exact math at T(0.3) gives 0.  On the 20 kinds'
own parameters the difference stays inside the bars (only Quantile's 0.3 and SmoothedL1Hinge's 0.6 are not
Float32 numbers, and neither kind is exact).
"""
import importlib.util
import math
import os

import numpy as np

import derivative_rules_common as drc
from conftest import GOLDEN
from derivative_rules_common import loss_object  # noqa: F401  (re-exported)
from forward_values_common import TILED_ROWS  # noqa: F401  (re-exported)


def _gen_module():
    spec = importlib.util.spec_from_file_location("make_loss_values", os.path.join(GOLDEN, "make_loss_values.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


GEN = _gen_module()
DIST, MARG, LOSS_P0 = GEN.DIST, GEN.MARG, GEN.LOSS_P0
KINDS = DIST + MARG
NP = drc.NP
EPS = drc.EPS
TINY = {"f32": float(np.finfo(np.float32).tiny), "f64": float(np.finfo(np.float64).tiny)}
POLY_KINDS = ("L2", "L1", "Huber", "L1EpsilonIns", "L2EpsilonIns", "Quantile", "ZeroOne", "Perceptron", "L1Hinge",
              "L2Hinge", "SmoothedL1Hinge", "ModifiedHuber", "L2Margin")
TRANS_KINDS = ("LP", "LogitDist", "Periodic", "LogitMargin", "Exp", "Sigmoid", "DWDMargin")
EXACT_KINDS = ("L1", "L1EpsilonIns", "ZeroOne", "Perceptron", "L1Hinge")
assert sorted(POLY_KINDS + TRANS_KINDS) == sorted(KINDS) and set(EXACT_KINDS) <= set(POLY_KINDS)
SMALL_POP_ROWS = 64 * 4096 + 65
MARGIN_Y = (-1.0, 1.0, -2.0, 2.0)
# extreme points whose loss in T is +Inf at a finite prediction (tests/test_loss_values_table.py asserts it of
# the CPU restatement); Float64's LP(1.5) stays finite on the tabulated points, so LogitMargin stands in
INF_POINTS = {"f32": (("Exp", -100.0), ("LP", 1e30), ("L2", 1e20)),
              "f64": (("Exp", -800.0), ("LogitMargin", -800.0), ("L2", 1e160))}

_TABLE = None


def table():
    """The loss table, with the general inputs of derivative_rules.npz beside it."""
    global _TABLE
    if _TABLE is None:
        z = dict(GEN.load_table())
        assert list(z["loss_kinds"]) == KINDS
        rules = drc.table()
        for dt in ("f32", "f64"):
            z[f"loss_d_{dt}"], z[f"loss_a_{dt}"] = rules[f"loss_d_{dt}"], rules[f"loss_a_{dt}"]
        _TABLE = z
    return _TABLE


def bar(kind):
    return 4 if kind in POLY_KINDS else drc.BAR


def floor(kind, x, dt):
    """floor_k at the residuals or agreements x (Float64 [n])."""
    x = np.asarray(x, np.float64)
    if kind == "LogitDist":
        with np.errstate(over="ignore", divide="ignore"):
            return 1.0 + (4.0 / drc.BAR) * TINY[dt] / np.exp(np.minimum(x, 0.0))
    if kind == "Sigmoid":
        return np.ones_like(x)
    if kind == "Periodic":
        return 1.0 + np.abs(2.0 * np.pi * x / LOSS_P0[kind])
    return np.zeros_like(x)


class Block:
    """Rows of one family ("dist" / "marg") and dtype: x1, y [n] in T, the residual or agreement v [n] in T,
    src [n] (the index of each row's point among the block's points) and exact [kinds of the family, n]."""

    def exact_of(self, kind):
        return self.exact[(DIST if self.family == "dist" else MARG).index(kind)]

    def kinds(self):
        return DIST if self.family == "dist" else MARG


def family(kind):
    return "dist" if kind in DIST else "marg"


def _points(fam, dt, which):
    """(v [P] in T, exact [kinds, P], y0 [P] bool: rows that must use y = 0) of the named blocks, concatenated."""
    z = table()
    c = "d" if fam == "dist" else "a"
    sl = slice(0, len(DIST)) if fam == "dist" else slice(len(DIST), None)
    vs, ex, y0 = [], [], []
    for w in which:
        if w == "general":
            v, e = z[f"loss_{c}_{dt}"], z[f"loss_l_{dt}"][sl]
            zero = np.arange(len(v)) % 4 == 3
        elif w == "param":  # (tabulated for PAR_KIND at PAR_P0 alone)
            assert fam == "dist"
            v = z[f"par_d_{dt}"]
            e = np.full((len(DIST), len(v)), np.nan)
            e[DIST.index(GEN.PAR_KIND)] = z[f"par_l_{dt}"]
            zero = np.ones(len(v), bool)
        else:
            blk = {"kinks": "kink", "extreme": "ext"}[w]
            v, e = z[f"{blk}_{c}_{dt}"], z[f"{blk}_l{c}_{dt}"]
            zero = np.ones(len(v), bool)
        vs.append(v)
        ex.append(e)
        y0.append(zero)
    return np.concatenate(vs), np.concatenate(ex, axis=1), np.concatenate(y0)


_BLOCKS = {}


def rows(fam, dt, which=("general", "kinks"), n=None, shift=0.0):
    """The Block of the named table blocks; n rows, the points cyclically (default: each point once).
    shift: x1 is the prediction minus shift (exactly), for the tree x1 + shift."""
    key = (fam, dt, tuple(which), n, shift)
    if key in _BLOCKS:
        return _BLOCKS[key]
    T = NP[dt]
    v, exact, y0 = _points(fam, dt, which)
    npts = len(v)
    n = npts if n is None else n
    src = np.arange(n) % npts
    v, exact, y0 = v[src], exact[:, src], y0[src]
    rng = np.random.default_rng([20250301, 32 if dt == "f32" else 64, n])
    with np.errstate(over="ignore", invalid="ignore"):
        if fam == "dist":
            pred = np.where(y0, v, (rng.integers(-8, 9, n) / 8).astype(T)).astype(T)
            y = np.where(y0, T(0), pred - v).astype(T)
            assert np.array_equal(pred - y, v), "pred - y == d exactly in T"
        else:
            y = np.array(MARGIN_Y, T)[np.arange(n) % 4]
            pred = (v / y).astype(T)
            assert np.array_equal(y * pred, v), "y * pred == a exactly in T"
    b = Block()
    b.family, b.dt, b.n, b.src, b.v, b.y, b.exact = fam, dt, n, src, v, y, exact
    b.pred = pred
    b.x1 = (pred - T(shift)).astype(T)
    assert np.array_equal(b.x1 + T(shift), pred), "x1 + shift == pred exactly in T"
    assert np.isfinite(b.x1).all() and np.isfinite(y).all()
    _BLOCKS[key] = b
    return b


def weights(dt, n, pow2):
    """Powers of two in {0.5, 1, 2} (w l / w stays exact per row) or uniform(0.5, 2) in T (for the sums)."""
    rng = np.random.default_rng([77, n, int(pow2)])
    if pow2:
        return np.array([0.5, 1.0, 2.0], NP[dt])[rng.integers(0, 3, n)]
    return rng.uniform(0.5, 2.0, n).astype(NP[dt])


# ---- the bars ---------------------------------------------------------------------------------------
def row_errors(kind, dt, got, exact, x):
    """Per row, |got - exact| - tiny in units of eps max(|exact|, floor): at most bar(kind) where the row meets
    its bar.  got and exact finite."""
    got, exact = np.asarray(got, np.float64), np.asarray(exact, np.float64)
    scale = np.maximum(np.abs(exact), floor(kind, x, dt))
    excess = np.maximum(np.abs(got - exact) - TINY[dt], 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(excess == 0, 0.0, excess / (EPS[dt] * scale))


def check_rows(kind, dt, got, exact, x, what=""):
    """Asserts the per-row bar (and equality with the exact value rounded to T for EXACT_KINDS); returns the
    worst multiple of eps * scale."""
    e = row_errors(kind, dt, got, exact, x)
    worst = float(e.max(initial=0.0))
    i = int(np.argmax(e)) if len(e) else 0
    assert worst <= bar(kind), (what, kind, dt, worst, float(np.asarray(x)[i]), float(np.asarray(got)[i]), float(exact[i]))
    if kind in EXACT_KINDS:
        want = np.asarray(exact, np.float64).astype(NP[dt])
        bad = np.nonzero(np.asarray(got).astype(NP[dt]) != want)[0]
        assert not len(bad), (what, kind, dt, [(float(np.asarray(x)[j]), float(np.asarray(got)[j]), float(want[j])) for j in bad[:5]])
    return worst


def mean_reference(kind, dt, exact, x, w=None):
    """(fsum(w l) / fold(w), fsum(w max(|l|, floor)) / fsum(w)) in Float64; fold(w) is the library's
    denominator, the weights added one by one in Float64 in the order given (the module docstring)."""
    exact = np.asarray(exact, np.float64)
    w64 = np.ones(len(exact)) if w is None else np.asarray(w, np.float64)
    sw = math.fsum(w64)
    want = math.fsum(w64 * exact) / float(np.cumsum(w64)[-1])  # (cumsum adds sequentially)
    scale = math.fsum(w64 * np.maximum(np.abs(exact), floor(kind, x, dt))) / sw
    return want, scale


def check_mean(kind, dt, got, exact, x, w=None, what=""):
    """Asserts the bar of a mean; returns the error as a multiple of eps * scale."""
    want, scale = mean_reference(kind, dt, exact, x, w)
    err = max(abs(float(got) - want) - TINY[dt], 0.0)
    mult = 0.0 if err == 0 else err / (EPS[dt] * scale)
    assert mult <= bar(kind), (what, kind, dt, mult, float(got), want)
    return mult


def classes(v):
    """0 finite, 1 +Inf, 2 -Inf, 3 NaN."""
    v = np.asarray(v, np.float64)
    return np.where(np.isnan(v), 3, np.where(v == np.inf, 1, np.where(v == -np.inf, 2, 0)))


CLASS_NAMES = ("finite", "+Inf", "-Inf", "NaN")


def param_loss(sr):
    """PAR_KIND at PAR_P0: the loss object of the parameter block."""
    return getattr(sr, GEN.PAR_KIND + "Loss")(GEN.PAR_P0)


def oracle_rows(oracle, sr, kind, blk, loss=None):
    """The CPU restatement's l(pred_i, y_i) in T on the rows of a Block."""
    ls = (loss or loss_object(sr, kind)).c_struct()
    return oracle.loss_rows(blk.pred, blk.y, kind=ls.kind, p0=ls.p0)


def report(test, kind, dt, mult, extra=""):
    print(f"LOSS_ERR {test} {kind} {dt}{extra} {mult:.2f}")


def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.uint64)
