"""srhip_eval_loss_expr on the device: a loss given as an expression, evaluated per row over predictions
that stay on the device and reduced there (csrc/srhip_lossx.hip)."""
import ctypes
import math
import os

import numpy as np
import pytest

import srhip
from srhip import _lib
from srhip import api

import loss_expr_common as X
from conftest import load_cases

pytestmark = pytest.mark.gpu

F32_REL = 1e-6   # the project's standing bars (tests/test_gpu_parity.py)
F64_REL = 1e-12
B = 4096         # LOSSX_BLOCK_ROWS of csrc/srhip_lossx.h (checked against the library's getter below)
DTYPES = [np.float32, np.float64]
DT_IDS = ["f32", "f64"]

TREE_OPS = dict(binary_operators=("+", "-", "*", "/"), unary_operators=("cos", "exp"))


def _rel(a, b):
    if a == b or (math.isnan(a) and math.isnan(b)):
        return 0.0
    return abs(a - b) / max(abs(b), 1e-300)


def _bits(v):
    return np.asarray(v, dtype=np.float64).view(np.uint64)


def _x(i):
    return srhip.Node(feature=i)


def _program(ctx, trees, dtype, opts=None):
    opts = opts or srhip.Options(**TREE_OPS)
    nodes, offs = srhip.flatten(trees, opts, dtype)
    return srhip.Program(ctx, nodes, offs, opts, dtype)


def test_block_rows_constant():
    assert _lib.load().srhip_lossx_block_rows() == B


# ---- 1. the reference's known answer ------------------------------------------------------------------
def test_reference_lp_known_answer(ctx):
    """test/test_losses.jl of the reference: abs(x - y)^2.5 and w * abs(x - y)^2.5 as function losses."""
    cases, ex = load_cases("losses.npz")
    cs = next(c for c in cases if int(c["kind"]) == _lib.LOSS["LP"])
    opts = srhip.Options(binary_operators=("+",), unary_operators=("cos",))
    prog = srhip.Program(ctx, ex["nodes"], np.array([0, len(ex["nodes"])], np.int64), opts, np.float32)
    lx = X.options()
    lp = X.N("abs", X.diff()) ** X.C(2.5)
    builtin = srhip.LPDistLoss(float(cs["p0"]))
    ds = srhip.DeviceDataset(ctx, cs["X"], cs["y"])
    l, ok = prog.eval_loss(ds, srhip.ExprLoss(lp, lx))
    ref, _ = prog.eval_loss(ds, builtin)
    assert ok[0] and abs(l[0] - float(cs["expected_mean"])) < 1e-6 and _rel(l[0], ref[0]) < F32_REL
    dsw = srhip.DeviceDataset(ctx, cs["X"], cs["y"], cs["w"])
    l, ok = prog.eval_loss(dsw, srhip.ExprLoss(X.W() * (X.N("abs", X.diff()) ** X.C(2.5)), lx))
    ref, _ = prog.eval_loss(dsw, builtin)
    assert ok[0] and abs(l[0] - float(cs["expected_weighted"])) < 1e-6 and _rel(l[0], ref[0]) < F32_REL


# ---- 2. exact sums -------------------------------------------------------------------------------------
# integer features (|v| <= 16, within the |v| <= 64 that keeps every value below Float32's 2^24), targets
# j mod 97, weights 1..7: every prediction, every loss value and every partial sum is an integer that T and
# double hold exactly, so any summation order gives the same double and equality is exact
INT_FORMS = [
    (lambda k: _x(1) + _x(2) + float(k), lambda F, k: F[0] + F[1] + k),
    (lambda k: _x(1) * _x(2) - _x(3) + float(k), lambda F, k: F[0] * F[1] - F[2] + k),
    (lambda k: _x(3) - _x(1) * float(k), lambda F, k: F[2] - F[0] * k),
    (lambda k: _x(2) * _x(3) + _x(1), lambda F, k: F[1] * F[2] + F[0]),
    (lambda k: _x(1) + float(k), lambda F, k: F[0] + k),
]
INT_LOSSES = [  # (expression, integer value of (p, t, w), reads the weight)
    (lambda: X.C(1.0), lambda p, t, w: np.ones_like(p), False),
    (lambda: X.T_(), lambda p, t, w: t, False),
    (lambda: X.diff(), lambda p, t, w: p - t, False),
    (lambda: X.N("square", X.diff()), lambda p, t, w: (p - t) ** 2, False),
    (lambda: X.N("abs", X.diff()), lambda p, t, w: np.abs(p - t), False),
    (lambda: X.N("max", X.diff(), X.C(0.0)) * X.C(3.0), lambda p, t, w: np.maximum(p - t, 0) * 3, False),
    (lambda: X.W() * X.N("square", X.diff()), lambda p, t, w: w * (p - t) ** 2, True),
]


def _int_population(n):
    nb = len(INT_FORMS)
    return [INT_FORMS[k % nb][0](k // nb) for k in range(n)], [(INT_FORMS[k % nb][1], k // nb) for k in range(n)]


@pytest.mark.parametrize("m", [1, 63, 64, 65, 255, 256, 257, B - 1, B, B + 1, 3 * B + 1])
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_exact_integer_sums(ctx, dtype, m):
    rng = np.random.default_rng(1000 + m)
    F = rng.integers(-16, 17, size=(3, m))
    y = np.arange(m) % 97
    w = rng.integers(1, 8, size=m)
    idx = rng.integers(0, m, size=m)
    idx[-1] = idx[0]  # a duplicate at every size
    lopts = X.options()
    losses = [(srhip.ExprLoss(b(), lopts), f, wt) for b, f, wt in INT_LOSSES]
    ds = {False: srhip.DeviceDataset(ctx, F.astype(dtype), y.astype(dtype)),
          True: srhip.DeviceDataset(ctx, F.astype(dtype), y.astype(dtype), w.astype(dtype))}
    for npop in (1, 2, 37):
        trees, forms = _int_population(npop)
        prog = _program(ctx, trees, dtype)
        for rows in (None, idx):
            sel = slice(None) if rows is None else rows
            Fs, ys, ws = F[:, sel], y[sel], w[sel]
            preds = [f(Fs, k) for f, k in forms]
            for loss, value, weighted in losses:
                got, ok = prog.eval_loss(ds[weighted], loss, rows)
                assert ok.all()
                den = int(ws.sum()) if weighted else len(ys)
                want = np.array([int(value(p, ys, ws).sum()) / den for p in preds])
                assert np.array_equal(_bits(got), _bits(want)), (npop, rows is None, loss, got, want)
        prog.close()


# ---- 3. the reduction contract, 4. the derived bound ---------------------------------------------------
M3 = 3 * B + 1


def _real_data(dtype):
    rng = np.random.default_rng(7)
    Xd = rng.standard_normal((3, M3)).astype(dtype)
    y = (2 * np.cos(Xd[1]) + Xd[0] ** 2 - 2).astype(dtype)
    return Xd, y


def _subject():
    return _x(1) * _x(1) + srhip.Node("cos", _x(2)) * 1.5 - _x(3) * 0.25


def _neighbours(n, failing):
    opts = srhip.Options(**TREE_OPS)
    out = srhip.random_population(n, opts, 3, np.float32, seed=11, max_size=12)
    if failing:
        for k in range(0, n, 3):
            out[k] = _x(1) / (_x(2) - _x(2))       # fails on the first row
        for k in range(1, n, 5):
            out[k] = _x(1) + srhip.Node(val=np.inf)  # fails before any row is evaluated
    return out


CONTRACT_LOSSES = [lambda: X.N("abs", X.diff()) ** X.C(2.5), lambda: X.N("log", X.N("cosh", X.diff()))]


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_reduction_contract(ctx, dtype):
    """A tree's loss is the same bits alone, at any position among 37, beside failing trees, and with idx =
    arange(m) instead of no idx."""
    Xd, y = _real_data(dtype)
    ds = srhip.DeviceDataset(ctx, Xd, y)
    lopts = X.options()
    for build in CONTRACT_LOSSES:
        loss = srhip.ExprLoss(build(), lopts)
        alone, ok = _program(ctx, [_subject()], dtype).eval_loss(ds, loss)
        assert ok[0] and np.isfinite(alone[0])
        for failing in (False, True):
            for pos in (0, 18, 36):
                trees = _neighbours(37, failing)
                trees[pos] = _subject()
                prog = _program(ctx, trees, dtype)
                got, gok = prog.eval_loss(ds, loss)
                assert gok[pos] and _bits(got[pos]) == _bits(alone[0]), (failing, pos, got[pos], alone[0])
                if failing:
                    bad = [k for k in range(37) if k != pos and (k % 3 == 0 or k % 5 == 1)]
                    assert not gok[bad].any() and np.all(np.isposinf(got[bad]))
                if pos == 18:
                    again, aok = prog.eval_loss(ds, loss, np.arange(M3))
                    assert np.array_equal(aok, gok) and np.array_equal(_bits(again), _bits(got))
                prog.close()


EXACT_CLASS = ["L2DistLoss", "L1DistLoss", "HuberLoss(1)", "L2EpsilonInsLoss(0.5)", "QuantileLoss(0.3)",
               "ModifiedHuberLoss"]


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_derived_bound(ctx, dtype):
    """|device - fsum(l) / m| <= m 2^-52 fsum(|l|) / m for exact-class expressions, l the host evaluator's values
    on the device's own predictions: the first-order error of any double summation of m exactly converted
    terms is (m - 1) 2^-53 sum|l|; the factor 2 covers the division and the higher-order terms.  For
    log(cosh(.)) and ^, whose values come from two different libms, the standing relative bars."""
    Xd, y = _real_data(dtype)
    ds = srhip.DeviceDataset(ctx, Xd, y)
    trees = [_subject()] + _neighbours(6, False)
    prog = _program(ctx, trees, dtype)
    pred, pok = prog.eval_predict(ds)
    lopts = X.options()
    m = M3
    by_name = {c[0]: c for c in X.CASES}
    for name in EXACT_CLASS:
        loss = srhip.ExprLoss(by_name[name][2](), lopts)
        got, ok = prog.eval_loss(ds, loss)
        assert np.array_equal(ok, pok)
        for t in np.nonzero(ok)[0]:
            l = loss(pred[t], y).astype(np.float64)
            assert abs(got[t] - math.fsum(l) / m) <= m * 2.0 ** -52 * math.fsum(np.abs(l)) / m, (name, t)
    tol = F32_REL if dtype == np.float32 else F64_REL
    for build in CONTRACT_LOSSES:
        loss = srhip.ExprLoss(build(), lopts)
        got, ok = prog.eval_loss(ds, loss)
        for t in np.nonzero(ok)[0]:
            l = loss(pred[t], y).astype(np.float64)
            assert _rel(got[t], math.fsum(l) / m) < tol, (t, got[t])
    prog.close()


# ---- 5. failures and non-finite losses --------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_failed_trees_and_non_finite_losses(ctx, dtype):
    m = B + 7
    rng = np.random.default_rng(5)
    Xd = rng.standard_normal((3, m)).astype(dtype)
    y = rng.standard_normal(m).astype(dtype)
    ds = srhip.DeviceDataset(ctx, Xd, y)
    lopts = X.options()
    l2 = srhip.ExprLoss(X.N("square", X.diff()), lopts)
    good = [_x(1) + _x(2), _x(1) * _x(3)]
    row_fail, static_fail = _x(1) / (_x(2) - _x(2)), _x(1) + srhip.Node(val=np.inf)
    base, bok = _program(ctx, good, dtype).eval_loss(ds, l2)
    assert bok.all()
    got, ok = _program(ctx, [row_fail, good[0], static_fail, good[1], row_fail], dtype).eval_loss(ds, l2)
    assert ok.tolist() == [False, True, False, True, False]
    assert np.all(np.isposinf(got[[0, 2, 4]]))
    assert _bits(got[1]) == _bits(base[0]) and _bits(got[3]) == _bits(base[1])
    assert ctx.last_kernel_ms() >= 0
    # no tree left: no loss launch
    got, ok = _program(ctx, [row_fail, static_fail, row_fail], dtype).eval_loss(ds, l2)
    assert not ok.any() and np.all(np.isposinf(got))
    assert ctx.last_kernel_ms() < 0
    # a non-finite loss value is no failure
    got, ok = _program(ctx, good, dtype).eval_loss(ds, srhip.ExprLoss(X.N("sqrt", X.diff()), lopts))
    assert ((Xd[0] + Xd[1] - y) < 0).any()
    assert ok.all() and np.all(np.isnan(got))
    got, ok = _program(ctx, good, dtype).eval_loss(ds, srhip.ExprLoss(X.C(1.0) / (X.P() - X.P()), lopts))
    assert ok.all() and np.all(np.isposinf(got))


# ---- 6. errors -------------------------------------------------------------------------------------------
def _raw_eval(ctx, ds, prog, loss, dtype):
    out, ok = np.empty(prog.ntrees), np.empty(prog.ntrees, np.uint8)
    rc = _lib.load().srhip_eval_loss_expr(ctx.handle, ds.handle, prog.handle, loss.handle(dtype), None, 0,
                                          _lib.ptr(out), _lib.ptr(ok))
    return rc, _lib.load().srhip_last_error().decode() if rc else ""


def test_errors(ctx, monkeypatch):
    m = 300
    rng = np.random.default_rng(3)
    Xd = rng.standard_normal((2, m)).astype(np.float32)
    y, w = rng.standard_normal(m).astype(np.float32), rng.uniform(1, 2, m).astype(np.float32)
    ds, dsw = srhip.DeviceDataset(ctx, Xd, y), srhip.DeviceDataset(ctx, Xd, y, w)
    prog = _program(ctx, [_x(1) + _x(2), _x(1) * _x(2)], np.float32)
    lopts = X.options()
    l2 = srhip.ExprLoss(X.N("square", X.diff()), lopts)
    l3 = srhip.ExprLoss(X.W() * X.N("square", X.diff()), lopts)
    rc, msg = _raw_eval(ctx, ds, prog, l3, np.float32)
    assert rc == _lib.ERR_INVALID and "nargs = 2" in msg
    rc, msg = _raw_eval(ctx, dsw, prog, l2, np.float32)
    assert rc == _lib.ERR_INVALID and "nargs = 3" in msg
    rc, msg = _raw_eval(ctx, ds, prog, l2, np.float64)  # a Float64 expression for a Float32 program
    assert rc == _lib.ERR_INVALID and "dtype" in msg
    # an Int32 program
    iopts = srhip.Options(binary_operators=("+", "*"), unary_operators=())
    Xi = rng.integers(-5, 6, size=(2, m)).astype(np.int32)
    dsi = srhip.DeviceDataset(ctx, Xi, Xi[0])
    progi = _program(ctx, [_x(1) + _x(2)], np.int32, iopts)
    rc, msg = _raw_eval(ctx, dsi, progi, l2, np.float32)
    assert rc == _lib.ERR_UNSUPPORTED and "Int32" in msg
    # the prediction buffer cap, read per call
    want, wok = prog.eval_loss(ds, l2)
    monkeypatch.setenv("SRHIP_LOSSX_MAX_BYTES", "1024")
    rc, msg = _raw_eval(ctx, ds, prog, l2, np.float32)
    assert rc == _lib.ERR_NOMEM and "1024" in msg and str(2 * m * 4) in msg
    monkeypatch.delenv("SRHIP_LOSSX_MAX_BYTES")
    got, ok = prog.eval_loss(ds, l2)  # the context still works
    assert np.array_equal(ok, wok) and np.array_equal(_bits(got), _bits(want))


# ---- 7. the Python mirror ----------------------------------------------------------------------------------
def _mirror_setup(dtype, m=1500, weighted=False):
    rng = np.random.default_rng(21)
    Xd = rng.standard_normal((3, m)).astype(dtype)
    y = (2 * np.cos(Xd[1]) + Xd[0] ** 2 - 2).astype(dtype)
    w = rng.uniform(0.5, 2.0, m).astype(dtype) if weighted else None
    return srhip.Dataset(Xd, y, weights=w)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_mirror_equals_the_python_callable(dtype, ctx, monkeypatch):
    """api.eval_loss_batch under Options(elementwise_loss=ExprLoss(...)) against the same loss as a Python
    callable (predictions copied to the host, the callable row by row), within the bars of the derived-bound
    test; the ExprLoss path never calls eval_predict."""
    trees = [_subject()] + _neighbours(4, True)
    lopts = X.options()
    m = 1500
    cases = [
        (False, X.N("square", X.diff()), lambda p, t: (p - t) * (p - t), True),
        (False, X.N("abs", X.diff()) ** X.C(2.5), lambda p, t: abs(p - t) ** type(p)(2.5), False),
        (True, X.W() * X.N("square", X.diff()), lambda p, t, w: w * ((p - t) * (p - t)), True),
    ]
    for weighted, expr, fn, exact in cases:
        dataset = _mirror_setup(dtype, m, weighted)
        want, wok = api.eval_loss_batch(trees, dataset, srhip.Options(elementwise_loss=fn, **TREE_OPS))
        eopts = srhip.Options(elementwise_loss=srhip.ExprLoss(expr, lopts), **TREE_OPS)
        with monkeypatch.context() as mp:
            def boom(*a, **k):
                raise AssertionError("predictions were copied to the host")
            mp.setattr(srhip.Program, "eval_predict", boom)
            got, ok = api.eval_loss_batch(trees, dataset, eopts)
            idx = np.arange(0, m, 3)
            goti, _ = api.eval_loss_batch(trees, dataset, eopts, idx=idx)
        wanti, _ = api.eval_loss_batch(trees, dataset, srhip.Options(elementwise_loss=fn, **TREE_OPS), idx=idx)
        assert np.array_equal(ok, wok) and ok[0] and not ok.all()
        for g, wv, rows in ((got, want, m), (goti, wanti, len(idx))):
            for t in range(len(trees)):
                if not ok[t]:
                    assert np.isposinf(g[t]) and np.isposinf(wv[t])
                elif exact:
                    # both are double sums of the same exactly converted terms: each within (rows - 1) 2^-53
                    # sum|l| / den of the exact quotient to first order; l >= 0 here, so sum|l| / den = loss
                    assert abs(g[t] - wv[t]) <= 2 * rows * 2.0 ** -52 * abs(wv[t]), (t, g[t], wv[t])
                else:
                    assert _rel(g[t], wv[t]) < (F32_REL if dtype == np.float32 else F64_REL)


def test_mirror_splits_a_population_over_the_cap(ctx, monkeypatch):
    dtype = np.float32
    dataset = _mirror_setup(dtype, 1500)
    trees = [_subject()] + _neighbours(7, True)
    eopts = srhip.Options(elementwise_loss=srhip.ExprLoss(X.N("abs", X.diff()) ** X.C(2.5), X.options()), **TREE_OPS)
    want, wok = api.eval_loss_batch(trees, dataset, eopts)
    calls = []
    orig = srhip.Program.eval_loss
    monkeypatch.setattr(srhip.Program, "eval_loss", lambda self, *a, **k: (calls.append(self.ntrees), orig(self, *a, **k))[1])
    monkeypatch.setenv("SRHIP_LOSSX_MAX_BYTES", str(3 * 1500 * 4))
    got, ok = api.eval_loss_batch(trees, dataset, eopts)
    assert calls == [3, 3, 2]
    assert np.array_equal(ok, wok) and np.array_equal(_bits(got), _bits(want))
    # a single tree over the cap is the library's error
    monkeypatch.setenv("SRHIP_LOSSX_MAX_BYTES", "1024")
    with pytest.raises(srhip.SrhipError) as ei:
        api.eval_loss_batch(trees[:1], dataset, eopts)
    assert ei.value.code == _lib.ERR_NOMEM


def test_optimize_constants_over_the_device_objective(ctx):
    """The host optimiser (finite differences over eval_loss) with an ExprLoss of L2: its objective runs on
    the device and the constants improve."""
    rng = np.random.default_rng(2)
    Xd = rng.standard_normal((2, 400))
    dataset = srhip.Dataset(Xd, 2.0 * Xd[0] + 1.0)
    opts = srhip.Options(elementwise_loss=srhip.ExprLoss(X.N("square", X.diff()), X.options()), **TREE_OPS)
    tree = _x(1) * 1.2 + 0.3
    before = api.eval_loss(tree, dataset, opts)
    tree, evals = api.optimize_constants(dataset, tree, opts, rng=np.random.default_rng(0))
    after = api.eval_loss(tree, dataset, opts)
    assert evals > 0 and after < 0.5 * before, (before, after)
