"""srhip_eval_loss_grad_expr and srhip_optimize_constants_expr on the device: exact constant gradients and
the batched constant optimiser under a loss given as an expression (csrc/srhip_grad_lossx.hip)."""
import math

import numpy as np
import pytest

import srhip
from srhip import _lib
from srhip import api

import loss_expr_common as X
import loss_expr_grad_common as G
from loss_expr_grad_common import DTYPES, DT_IDS, bits, flat, program, x

pytestmark = pytest.mark.gpu


# ---- 1. bits of the built-in L2 ----------------------------------------------------------------------------
def _l2_pairs(ctx, dtype, trees, Xd, y, w, idx, monkeypatch):
    """Every (weighted, idx, tangent width) combination: the expression's triple and the built-in's."""
    ds = {False: srhip.DeviceDataset(ctx, Xd, y), True: srhip.DeviceDataset(ctx, Xd, y, w)}
    prog = program(ctx, trees, dtype)
    out = []
    for weighted in (False, True):
        expr = G.l2_expr(weighted)
        for rows in (None, idx):
            per_kt = []
            for kt in ("4", "8"):
                monkeypatch.setenv("SRHIP_GRAD_KT", kt)
                want = prog.eval_loss_grad(ds[weighted], srhip.L2DistLoss(), rows)
                got = prog.eval_loss_grad(ds[weighted], expr, rows)
                assert G.same_bits(got, want), (weighted, rows is None, kt, got[0], want[0])
                per_kt.append(got)
            assert G.same_bits(per_kt[0], per_kt[1])
            out.append(per_kt[0])
    monkeypatch.delenv("SRHIP_GRAD_KT")
    prog.close()
    return out


@pytest.mark.parametrize("m", [1, 63, 64, 65, 255, 256, 257, 1000])
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_l2_expression_has_the_builtin_bits(ctx, dtype, m, monkeypatch):
    """square(p - t) and w * square(p - t): every step of the dual program is exact where the built-in's is,
    so loss, every gradient component and ok are srhip_eval_loss_grad's bits under SRHIP_LOSS_L2."""
    Xd, y, w, idx = G.edge_data(dtype, m)
    res = _l2_pairs(ctx, dtype, G.edge_population(False), Xd, y, w, idx, monkeypatch)
    for loss, grads, ok in res:
        assert ok.tolist() == [True, True, False, False, True]
        assert np.all(np.isposinf(loss[[2, 3]])) and not np.any(flat(grads[2:4]))
        assert np.isfinite(loss[[0, 1, 4]]).all() and len(grads[0]) == 0 and len(grads[1]) == 9
        assert np.all(flat(grads[1:2]) != 0)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_l2_expression_bits_on_the_derived_view(ctx, dtype, monkeypatch):
    m = 8192 + 65
    Xd, y, w, idx = G.edge_data(dtype, m)
    idx = np.concatenate([idx, idx])[:8192 + 1]  # the gathered view is above the derived view's threshold too
    res = _l2_pairs(ctx, dtype, G.edge_population(True), Xd, y, w, idx, monkeypatch)
    for loss, grads, ok in res:
        assert ok.tolist() == [True, True, False, False, True, True] and np.all(flat(grads[5:6]) != 0)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_l2_expression_bits_with_a_copied_chunk_list(ctx, dtype, monkeypatch):
    """More than 96 chunks: the (tree, first constant) list is copied to the device, not inline."""
    trees = [x(1) * (0.1 + 0.05 * k) + x(2) * (1.0 - 0.03 * k) + (0.01 * k) for k in range(100)]
    trees[7], trees[50] = G.row_failing(), G.nine_constants()
    Xd, y, w, idx = G.edge_data(dtype, 300)
    res = _l2_pairs(ctx, dtype, trees, Xd, y, w, idx, monkeypatch)
    assert all(ok.sum() == 99 for _, _, ok in res)


# ---- 2. position independence --------------------------------------------------------------------------------
def _subject():
    return x(1) * x(1) * 0.9 + srhip.Node("cos", x(2)) * 1.5 - x(3) * 0.25 + 0.1


def _neighbours(n, failing):
    out = srhip.random_population(n, G.tree_options(), 3, np.float32, seed=11, max_size=12)
    if failing:
        for k in range(0, n, 3):
            out[k] = G.row_failing()
        for k in range(1, n, 5):
            out[k] = G.static_failing()
    return out


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_position_independence(ctx, dtype):
    """abs(p - t)^2.5 (a libm operator): the subject's loss and gradient bits alone, among neighbours, at
    another position and beside failed trees."""
    Xd, y, _, _ = G.edge_data(dtype, 1000)
    ds = srhip.DeviceDataset(ctx, Xd, y)
    loss = G.lp_expr()
    alone = program(ctx, [_subject()], dtype).eval_loss_grad(ds, loss)
    assert alone[2][0] and np.isfinite(alone[0][0]) and len(alone[1][0]) == 4 and np.all(alone[1][0] != 0)
    for failing in (False, True):
        for pos in (0, 18, 36):
            trees = _neighbours(37, failing)
            trees[pos] = _subject()
            l, g, ok = program(ctx, trees, dtype).eval_loss_grad(ds, loss)
            assert ok[pos] and bits(l[pos]) == bits(alone[0][0]), (failing, pos)
            assert np.array_equal(bits(g[pos]), bits(alone[1][0])), (failing, pos)
            if failing:
                bad = [k for k in range(37) if k != pos and (k % 3 == 0 or k % 5 == 1)]
                assert not ok[bad].any() and np.all(np.isposinf(l[bad])) and not np.any(flat([g[k] for k in bad]))


# ---- 3. every built-in as an expression ------------------------------------------------------------------------
def _builtin_case(ctx, dtype, case, weighted):
    """(expression triple, built-in triple, S_k) of one CASES row in dtype."""
    name, inst, build, _, family = case
    pred, y, w = X.inputs(family, dtype)
    z = np.random.default_rng(77).standard_normal(len(pred)).astype(dtype)
    Xd = np.stack([pred, z])
    ds = srhip.DeviceDataset(ctx, Xd, y, w) if weighted else srhip.DeviceDataset(ctx, Xd, y)
    prog = program(ctx, [(x(1) + x(2) * 0.0) * 1.0], dtype)
    lopts = X.options()
    expr = srhip.ExprLoss(X.W() * build(), lopts, nargs=3) if weighted else srhip.ExprLoss(build(), lopts)
    got = prog.eval_loss_grad(ds, expr)
    want = prog.eval_loss_grad(ds, inst)
    dp, dg, dok = prog.eval_grad_predict(ds)
    assert dok[0] and np.array_equal(dp[0], pred)  # the tree's prediction is pred exactly
    wabs = np.abs(w.astype(np.float64)) if weighted else np.ones(len(pred))
    den = float(wabs.sum()) if weighted else float(len(pred))
    dl = G.host_dloss_abs(srhip.ExprLoss(build(), lopts), pred, y)
    S = G.scale(wabs, dl, dg[0], den)
    prog.close()
    return got, want, S


@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weighted"])
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("case", X.CASES, ids=X.CASE_IDS)
def test_every_builtin_as_an_expression(ctx, case, dtype, weighted):
    """The expression's gradient against the built-in's for the losses.py instance, on the tree
    (x1 + c1 x2) c2 at c = (0, 1): prediction pred exactly, per-row derivatives z and pred.  Differences are
    measured against S_k = sum_i |w_i| |dl_i| |g_ik| / den (g from eval_grad_predict, |dl_i| a Float64 central
    difference of the expression's host callable: a scale only), the bar F32_REL / F64_REL times S_k; the
    losses by the same bars relatively.  (Every Float32 case meets the bar -- the largest measured difference is
    1e-8 S_k, LogitMarginLoss -- so none takes the Float64 detour the bar's fallback would be.)"""
    bar = G.rel_bar(dtype)
    got, want, S = _builtin_case(ctx, dtype, case, weighted)
    assert got[2][0] and want[2][0]
    ge, gb = np.asarray(got[1][0]), np.asarray(want[1][0])
    print(case[0], np.dtype(dtype).name, "weighted" if weighted else "unweighted", "loss rel",
          abs(got[0][0] - want[0][0]) / abs(want[0][0]), "grad |diff| / S", np.abs(ge - gb) / np.maximum(S, 1e-300))
    assert abs(got[0][0] - want[0][0]) <= bar * abs(want[0][0])
    assert np.all(S > 0) or case[0] == "ZeroOneLoss"
    assert np.all(np.abs(ge - gb) <= bar * S), (ge, gb, S)


# ---- 4. a loss that is no built-in ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_log_cosh_against_tanh(ctx, dtype):
    """log(cosh(p - t)): d / dc_k = fsum(tanh(pred_i - y_i) g_ik) / m in Float64 from the device's own
    eval_grad_predict output, against S_k = sum_i |tanh| |g_ik| / m."""
    m = 1000
    Xd, y, _, _ = G.edge_data(dtype, m)
    ds = srhip.DeviceDataset(ctx, Xd, y)
    prog = program(ctx, [_subject(), G.nine_constants()], dtype)
    loss = srhip.ExprLoss(X.N("log", X.N("cosh", X.diff())), X.options())
    l, g, ok = prog.eval_loss_grad(ds, loss)
    pred, dg, pok = prog.eval_grad_predict(ds)
    assert ok.all() and pok.all()
    bar = G.rel_bar(dtype)
    for t in range(2):
        th = np.tanh(pred[t].astype(np.float64) - y.astype(np.float64))
        gt = np.asarray(dg[t], dtype=np.float64)
        want = np.array([math.fsum(th * gt[k]) / m for k in range(gt.shape[0])])
        S = G.scale(np.ones(m), np.abs(th), gt, float(m))
        print("log cosh", np.dtype(dtype).name, t, np.abs(g[t] - want) / S)
        assert np.all(np.abs(g[t] - want) <= bar * S), (t, g[t], want, S)
        lw = math.fsum(np.log(np.cosh(pred[t].astype(np.float64) - y.astype(np.float64)))) / m
        assert abs(l[t] - lw) <= bar * abs(lw)


# ---- 5. non-finite losses ----------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_non_finite_losses_are_no_failure(ctx, dtype):
    Xd, y, _, _ = G.edge_data(dtype, 700)
    ds = srhip.DeviceDataset(ctx, Xd, y)
    trees = [x(1) * 1.5 + x(2), G.row_failing(), x(1) * x(3) + 0.5, G.row_failing() + 0.5]
    prog = program(ctx, trees, dtype)
    l2 = prog.eval_loss_grad(ds, G.l2_expr())
    assert ((1.5 * Xd[0] + Xd[1] - y) < 0).any()
    l, g, ok = prog.eval_loss_grad(ds, srhip.ExprLoss(X.N("sqrt", X.diff()), X.options()))
    assert np.array_equal(ok, l2[2]) and ok.tolist() == [True, False, True, False]
    assert np.isnan(l[0]) and np.isnan(l[2])
    assert np.all(np.isposinf(l[[1, 3]])) and not np.any(flat([g[1], g[3]]))
    assert ctx.last_kernel_ms() >= 0


# ---- 6. the optimiser, bit for bit ---------------------------------------------------------------------------
def _line_problem(dtype, m=400):
    rng = np.random.default_rng(2)
    Xd = rng.standard_normal((2, m)).astype(dtype)
    y = (2.0 * Xd[0] + 1.0).astype(dtype)
    return Xd, y


def _far_trees():
    return [x(1) * 1.2 + 0.3, x(1) * 0.7, x(1) + x(2), (x(1) + 0.2) * 1.5 + x(2) * 0.4, G.row_failing() + 0.5,
            x(1) * -0.5 + 3.0]


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_optimiser_equals_builtin_l2_bit_for_bit(ctx, dtype):
    """square(p - t) against SRHIP_LOSS_L2 with explicit starts: the same objective bits give the same
    trajectory, so the constants left in the program, improved and fcalls are identical; out_loss comes from two
    evaluators that sum in different orders and is held by the standing bars."""
    Xd, y = _line_problem(dtype)
    ds = srhip.DeviceDataset(ctx, Xd, y)
    bar = G.rel_bar(dtype)
    for rows in (None, np.random.default_rng(3).integers(0, 400, size=150)):
        pa, pb = program(ctx, _far_trees(), dtype), program(ctx, _far_trees(), dtype)
        nall = int(pa.num_constants().sum())
        x0 = np.concatenate(pa.get_constants())
        starts = np.stack([x0 * (1 + 0.5 * r) for r in np.random.default_rng(5).standard_normal((2, nall))])
        base, _ = pa.eval_loss(ds, srhip.L2DistLoss(), rows)
        la, ia, fa = pa.optimize_constants(ds, srhip.L2DistLoss(), iterations=8, nrestarts=2, idx=rows, starts=starts)
        lb, ib, fb = pb.optimize_constants(ds, G.l2_expr(), iterations=8, nrestarts=2, idx=rows, starts=starts)
        assert np.array_equal(bits(np.concatenate(pa.get_constants())), bits(np.concatenate(pb.get_constants())))
        assert np.array_equal(ia, ib) and np.array_equal(fa, fb)
        assert ia.tolist() == [True, True, False, True, False, True] and fa[2] == 0
        # the margin the comparison relies on: no acceptance sits on the edge between the two baselines
        assert np.all(la[ia] < 0.5 * base[ia])
        for t in range(len(la)):
            if np.isfinite(la[t]):
                assert abs(la[t] - lb[t]) <= bar * max(abs(la[t]), np.finfo(dtype).tiny), (t, la[t], lb[t])
            else:
                assert la[t] == lb[t]
        pa.close()
        pb.close()


# ---- 7. the optimiser's invariants ----------------------------------------------------------------------------
@pytest.mark.parametrize("build", [lambda: X.N("abs", X.diff()) ** X.C(2.5), lambda: X.N("sqrt", X.N("abs", X.diff()))],
                         ids=["lp2.5", "sqrt_abs"])
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_optimiser_invariants(ctx, dtype, build):
    Xd, y = _line_problem(dtype)
    ds = srhip.DeviceDataset(ctx, Xd, y)
    loss = srhip.ExprLoss(build(), X.options())
    prog = program(ctx, _far_trees(), dtype)
    before = np.concatenate(prog.get_constants())
    nconst = prog.num_constants()
    base, _ = prog.eval_loss(ds, loss)
    out, imp, fc = prog.optimize_constants(ds, loss, iterations=8, nrestarts=2, seed=9)
    again, _ = prog.eval_loss(ds, loss)
    assert np.array_equal(bits(out), bits(again))
    assert imp[0] and not imp[2] and not imp[4]
    assert np.all(out[imp] < base[imp])
    after = np.concatenate(prog.get_constants())
    off = np.concatenate([[0], np.cumsum(nconst)])
    for t in range(prog.ntrees):
        if not imp[t]:
            assert np.array_equal(bits(after[off[t]:off[t + 1]]), bits(before[off[t]:off[t + 1]]))
            assert bits(out[t]) == bits(base[t])
    prog.close()


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_optimiser_never_accepts_nan(ctx, dtype):
    """sqrt(p - t) is NaN wherever a prediction lies below its target: a NaN objective counts as +Inf inside
    the optimiser, so the call returns, and a tree is left unchanged or strictly improved."""
    Xd, y = _line_problem(dtype)
    ds = srhip.DeviceDataset(ctx, Xd, y)
    loss = srhip.ExprLoss(X.N("sqrt", X.diff()), X.options())
    # tree 0 starts at a NaN loss, tree 1 at a finite one (p - t = 4 on every row)
    trees = [x(1) * 1.2 + 0.3, x(1) * 2.0 + 5.0]
    prog = program(ctx, trees, dtype)
    base, bok = prog.eval_loss(ds, loss)
    assert bok.all() and np.isnan(base[0]) and abs(base[1] - 2.0) < 1e-3
    before = np.concatenate(prog.get_constants())
    starts = np.array([[2.0, 5.0, 1.2, 0.3], [2.0, 9.0, 2.0, 6.0]])
    out, imp, fc = prog.optimize_constants(ds, loss, iterations=8, nrestarts=2, starts=starts)
    after = np.concatenate(prog.get_constants())
    again, _ = prog.eval_loss(ds, loss)
    assert np.array_equal(bits(out), bits(again)) and (fc >= 0).all()
    for t in range(2):
        if imp[t]:
            assert out[t] < base[t] and not np.isnan(out[t])
        else:
            assert np.array_equal(bits(after[2 * t:2 * t + 2]), bits(before[2 * t:2 * t + 2]))
    assert not imp[0]  # nothing compares below a NaN baseline
    assert imp[1] and out[1] < base[1]
    prog.close()


# ---- 8. errors -------------------------------------------------------------------------------------------------
def _raw(ctx, ds, prog, loss, dtype, which, null_out=False):
    lib = _lib.load()
    nt = prog.ntrees
    out, ok, grad = np.empty(nt), np.empty(nt, np.uint8), np.empty(max(1, int(prog.num_constants().sum())))
    if which == "grad":
        rc = lib.srhip_eval_loss_grad_expr(ctx.handle, ds.handle, prog.handle, loss.handle(dtype), None, 0, _lib.ptr(out),
                                           None if null_out else _lib.ptr(grad), _lib.ptr(ok))
    else:
        import ctypes
        opt = _lib.OptimOptions(2, 1, 0, 1e-8)
        imp, fc = np.empty(nt, np.uint8), np.empty(nt, np.int64)
        rc = lib.srhip_optimize_constants_expr(ctx.handle, ds.handle, prog.handle, loss.handle(dtype), None, 0,
                                               ctypes.byref(opt), None, None, None if null_out else _lib.ptr(out),
                                               _lib.ptr(imp), _lib.ptr(fc))
    return rc, lib.srhip_last_error().decode() if rc else ""


@pytest.mark.parametrize("which", ["grad", "optim"])
def test_errors(ctx, which):
    m = 300
    rng = np.random.default_rng(3)
    Xd = rng.standard_normal((2, m)).astype(np.float32)
    y, w = rng.standard_normal(m).astype(np.float32), rng.uniform(1, 2, m).astype(np.float32)
    ds, dsw = srhip.DeviceDataset(ctx, Xd, y), srhip.DeviceDataset(ctx, Xd, y, w)
    prog = program(ctx, [x(1) * 1.5 + x(2), x(1) * x(2) + 0.5], np.float32)
    before = np.concatenate(prog.get_constants())
    l2, l3 = G.l2_expr(False), G.l2_expr(True)
    rc, msg = _raw(ctx, ds, prog, l3, np.float32, which)
    assert rc == _lib.ERR_INVALID and "nargs = 2" in msg
    rc, msg = _raw(ctx, dsw, prog, l2, np.float32, which)
    assert rc == _lib.ERR_INVALID and "nargs = 3" in msg
    rc, msg = _raw(ctx, ds, prog, l2, np.float64, which)  # a Float64 expression for a Float32 program
    assert rc == _lib.ERR_INVALID and "dtype" in msg
    rc, msg = _raw(ctx, ds, prog, l2, np.float32, which, null_out=True)
    assert rc == _lib.ERR_INVALID and "null" in msg
    iopts = srhip.Options(binary_operators=("+", "*"), unary_operators=())
    Xi = rng.integers(-5, 6, size=(2, m)).astype(np.int32)
    dsi = srhip.DeviceDataset(ctx, Xi, Xi[0])
    progi = program(ctx, [x(1) + x(2)], np.int32, iopts)
    rc, msg = _raw(ctx, dsi, progi, l2, np.float32, which)
    assert rc == _lib.ERR_UNSUPPORTED and "Int32" in msg
    # a failed call leaves the constants unchanged, and the context still works
    assert np.array_equal(bits(np.concatenate(prog.get_constants())), bits(before))
    assert G.same_bits(prog.eval_loss_grad(ds, l2), prog.eval_loss_grad(ds, srhip.L2DistLoss()))


# ---- 9. the mirror ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["one", "list", "batching"])
def test_mirror_stays_on_the_device(ctx, mode, monkeypatch):
    """api.optimize_constants under Options(elementwise_loss=ExprLoss(...)) never reaches the host optimiser;
    an improved member's loss and score are re-computed."""
    from srhip import host_optim

    def boom(*a, **k):
        raise AssertionError("the host optimiser ran")

    monkeypatch.setattr(host_optim, "optimize", boom)
    Xd, y = _line_problem(np.float64)
    dataset = srhip.Dataset(Xd, y)
    opts = srhip.Options(elementwise_loss=G.lp_expr(), batching=mode == "batching", batch_size=50, **G.TREE_OPS)
    api.update_baseline_loss(dataset, opts)
    calls = []
    orig = srhip.Program.optimize_constants
    monkeypatch.setattr(srhip.Program, "optimize_constants",
                        lambda self, *a, **k: (calls.append(self.ntrees), orig(self, *a, **k))[1])
    members = [G.Member(t) for t in (x(1) * 1.2 + 0.3, x(1) * 0.7, x(1) * -0.5 + 3.0)]
    before = [api.eval_loss(mb.tree, dataset, opts) for mb in members]
    arg = members[0] if mode == "one" else members
    res, evals = api.optimize_constants(dataset, arg, opts, rng=np.random.default_rng(0))
    assert evals > 0
    assert calls == {"one": [1], "list": [3], "batching": [1, 1, 1]}[mode]
    for mb, b in zip(members[:1] if mode == "one" else members, before):
        full = api.eval_loss(mb.tree, dataset, opts)
        assert full < b, (b, full)
        assert mb.birth != -1 and np.isfinite(mb.loss) and mb.loss > 0
        if mode != "batching":  # (batching: the member's loss is the loss on its own minibatch)
            assert float(mb.loss) == float(full)
        assert float(mb.score) == float(api.loss_to_score(mb.loss, dataset.use_baseline, dataset.baseline_loss, mb, opts))
