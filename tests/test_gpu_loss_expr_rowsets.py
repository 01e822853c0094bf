"""srhip_eval_loss_expr_rowsets, srhip_eval_loss_grad_expr_rowsets and srhip_optimize_constants_expr_rowsets on
the device: a loss given as an expression in batching mode, every tree on a row subset of its own in one call
(csrc/srhip_rowsets_lossx.hip, csrc/srhip_grad_rowsets_lossx.hip).  Every comparison is bit for bit against
the one-tree single-idx expression call on the tree's set."""
import ctypes
import math

import numpy as np
import pytest

import srhip
from srhip import _lib
from srhip import api

import loss_expr_common as X
import loss_expr_grad_common as G
import loss_expr_rowsets_common as R
from loss_expr_grad_common import DTYPES, DT_IDS, bits, program, x

pytestmark = pytest.mark.gpu

N = 3000
BASE_LENGTHS = [1, 2, 50, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025]


def _dataset(ctx, dtype, weighted, n=N, seed=0):
    Xd, y, w, _ = G.edge_data(dtype, n, seed)
    return (srhip.DeviceDataset(ctx, Xd, y, w) if weighted else srhip.DeviceDataset(ctx, Xd, y)), Xd, y, w


# ---- 1. scoring parity ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weighted"])
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_scoring_parity(ctx, dtype, weighted):
    """Sets of every length around the tile, the 256-row statistics step and the cap; static failure, row
    failure, nine constants and cos among the trees.  The hook tells the kernel from the fallback."""
    ds, _, _, _ = _dataset(ctx, dtype, weighted)
    cap = R.score_cap(dtype, 3, weighted)
    lengths = BASE_LENGTHS + [cap - 1, cap, cap + 1]
    trees = R.repeated(G.edge_population(True), len(lengths))
    sets = R.draw_sets(np.random.default_rng(1), N, lengths)
    loss = R.lp_expr(weighted)
    want = R.loop_loss(ctx, trees, dtype, ds, loss, sets)
    oks = [want[t][1] for t in range(6)]
    assert oks == [True, True, False, False, True, True]
    # without the over-cap set: every tree by the kernel
    prog = program(ctx, trees[:-1], dtype)
    got = R.rowsets_loss(prog, ds, loss, sets[:-1])
    assert ctx.rowsets_fallback_trees() == 0
    assert got == {t: want[t] for t in range(len(lengths) - 1)}
    prog.close()
    # with it: one tree through the one-tree call.  (Tree 17 of the repeated population is cos(x1) 0.7 + 0.2.)
    prog = program(ctx, trees, dtype)
    got = R.rowsets_loss(prog, ds, loss, sets)
    assert ctx.rowsets_fallback_trees() == 1
    assert got == want
    prog.close()


# ---- 2. crossing a 4096-row summation block ------------------------------------------------------------------
def test_crossing_a_summation_block(ctx):
    """One Float32 feature, unweighted: the cap is 5120 rows, so sets of 4095, 4096, 4097 and 5120 rows are all
    staged by the kernel, and the last three sum over two blocks of the loss pass."""
    assert _lib.load().srhip_lossx_block_rows() == 4096 and R.score_cap(np.float32, 1, False) == 5120
    n = 6000
    rng = np.random.default_rng(4)
    Xd = rng.standard_normal((1, n)).astype(np.float32)
    y = (Xd[0] * 1.5 + 0.25 * rng.standard_normal(n)).astype(np.float32)
    ds = srhip.DeviceDataset(ctx, Xd, y)
    trees = [x(1) * 1.25 + 0.1, srhip.Node("cos", x(1)) * 0.7 + 0.2, x(1) * x(1) - 0.5, x(1) * 1.5]
    loss = R.lp_expr()
    for lengths, fallback in (([4095, 4096, 4097, 5120], 0), ([4097, 5121, 5120, 50], 1)):
        sets = R.draw_sets(rng, n, lengths)
        want = R.loop_loss(ctx, trees, np.float32, ds, loss, sets)
        prog = program(ctx, trees, np.float32)
        got = R.rowsets_loss(prog, ds, loss, sets)
        assert ctx.rowsets_fallback_trees() == fallback, lengths
        assert got == want, lengths
        assert all(ok and np.isfinite(np.uint64(b).view(np.float64)) for b, ok in got.values())
        prog.close()


# ---- 3. exact integer sums --------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_exact_integer_sums(ctx, dtype):
    """Integer-valued data under square(p - t) on x1 + x2: every term and every partial sum is an exact
    integer, so the loss is the exact integer sum / m whatever the order -- and every row is read once."""
    n = 3000
    rng = np.random.default_rng(8)
    Xd = rng.integers(-9, 10, size=(3, n)).astype(dtype)
    y = rng.integers(-9, 10, size=n).astype(dtype)
    ds = srhip.DeviceDataset(ctx, Xd, y)
    cap = R.score_cap(dtype, 3, False)
    lengths = BASE_LENGTHS + [cap - 1, cap, cap + 1]
    sets = R.draw_sets(rng, n, lengths)
    prog = program(ctx, [x(1) + x(2) for _ in lengths], dtype)
    got, ok = prog.eval_loss_rowsets(ds, G.l2_expr(), sets)
    assert ok.all() and ctx.rowsets_fallback_trees() == 1
    Xi, yi = Xd.astype(np.int64), y.astype(np.int64)
    for t, s in enumerate(sets):
        exact = int(((Xi[0, s] + Xi[1, s] - yi[s]) ** 2).sum())
        assert got[t] == exact / len(s), (len(s), got[t], exact)
    prog.close()


# ---- 4. an independent bound ------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weighted"])
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_independent_bound(ctx, dtype, weighted):
    """An expression of + - * abs square only: the host evaluator's values are the device's.  The device loss
    lies within m 2^-52 sum|l_i| / den of fsum(l) / den over the device's own predictions on the set
    (tests/test_gpu_loss_expr.py::test_derived_bound's bar; den = m, or the weights' exact sum).  Weighted, the
    bar holds to first order too: (m - 1) 2^-53 for each of the two double sums of exactly converted terms and
    2^-53 for the division, (2 m - 1) 2^-53 < m 2^-52 in all."""
    ds, Xd, y, w = _dataset(ctx, dtype, weighted)
    e = X.N("abs", X.diff()) * X.N("square", X.diff()) + X.N("abs", X.diff()) - X.C(0.125) * X.diff()
    loss = srhip.ExprLoss(X.W() * e if weighted else e, X.options())
    cap = R.score_cap(dtype, 3, weighted)
    lengths = [1, 50, 257, 1023, cap]  # (1024 is the smallest cap: Float64 with weights)
    trees = R.repeated([x(1) * x(1) * 0.9 + srhip.Node("cos", x(2)) * 1.5 - x(3) * 0.25 + 0.1, G.nine_constants()],
                       len(lengths))
    sets = R.draw_sets(np.random.default_rng(2), N, lengths)
    prog = program(ctx, trees, dtype)
    got, ok = prog.eval_loss_rowsets(ds, loss, sets)
    assert ok.all() and ctx.rowsets_fallback_trees() == 0
    for t, s in enumerate(sets):
        p1 = program(ctx, [trees[t]], dtype)
        pred, pok = p1.eval_predict(ds, idx=s)
        p1.close()
        assert pok[0]
        l = (loss(pred[0], y[s], w[s]) if weighted else loss(pred[0], y[s])).astype(np.float64)
        m = len(s)
        den = math.fsum(w[s].astype(np.float64)) if weighted else float(m)
        err = abs(got[t] - math.fsum(l) / den)
        bar = m * 2.0 ** -52 * math.fsum(np.abs(l)) / den
        print(np.dtype(dtype).name, weighted, m, "error", err, "bar", bar)
        assert err <= bar, (t, m, got[t])
    prog.close()


# ---- 5. results do not depend on the batch --------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_results_do_not_depend_on_the_batch(ctx, dtype):
    ds, _, _, _ = _dataset(ctx, dtype, False)
    loss = R.lp_expr()
    rng = np.random.default_rng(6)
    opts = G.tree_options()
    trees = srhip.random_population(37, opts, 3, dtype, seed=21, max_size=14)
    trees[3], trees[20] = G.nine_constants(), srhip.Node("cos", x(1)) * 0.7 + 0.2
    sets = R.draw_sets(rng, N, rng.integers(1, 700, size=37))

    def run(order):
        prog = program(ctx, [trees[t] for t in order], dtype)
        got = R.rowsets_loss(prog, ds, loss, [sets[t] for t in order])
        prog.close()
        return {t: got[k] for k, t in enumerate(order)}

    base = run(list(range(37)))
    assert sum(ok for _, ok in base.values()) >= 20
    perm = list(np.random.default_rng(7).permutation(37))
    assert run(perm) == base
    for t in (0, 3, 20, 36):
        assert run([t]) == {t: base[t]}
    assert run([3, 20]) == {3: base[3], 20: base[20]}
    # beside failed trees
    bad = [G.row_failing(), G.static_failing()]
    prog = program(ctx, [bad[0], trees[3], bad[1], trees[20], bad[0]], dtype)
    got = R.rowsets_loss(prog, ds, loss, [sets[0], sets[3], sets[1], sets[20], sets[2]])
    prog.close()
    assert got[1] == base[3] and got[3] == base[20]
    assert all(got[k] == (int(bits(np.inf)[0]), False) for k in (0, 2, 4))


# ---- 6. gradient parity ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kt", ["4", "8"])
@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weighted"])
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_gradient_parity(ctx, dtype, weighted, kt, monkeypatch):
    """Loss, gradient slice and ok of every tree against the one-tree eval_loss_grad on its set, both tangent
    widths; square(p - t) and w * square(p - t) also against the built-in L2's row-set call."""
    monkeypatch.setenv("SRHIP_GRAD_KT", kt)
    ds, _, _, _ = _dataset(ctx, dtype, weighted)
    cap = R.grad_cap(dtype, 3, weighted)
    lengths = [1, 50, 255, 256, 257, 513, cap, cap + 1]
    trees = R.repeated(G.edge_population(True), len(lengths))
    trees[6], trees[7] = G.nine_constants(), G.nine_constants()  # the cap and the cap + 1 carry gradients
    sets = R.draw_sets(np.random.default_rng(3), N, lengths)
    loss = R.lp_expr(weighted)
    want = R.loop_grad(ctx, trees, dtype, ds, loss, sets)
    assert [want[t][2] for t in range(6)] == [True, True, False, False, True, True]
    prog = program(ctx, trees[:-1], dtype)
    got = R.rowsets_grad(prog, ds, loss, sets[:-1])
    assert ctx.rowsets_fallback_trees() == 0
    assert got == {t: want[t] for t in range(len(lengths) - 1)}
    prog.close()
    prog = program(ctx, trees, dtype)
    got = R.rowsets_grad(prog, ds, loss, sets)
    assert ctx.rowsets_fallback_trees() == 1
    assert got == want
    assert any(v != 0 for v in got[6][1]) and any(v != 0 for v in got[7][1])
    # the built-in's bits
    a = prog.eval_loss_grad_rowsets(ds, G.l2_expr(weighted), sets)
    b = prog.eval_loss_grad_rowsets(ds, srhip.L2DistLoss(), sets)
    assert G.same_bits(a, b)
    prog.close()


# ---- 7. optimiser parity ----------------------------------------------------------------------------------------
OPTIM_OPS = dict(binary_operators=("+", "-", "*", "/"), unary_operators=("cos", "exp", "sin"))


def _optim_problem(ctx, dtype, ntrees=40, n=3000, seed=11, max_size=20):
    opts = srhip.Options(**OPTIM_OPS)
    trees = srhip.random_population(ntrees, opts, 3, dtype, seed=seed, max_size=max_size)
    rng = np.random.default_rng(seed + 1)
    Xd = rng.standard_normal((3, n)).astype(dtype)
    y = (np.cos(1.3 * Xd[0]) * 2.0 + Xd[1] * 0.7 - 0.3).astype(dtype)
    lengths = [50] * (ntrees - 4) + [1, 7, 257, 300]
    sets = R.draw_sets(rng, n, lengths)
    seeds = [int(s) for s in rng.integers(0, 2**62, size=ntrees)]
    return opts, trees, srhip.DeviceDataset(ctx, Xd, y), sets, seeds


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_optimiser_parity(ctx, dtype):
    """out_loss, improved, fcalls, the constants left in the program and starts_out against the loop of
    one-tree optimize_constants(expr, idx=set, seed=seed_t); under log(p - t) many objective values are NaN."""
    opts, trees, ds, sets, seeds = _optim_problem(ctx, dtype)
    kw = dict(iterations=8, nrestarts=2)
    for name, loss in (("lp", R.lp_expr()), ("log", srhip.ExprLoss(X.N("log", X.diff()), X.options()))):
        want = R.loop_optim(ctx, trees, dtype, ds, loss, sets, seeds, opts, **kw)
        prog = program(ctx, trees, dtype, opts)
        got = R.rowsets_optim(prog, ds, loss, sets, seeds, **kw)
        prog.close()
        assert ctx.rowsets_fallback_trees() == 0
        diff = [t for t in want if want[t] != got[t]]
        assert not diff, (name, diff[:5], [(want[t], got[t]) for t in diff[:2]])
        if name == "lp":
            assert any(v[1] for v in got.values())  # the optimiser moved something
        else:
            assert any(np.isnan(np.uint64(v[0]).view(np.float64)) for v in got.values())


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_optimiser_equals_builtin_l2(ctx, dtype):
    """square(p - t): the objective has the built-in L2's bits, so constants, improved, fcalls and starts are
    srhip_optimize_constants_rowsets' under L2DistLoss (out_loss comes from two evaluators)."""
    opts, trees, ds, sets, seeds = _optim_problem(ctx, dtype)
    kw = dict(iterations=8, nrestarts=2)
    pa, pb = program(ctx, trees, dtype, opts), program(ctx, trees, dtype, opts)
    a = R.rowsets_optim(pa, ds, G.l2_expr(), sets, seeds, **kw)
    b = R.rowsets_optim(pb, ds, srhip.L2DistLoss(), sets, seeds, **kw)
    pa.close()
    pb.close()
    # trees whose acceptance does not sit between the two evaluators' baselines (the margin of
    # test_optimiser_equals_builtin_l2_bit_for_bit): all of them here, or the comparison says which
    diff = [t for t in a if a[t][1:] != b[t][1:]]
    assert not diff, (diff, [(a[t], b[t]) for t in diff[:2]])


# ---- 8. more chunks than one round of waves ---------------------------------------------------------------------
def test_many_small_sets(ctx):
    dtype = np.float32
    ds, _, _, _ = _dataset(ctx, dtype, False)
    opts = G.tree_options()
    trees = srhip.random_population(1500, opts, 3, dtype, seed=5, max_size=12)
    rng = np.random.default_rng(9)
    sets = R.draw_sets(rng, N, [3] * 1500)
    sample = sorted(int(t) for t in rng.choice(1500, size=64, replace=False))
    loss = R.lp_expr()
    prog = program(ctx, trees, dtype)
    got = R.rowsets_loss(prog, ds, loss, sets, sample)
    assert ctx.rowsets_fallback_trees() == 0
    gotg = R.rowsets_grad(prog, ds, loss, sets, sample)
    assert ctx.rowsets_fallback_trees() == 0
    prog.close()
    assert got == R.loop_loss(ctx, trees, dtype, ds, loss, sets, sample)
    assert gotg == R.loop_grad(ctx, trees, dtype, ds, loss, sets, sample)


# ---- 9. validation ----------------------------------------------------------------------------------------------
def _raw(ctx, ds, prog, loss, dtype, which, offsets, rows, null=False):
    lib = _lib.load()
    nt = prog.ntrees
    out, ok = np.empty(nt), np.empty(nt, np.uint8)
    grad = np.empty(max(1, int(prog.num_constants().sum())))
    off = None if offsets is None else np.ascontiguousarray(offsets, dtype=np.int64)
    rw = None if rows is None else np.ascontiguousarray(rows, dtype=np.int64)
    h = loss.handle(dtype)
    if which == "score":
        rc = lib.srhip_eval_loss_expr_rowsets(ctx.handle, ds.handle, prog.handle, h, _lib.ptr(off), _lib.ptr(rw),
                                              None if null else _lib.ptr(out), _lib.ptr(ok))
    elif which == "grad":
        rc = lib.srhip_eval_loss_grad_expr_rowsets(ctx.handle, ds.handle, prog.handle, h, _lib.ptr(off), _lib.ptr(rw),
                                                   _lib.ptr(out), None if null else _lib.ptr(grad), _lib.ptr(ok))
    else:
        opt = _lib.OptimOptions(2, 1, 0, 1e-8)
        imp, fc = np.empty(nt, np.uint8), np.empty(nt, np.int64)
        rc = lib.srhip_optimize_constants_expr_rowsets(ctx.handle, ds.handle, prog.handle, h, _lib.ptr(off), _lib.ptr(rw),
                                                       ctypes.byref(opt), None, None, None,
                                                       None if null else _lib.ptr(out), _lib.ptr(imp), _lib.ptr(fc))
    return rc, lib.srhip_last_error().decode() if rc else ""


@pytest.mark.parametrize("which", ["score", "grad", "optim"])
def test_validation(ctx, which):
    m = 300
    rng = np.random.default_rng(3)
    Xd = rng.standard_normal((2, m)).astype(np.float32)
    y, w = rng.standard_normal(m).astype(np.float32), rng.uniform(1, 2, m).astype(np.float32)
    ds, dsw = srhip.DeviceDataset(ctx, Xd, y), srhip.DeviceDataset(ctx, Xd, y, w)
    prog = program(ctx, [x(1) * 1.5 + x(2), x(1) * x(2) + 0.5], np.float32)
    before = np.concatenate(prog.get_constants())
    l2, l3 = G.l2_expr(False), G.l2_expr(True)
    f32 = np.float32
    good_off, good_rows = [0, 3, 5], [0, 1, 2, 3, 299]
    # row-set errors, naming tree and position
    rc, msg = _raw(ctx, ds, prog, l2, f32, which, [0, 3, 3], [0, 1, 2])
    assert rc == _lib.ERR_INVALID and "tree 1 has an empty row set" in msg
    rc, msg = _raw(ctx, ds, prog, l2, f32, which, [0, 3, 2], [0, 1, 2])
    assert rc == _lib.ERR_INVALID and "row_offsets[2] = 2 < row_offsets[1] = 3" in msg
    rc, msg = _raw(ctx, ds, prog, l2, f32, which, [1, 3, 5], good_rows)
    assert rc == _lib.ERR_INVALID and "row_offsets[0] must be 0" in msg
    rc, msg = _raw(ctx, ds, prog, l2, f32, which, good_off, [0, 1, 2, 3, 300])
    assert rc == _lib.ERR_INVALID and "tree 1" in msg and "position 1 of its set" in msg and "out of range [0, 300)" in msg
    rc, msg = _raw(ctx, ds, prog, l2, f32, which, good_off, [0, -1, 2, 3, 4])
    assert rc == _lib.ERR_INVALID and "tree 0" in msg and "position 1 of its set" in msg
    rc, msg = _raw(ctx, ds, prog, l2, f32, which, None, good_rows)
    assert rc == _lib.ERR_INVALID and "null" in msg
    rc, msg = _raw(ctx, ds, prog, l2, f32, which, good_off, None)
    assert rc == _lib.ERR_INVALID and "null" in msg
    rc, msg = _raw(ctx, ds, prog, l2, f32, which, good_off, good_rows, null=True)
    assert rc == _lib.ERR_INVALID and "null" in msg
    # expression errors
    rc, msg = _raw(ctx, ds, prog, l3, f32, which, good_off, good_rows)
    assert rc == _lib.ERR_INVALID and "nargs = 2" in msg
    rc, msg = _raw(ctx, dsw, prog, l2, f32, which, good_off, good_rows)
    assert rc == _lib.ERR_INVALID and "nargs = 3" in msg
    rc, msg = _raw(ctx, ds, prog, l2, np.float64, which, good_off, good_rows)
    assert rc == _lib.ERR_INVALID and "dtype" in msg
    iopts = srhip.Options(binary_operators=("+", "*"), unary_operators=())
    Xi = rng.integers(-5, 6, size=(2, m)).astype(np.int32)
    dsi = srhip.DeviceDataset(ctx, Xi, Xi[0])
    progi = program(ctx, [x(1) + x(2), x(1) * x(2)], np.int32, iopts)
    rc, msg = _raw(ctx, dsi, progi, l2, f32, which, good_off, good_rows)
    assert rc == _lib.ERR_UNSUPPORTED and "Int32" in msg
    # a failed call leaves the constants' bits unchanged, and the context still works
    assert np.array_equal(bits(np.concatenate(prog.get_constants())), bits(before))
    rc, msg = _raw(ctx, ds, prog, l2, f32, which, good_off, good_rows)
    assert rc == 0, msg
    sets = [np.array(good_rows[:3]), np.array(good_rows[3:])]
    fresh = program(ctx, [x(1) * 1.5 + x(2), x(1) * x(2) + 0.5], np.float32)
    assert R.rowsets_loss(fresh, ds, l2, sets) == R.loop_loss(ctx, [x(1) * 1.5 + x(2), x(1) * x(2) + 0.5], f32, ds, l2, sets)
    fresh.close()
    prog.close()
    progi.close()


# ---- 10. the mirror ---------------------------------------------------------------------------------------------
def _count(monkeypatch, name, calls):
    orig = getattr(srhip.Program, name)
    monkeypatch.setattr(srhip.Program, name, lambda self, *a, **k: (calls.append((name, self.ntrees)), orig(self, *a, **k))[1])


def test_mirror_makes_one_call_with_the_loops_bits(ctx, monkeypatch):
    rng = np.random.default_rng(2)
    Xd = rng.standard_normal((2, 400))
    y = 2.0 * Xd[0] + 1.0
    dataset = srhip.Dataset(Xd, y)
    opts = srhip.Options(elementwise_loss=R.lp_expr(), **G.TREE_OPS)
    api.update_baseline_loss(dataset, opts)
    build = lambda: [x(1) * 1.2 + 0.3, x(1) * 0.7, x(1) * -0.5 + 3.0, G.row_failing() + 0.5]
    idxs = R.draw_sets(rng, 400, [50, 50, 7, 50])
    # the loops first (the single-idx calls), then the one call of each mirror function
    want_l = [api.eval_loss_batch([t], dataset, opts, idx=i) for t, i in zip(build(), idxs)]
    want_g = [api.eval_grad_loss_batch([t], dataset, opts, idx=i) for t, i in zip(build(), idxs)]
    loop_members = [G.Member(t) for t in build()]
    r1, loop_evals = np.random.default_rng(0), 0.0
    for mb, i in zip(loop_members, idxs):
        _, ev = api.optimize_constants(dataset, mb, opts, rng=r1, idx=i)
        loop_evals += ev
    calls = []
    for name in ("eval_loss_rowsets", "eval_loss_grad_rowsets", "optimize_constants_rowsets", "eval_loss", "eval_loss_grad",
                 "optimize_constants"):
        _count(monkeypatch, name, calls)
    l, ok = api.eval_loss_rowsets_batch(build(), dataset, opts, idxs)
    assert calls == [("eval_loss_rowsets", 4)]
    assert np.array_equal(bits(l), bits([float(p[0][0]) for p in want_l])) and ok.tolist() == [bool(p[1][0]) for p in want_l]
    assert ok.tolist() == [True, True, True, False]
    del calls[:]
    gl, gg, gok = api.eval_grad_loss_batch(build(), dataset, opts, idxs=idxs)
    assert calls == [("eval_loss_grad_rowsets", 4)]
    assert G.same_bits((gl, gg, gok), (np.array([p[0][0] for p in want_g]), [p[1][0] for p in want_g],
                                       np.array([p[2][0] for p in want_g])))
    del calls[:]
    members = [G.Member(t) for t in build()]
    r2 = np.random.default_rng(0)
    _, evals = api.optimize_constants(dataset, members, opts, rng=r2, idxs=idxs)
    assert calls == [("optimize_constants_rowsets", 4)]
    assert evals == loop_evals and r1.integers(0, 2**62) == r2.integers(0, 2**62)  # the generator consumed alike
    for a, b in zip(members, loop_members):
        assert np.array_equal(bits(srhip.get_constants(a.tree)), bits(srhip.get_constants(b.tree)))
        assert bits(a.loss)[0] == bits(b.loss)[0] and (a.birth == -1) == (b.birth == -1)
    assert members[0].birth != -1
