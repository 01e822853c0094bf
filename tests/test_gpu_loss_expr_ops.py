"""Loss expressions on the device against exact math: every operator at every value slot the loss compiler can
reach, in both operand orders (the forms of tests/loss_expr_ops_common.py; tests/test_loss_expr_ops_table.py
shows without a device that they compile to those slots and that the host interpreter meets the same bars).

(a) rowsets_lossx_kernel, per row: one leaf tree `x1` per table row with the singleton row set {i} on an
    unweighted dataset, so out_loss[i] is l(p_i, t_i) converted to double and added to +0.0, nothing else; against
    tests/golden/forward_values.npz under the table's class bars (forward_values_common.failing_rows), and the
    host interpreter's bits for the exact and rounded-once classes.
(b) grad_rowsets_lossx_kernel, per row: one-constant trees `x1 + 0.5` over the feature x - 0.5 (prediction =
    the tabulated x exactly, d pred / d c = 1 exactly), so the gradient slice is dl/dp in T; against
    tests/golden/derivative_rules.npz under derivative_rules_common's bars (128 eps(T) relative; bit-exact for
    partials that are exactly 0 or +-1 and for `*`'s).
(c) row positions: multi-row sets (the points tiled cyclically) through lossx_kernel, eval_lossx_kernel,
    rowsets_lossx_kernel, grad_lossx_kernel and grad_rowsets_lossx_kernel: the same bits from every entry
    point, and the mean within the derived bound m 2^-52 sum|l| / m (tests/test_gpu_loss_expr.py
    test_derived_bound) of the exact mean of the per-row device values of (a) / (b).

A leaf tree over a non-finite feature row fails its column check (csrc/srhip_decide.cpp column_fails: did_succeed
is false, the loss +Inf), so on the device a non-finite operand travels in y: op(t) for a unary operator,
`t op p` / `p op t` for a binary one with the finite operand as the prediction.  What is left out is asserted:
no point of a unary operator, and of a binary operator exactly the special points whose two operands are both
non-finite (the host interpreter is held to those).  Every dataset holds one feature column and y, which keeps
every row set below the row-set kernels' cap; srhip_rowsets_fallback_trees is 0 after every row-set call.

One thing a mean cannot carry: the sum over a row set starts from +0.0 in double, and +0.0 + -0.0 is +0.0, so a
loss of -0.0 (neg(+0.0), -0.0 * x, ...) comes back as +0.0 from every entry point.  The device comparisons
therefore take a zero of either sign for a tabulated zero (`+ T(0)` on both sides; nothing else changes under
it); the sign of a zero result is held by the host interpreter's test, bit for bit.
"""
import math

import numpy as np
import pytest

import srhip

import derivative_rules_common as dr
import forward_values_common as fv
import loss_expr_grad_common as G
import loss_expr_ops_common as ops
import loss_expr_rowsets_common as R

pytestmark = pytest.mark.gpu

DTS = ("f32", "f64")
_CACHE = {}
_TREE_OPTS = dict(binary_operators=("+", "*"), unary_operators=())


def _x1():
    return srhip.Node(feature=1)


def _program(ctx, dt, n, kind):
    """n copies of the leaf x1 ("leaf"), of x1 + 0.5 ("shift") or of x1 + (-0.0) ("zero": the prediction is x1
    for every value, -0.0 included), made once."""
    key = ("prog", dt, n, kind)
    if key not in _CACHE:
        make = {"leaf": _x1, "shift": ops.shifted_tree, "zero": lambda: ops.N("+", _x1(), ops.C(-0.0))}[kind]
        opts = srhip.Options(**_TREE_OPTS)
        nodes, offs = srhip.flatten([make() for _ in range(n)], opts, fv.NP[dt])
        _CACHE[key] = srhip.Program(ctx, nodes, offs, opts, fv.NP[dt])
    return _CACHE[key]


def _singletons(n):
    if ("sets", n) not in _CACHE:
        _CACHE["sets", n] = [np.array([i]) for i in range(n)]
    return _CACHE["sets", n]


def _same(a, b):
    return np.array_equal(G.bits(a), G.bits(b))


def _as_T(loss, T):
    """A per-row loss is a T value converted to double: back in T without a rounding."""
    got = loss.astype(T)
    back = got.astype(np.float64)
    assert np.array_equal(np.isnan(back), np.isnan(loss)) and np.array_equal(back[~np.isnan(loss)], loss[~np.isnan(loss)])
    return got


def _agree(got, host):
    return fv.bits_equal(np.ascontiguousarray(got), np.ascontiguousarray(host)) | (np.isnan(got) & np.isnan(host))


# ---- (a) per-row values -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("op", ops.UN_OPS + ops.BIN_OPS)
def test_per_row_values(ctx, op, dt):
    """Every device form of one operator (bases 0 .. 5 / 0 .. 4, swapped order at bases 0 .. 3, constant
    operands) on the general points and the special block, one srhip_eval_loss_expr_rowsets call per form."""
    T = fv.NP[dt]
    cls = fv.op_class(op, dt)
    bad, worst = [], 0.0
    for which in ("general", "special"):
        datasets = {}
        a, b, _, mask0 = ops.operands("un" if op in ops.UN_OPS else "bin", op, dt, which)
        covered = np.zeros(len(a), bool)
        for form in (f for f in ops.forms(dt) if f["op"] == op and not f["w"]):
            pred, y, _, want, mask = ops.columns(form, dt, which)
            if not mask.any():
                continue
            n = len(pred)
            fin = np.isfinite(pred)
            prog = _program(ctx, dt, n, "leaf")
            if (form["p"], form["t"]) not in datasets:
                ds = datasets[form["p"], form["t"]] = srhip.DeviceDataset(ctx, pred[None, :], y)
                # the leaf returns the table's inputs bit for bit and succeeds on every finite row.  The special
                # block goes row by row: a view fails as a whole when it holds a non-finite row or when its
                # column sum overflows (the largest value twice); the row-set call below fails exactly the
                # non-finite rows
                one = _program(ctx, dt, 1, "leaf")
                views = [None] if which == "general" else [np.array([i]) for i in np.nonzero(fin)[0]]
                for view in views:
                    out, pok = one.eval_predict(ds, idx=view)
                    assert pok.all() and fv.bits_equal(out[0], pred if view is None else pred[view]).all(), (form["label"], view)
            ds = datasets[form["p"], form["t"]]
            loss, ok = prog.eval_loss_rowsets(ds, ops.expr(form), _singletons(n))
            assert ctx.rowsets_fallback_trees() == 0, form["label"]
            assert np.array_equal(ok, fin) and np.all(np.isposinf(loss[~fin])), form["label"]
            got = _as_T(loss, T) + T(0)  # (the mean starts from +0.0: a zero comes back positive, see above)
            want = want + T(0)
            count = mask & fin
            rows = fv.failing_rows(op, dt, got, want, count)
            bad += [(form["label"], which, int(r), float(pred[r]), float(y[r]), float(got[r]), float(want[r])) for r in rows[:3]]
            if cls in ("exact", "rounded"):
                host = ops.host_values(form, pred, y) + T(0)
                off = np.nonzero(count & ~_agree(got, host))[0]
                bad += [(form["label"], which, "host", int(r), float(got[r]), float(host[r])) for r in off[:3]]
            worst = max(worst, ops.worst_ulp(got, want, count))
            if form["row"] is None:
                covered |= count
        left = mask0 & ~covered
        if b is None:
            assert not left.any()
        else:
            assert np.array_equal(left, mask0 & ~np.isfinite(a) & ~np.isfinite(b))
            assert which == "special" or not left.any()
    print(f"LOSSX_ERR device value {op} {dt} {worst:.0f} ulp")
    assert not bad, (len(bad), bad[:10])


# ---- (b) per-row derivatives ------------------------------------------------------------------------------------
def _grad_rows(ctx, dt, form, kind="shift"):
    """(loss [n], dl/dp [n], dataset) of one derivative form, per row: singleton sets over n one-constant trees
    whose prediction is the form's p column exactly."""
    T = fv.NP[dt]
    p, t = form["p"], form["t"]
    n = len(p)
    prog = _program(ctx, dt, n, kind)
    feat = p - T(0.5) if kind == "shift" else p
    ds = srhip.DeviceDataset(ctx, feat[None, :], t)
    pred, ok = _program(ctx, dt, 1, kind).eval_predict(ds)
    assert ok.all() and fv.bits_equal(pred[0], p).all(), form["label"]
    loss, g, ok = prog.eval_loss_grad_rowsets(ds, ops.expr(form), _singletons(n))
    assert ctx.rowsets_fallback_trees() == 0 and ok.all(), form["label"]
    dl = np.array([gi[0] for gi in g])
    assert all(gi.shape == (1,) for gi in g)
    # the same loss bits as the scoring kernel's on the same rows
    l2, ok2 = prog.eval_loss_rowsets(ds, ops.expr(form), _singletons(n))
    assert ctx.rowsets_fallback_trees() == 0 and ok2.all() and _same(loss, l2), form["label"]
    return loss, dl, ds


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("name", dr.UN_OPS + dr.BIN_CASES)
def test_per_row_derivatives(ctx, name, dt):
    """dl/dp of every form of one rule against the table: op(p) at bases 0 .. 5; p op t (d/da) and t op p
    (d/db) at bases 0 .. 4 and in swapped order at bases 0 .. 3.  The loss of the gradient call has the bits of
    the scoring call, and for an exact-class operator the host interpreter's."""
    T = fv.NP[dt]
    worst = 0.0
    for form in (f for f in ops.grad_forms(dt) if f["name"] == name):
        loss, dl, _ = _grad_rows(ctx, dt, form)
        assert np.isfinite(loss).all() and np.isfinite(dl).all(), form["label"]
        _as_T(dl, T)
        err = float(np.max(dr.rel_err(dl, form["want"]))) / dr.EPS[dt]
        assert err <= (0 if form["exact"] else dr.BAR), (form["label"], err)
        worst = max(worst, err)
        if fv.op_class(form["op"], dt) == "exact":
            assert _agree(_as_T(loss, T) + T(0), ops.expr(form)(form["p"], form["t"]) + T(0)).all(), form["label"]
    print(f"LOSSX_ERR device rule {name} {dt} {worst:.2f} eps")


@pytest.mark.parametrize("dt", DTS)
def test_gamma_has_a_value_and_no_tangent(ctx, dt):
    """gamma(p) at every base: dl/dp is NaN, the value stays the table's and did_succeed stays true (the
    expression's outputs take no part in the decision)."""
    T = fv.NP[dt]
    x, _, want, mask = ops.operands("un", "gamma", dt, "general")
    for form in (f for f in ops.forms(dt) if f["op"] == "gamma" and f["order"] == "nat" and f["p"] == "a"):
        gf = dict(label=form["label"], tree=form["tree"], nargs=2, p=x, t=np.zeros_like(x))
        loss, dl, _ = _grad_rows(ctx, dt, gf, kind="zero")
        assert np.isnan(dl).all(), form["label"]
        assert not len(fv.failing_rows("gamma", dt, _as_T(loss, T), want, mask)), form["label"]


@pytest.mark.parametrize("dt", DTS)
def test_derivative_conventions(ctx, dt):
    """DESIGN.md 4 "Derivative conventions" inside a loss expression: abs'(0) = relu'(0) = 0 at both zeros; a
    tie of max / min gives the second operand; cond has no first partial and its second is 0 where a <= 0;
    a ^ b at a <= 0 has d/da = b a^(b - 1) and d/db = 0."""
    T = fv.NP[dt]
    N, P, T_ = ops.N, ops.P, ops.T_
    z4 = [0.0, -0.0, 1.0, -1.0]
    tie = [1.0, -2.0, 0.0, 0.5]
    cases = [
        ("abs", N("abs", P()), z4, [0.0] * 4, [0.0, 0.0, 1.0, -1.0]),
        ("relu", N("relu", P()), z4, [0.0] * 4, [0.0, 0.0, 1.0, 0.0]),
        ("max(p, t)", N("max", P(), T_()), tie, tie, [0.0] * 4),
        ("max(t, p)", N("max", T_(), P()), tie, tie, [1.0] * 4),
        ("min(p, t)", N("min", P(), T_()), tie, tie, [0.0] * 4),
        ("min(t, p)", N("min", T_(), P()), tie, tie, [1.0] * 4),
        ("cond(p, t)", N("cond", P(), T_()), [0.0, -0.0, 2.0, -2.0], [3.0] * 4, [0.0] * 4),
        ("cond(t, p)", N("cond", T_(), P()), [3.0] * 4, [0.0, -0.0, 2.0, -2.0], [0.0, 0.0, 1.0, 0.0]),
        ("p ^ t", N("^", P(), T_()), [0.0, -1.5, -2.0, 2.0], [2.0, 2.0, 3.0, 2.0], [0.0, -3.0, 12.0, 4.0]),
        ("t ^ p", N("^", T_(), P()), [2.0, 2.0, 3.0, 2.0], [0.0, -1.5, -2.0, -2.0], [0.0] * 4),  # (the base is t)
    ]
    for label, tree, p, t, want in cases:
        for k in (0, 3):
            form = dict(label=f"{label}@{k}", tree=ops.at_base(tree, k), nargs=2, p=np.array(p, T), t=np.array(t, T))
            _, dl, _ = _grad_rows(ctx, dt, form, kind="zero")
            assert np.array_equal(dl, want), (form["label"], dl)


# ---- (c) row positions and the whole-dataset kernels ----------------------------------------------------------
def _population(ctx, dt, first):
    """[first, x1 * x1, x1 + x1, first]: the tree under test at positions 0 and last."""
    key = ("pop", dt, first)
    if key not in _CACHE:
        make = _x1 if first == "leaf" else ops.shifted_tree
        opts = srhip.Options(**_TREE_OPTS)
        trees = [make(), ops.N("*", _x1(), _x1()), ops.N("+", _x1(), ops.N("*", _x1(), ops.C(0.75))), make()]
        nodes, offs = srhip.flatten(trees, opts, fv.NP[dt])
        _CACHE[key] = srhip.Program(ctx, nodes, offs, opts, fv.NP[dt])
    return _CACHE[key]


def _within_derived_bound(got, rows, what):
    """|got - fsum(l) / m| <= m 2^-52 fsum|l| / m for finite rows; the same non-finite value otherwise."""
    m = len(rows)
    if not np.isfinite(rows).all():
        exact = np.sum(rows)  # NaN, or the one infinity (both signs: NaN)
        assert (np.isnan(got) and np.isnan(exact)) or got == exact, (what, got, exact)
        return
    err = abs(got - math.fsum(rows) / m)
    bar = m * 2.0 ** -52 * math.fsum(np.abs(rows)) / m
    assert err <= bar, (what, m, got, err, bar)


def _big(dt, cap):
    tile = 64 * (8 if dt == "f32" else 4)
    return ops.POSITION_SIZES[2] if ops.POSITION_SIZES[2] <= cap else cap - tile + 65


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("kind", ["un", "bin"])
def test_row_positions_scoring(ctx, kind, dt):
    """The general points tiled cyclically to 50, 257 and 4096 + 65 rows (Float64: the last ragged tile under
    its 2560-row cap), so that every point visits every register row, lane and pass: the same bits from
    srhip_eval_loss_expr_rowsets, srhip_eval_loss_expr(idx) and srhip_eval_loss_expr_fused(idx), for one tree and
    for the tree at positions 0 and last of a population of 4; the mean within the derived bound of the exact
    mean of the per-row device values.  Prints, for Float32, how many rows per form lie under the bound's
    resolution of one ulp (0 for the exact-class operators: tests/test_loss_expr_ops_table.py)."""
    T = fv.NP[dt]
    cap = R.score_cap(T, 1, False)
    sizes = ops.POSITION_SIZES[:2] + (_big(dt, cap),)
    assert max(sizes) <= cap and (dt == "f64" or sizes[2] == 4096 + 65)
    one, pop = _program(ctx, dt, 1, "leaf"), _population(ctx, dt, "leaf")
    other = [np.arange(7), np.arange(100)]
    for form in (f for f in ops.position_forms(dt) if f["kind"] == kind):
        loss = ops.expr(form)
        pred, y, _, _, _ = ops.columns(form, dt, "general")
        rows, ok = _program(ctx, dt, fv.P, "leaf").eval_loss_rowsets(srhip.DeviceDataset(ctx, pred[None, :], y), loss,
                                                                      _singletons(fv.P))
        assert ok.all() and ctx.rowsets_fallback_trees() == 0
        pts = ops.position_points(form["op"], kind, dt)
        idx = pts[np.arange(max(sizes)) % len(pts)]
        ds = srhip.DeviceDataset(ctx, pred[idx][None, :], y[idx])
        for m in sizes:
            s = np.arange(m)
            a, oka = one.eval_loss_rowsets(ds, loss, [s])
            assert ctx.rowsets_fallback_trees() == 0 and oka.all()
            for name, (b, okb) in (("idx", one.eval_loss(ds, loss, idx=s)), ("fused", one.eval_loss_fused(ds, loss, idx=s))):
                assert okb.all() and _same(a, b), (form["label"], m, name, a, b)
            pa, _ = pop.eval_loss_rowsets(ds, loss, [s] + other + [s])
            assert ctx.rowsets_fallback_trees() == 0
            pb, _ = pop.eval_loss(ds, loss, idx=s)
            pc, _ = pop.eval_loss_fused(ds, loss, idx=s)
            for name, v in (("rowsets", pa), ("idx", pb), ("fused", pc)):
                assert _same(v[[0, 3]], np.repeat(a, 2)), (form["label"], m, "population", name)
            _within_derived_bound(a[0], rows[idx[:m]], (form["label"], dt))
            if dt == "f32":
                print(f"LOSSX_SMALL {form['label']} m={m} rows under one ulp: {ops.small_rows(rows[idx[:m]], m)}")


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("kind", ["un", "bin"])
def test_row_positions_gradient(ctx, kind, dt):
    """The 300 derivative points tiled cyclically to 50, 257 and the gradient row-set cap (computed: 5120 /
    2560 rows): the same bits from srhip_eval_loss_grad_expr_rowsets and srhip_eval_loss_grad_expr(idx), for one
    tree and at positions 0 and last of a population; loss and gradient within the derived bound of the exact
    means of the per-row device values of (b)."""
    T = fv.NP[dt]
    cap = R.grad_cap(T, 1, False)
    assert cap == min(R.score_cap(T, 1, False), 64 * R.GRAD_RB) and cap % R.GRAD_RB == 0
    sizes = (50, 257, cap)
    one, pop = _program(ctx, dt, 1, "shift"), _population(ctx, dt, "shift")
    other = [np.arange(7), np.arange(100)]
    unary = set(dr.UN_OPS)
    for form in (f for f in ops.position_grad_forms(dt) if (f["name"] in unary) == (kind == "un")):
        loss = ops.expr(form)
        lrow, dlrow, _ = _grad_rows(ctx, dt, form)
        idx = np.arange(cap) % len(lrow)
        ds = srhip.DeviceDataset(ctx, (form["p"][idx] - T(0.5))[None, :], form["t"][idx])
        for m in sizes:
            s = np.arange(m)
            r = one.eval_loss_grad_rowsets(ds, loss, [s])
            assert ctx.rowsets_fallback_trees() == 0 and r[2].all()
            assert G.same_bits(r, one.eval_loss_grad(ds, loss, idx=s)), (form["label"], m)
            pr = pop.eval_loss_grad_rowsets(ds, loss, [s] + other + [s])
            assert ctx.rowsets_fallback_trees() == 0
            pi = pop.eval_loss_grad(ds, loss, idx=s)
            for name, v in (("rowsets", pr), ("idx", pi)):
                for t in (0, 3):
                    assert G.same_bits((v[0][t:t + 1], [v[1][t]], v[2][t:t + 1]), r), (form["label"], m, "population", name, t)
            _within_derived_bound(r[0][0], lrow[idx[:m]], (form["label"], dt, "loss"))
            _within_derived_bound(r[1][0][0], dlrow[idx[:m]], (form["label"], dt, "gradient"))
