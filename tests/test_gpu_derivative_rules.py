"""Every derivative rule of the dual-number kernel (csrc/srhip_grad_impl.h: 33 unary operators, 13 binary
operators, 9 distance and 11 margin losses) against exact math: tests/golden/derivative_rules.npz, computed
by mpmath at 40 digits at the exact stored inputs (tests/golden/make_derivative_rules.py).

300 rows (a 256-row block and a 44-row tail that is no multiple of 64), 3 features, Float32 and Float64.
Smooth rules: within 128 eps(T) of the table, relative -- the formulas themselves stay within 16 eps on the
table's domains (tests/test_oracle_grad_rules.py), which leaves a vendor function a few ulps off (amplified
by the same conditioning, at most about 27: tanh at 2) inside the bar, and a wrong rule, a swapped partial
or a single-precision constant in the Float64 path (1e-8 or more) far outside.  Partials that are exactly 0
or +-1 are bit-exact.  The measured worst errors are tabulated in DESIGN.md ("Derivative rules").
"""
import numpy as np
import pytest

import derivative_rules_common as C

pytestmark = pytest.mark.gpu

DTS = ["f32", "f64"]


def _sr():
    import srhip

    return srhip


def _report(kind, name, dt, err_eps):
    print(f"RULE_ERR {kind} {name} {dt} {err_eps:.2f}")


def _check(got, want, exact, dt, what):
    """Worst relative error in eps(T); asserts the bar (bit-exact rules: 0)."""
    err = float(np.max(C.rel_err(got, want))) / C.EPS[dt]
    assert err <= (0 if exact else C.BAR), (what, dt, err)
    return err


def _grad_predict(prog, ds, variable):
    """eval_grad_predict, with its predictions and did_succeed held to eval_predict's (what eval_tree_array
    returns).  The library fills them by running the evaluator itself, so this pins the contract of the
    call, not a second computation."""
    pred, grads, ok = prog.eval_grad_predict(ds, variable=variable)
    ev, eok = prog.eval_predict(ds)
    assert np.array_equal(ok, eok)
    assert np.array_equal(pred.view(np.uint8), ev.view(np.uint8)), "predictions are the evaluator's, bit for bit"
    return pred, grads, ok


# ---- unary rules, per row ---------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("op", C.UN_OPS)
def test_unary_rule(ctx, op, dt):
    """U(x1), U(2 * x2) and U(x1) * 2 by feature; U(2 * x2), the constant-subtree form U(c) * x1 and
    U(x1) * c by constant."""
    sr = _sr()
    T = C.NP[dt]
    X, df = C.unary_inputs(op, dt)
    x64 = X[0].astype(np.float64)
    opts = sr.Options(binary_operators=("*",), unary_operators=(op,))
    trees = C.unary_trees(sr, op, X[0])
    nodes, offs = sr.flatten(trees, opts, T)
    prog = sr.Program(ctx, nodes, offs, opts, T)
    ds = sr.DeviceDataset(ctx, X)
    exact = op in C.EXACT_UN
    worst = 0.0
    pred, g, ok = _grad_predict(prog, ds, True)
    assert ok.all() and all(gi.dtype == T and gi.shape == (3, 300) for gi in g)
    worst = max(worst, _check(g[0][0], df, exact, dt, "U(x1) by x1"))
    worst = max(worst, _check(g[4][0], 2.0 * df, exact, dt, "U(x1) 2 by x1"))
    worst = max(worst, _check(g[1][1], 2.0 * df, exact, dt, "U(2 x2) by x2"))  # a power of two: same relative error
    for t, f in ((0, 1), (0, 2), (1, 0), (1, 2), (2, 1), (2, 2), (3, 1), (3, 2), (4, 1), (4, 2)):
        assert not g[t][f].any(), ("an absent feature has derivative exactly 0", t, f)
    _, g, ok = _grad_predict(prog, ds, False)
    assert ok.all() and [gi.shape[0] for gi in g] == [0, 1, 1, 1, 1]
    assert np.array_equal(g[4][0], pred[0]), "d (U(x1) c) / d c = U(x1), exactly"
    worst = max(worst, _check(g[1][0], (x64 / 2) * df, exact, dt, "U(c x2) by c"))
    for t, j in ((2, 0), (3, -1)):  # d (U(c) x1) / d c = U'(c) x1; the product rounds once more
        worst = max(worst, _check(g[t][0], df[j] * x64, exact, dt, "U(c) x1 by c"))
    _report("unary", op, dt, worst)


# ---- binary rules, every operand form ---------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("case", C.BIN_CASES)
def test_binary_rule_every_operand_form(ctx, case, dt):
    """A op X, X op A, A op c, c op A, S[k] op A (k = 0 .. 3) and A op S[0], the leaf-leaf forms and the
    constant-subtree form B(c1, c2) * x1 (csrc/srhip_grad_tile.inc), by feature and by constant: a form that
    swapped or dropped a partial shows in the non-commutative operators, whichever operand it sits on."""
    sr = _sr()
    T = C.NP[dt]
    a, b, fa, fb = C.binary_inputs(case, dt)
    part = {"a": fa, "b": fb}
    forms = C.binary_trees(sr, case, a, b)
    opts = C.binary_options(sr, case)
    exact = case in C.EXACT_BIN or case == "*"
    worst = 0.0
    for d, X in enumerate(C.binary_datasets(a, b)):
        mine = [f for f in forms if f[1] == d]
        nodes, offs = sr.flatten([f[2] for f in mine], opts, T)
        prog = sr.Program(ctx, nodes, offs, opts, T)
        ds = sr.DeviceDataset(ctx, X)
        x1 = X[0].astype(np.float64)
        _, gv, okv = _grad_predict(prog, ds, True)
        _, gc, okc = _grad_predict(prog, ds, False)
        assert okv.all() and okc.all()
        for t, (form, _, _, row, var, const) in enumerate(mine):
            rows = slice(None) if row is None else slice(row, row + 1)
            if var is not None:
                for f, w in enumerate(var):
                    if w is None:
                        assert not gv[t][f].any(), (form, f)
                    else:
                        worst = max(worst, _check(gv[t][f][rows], part[w][rows], exact, dt, (form, "x", f)))
            assert gc[t].shape == (len(const), 300), form
            for k, w in enumerate(const):
                if w == 1:
                    assert np.array_equal(gc[t][k], np.ones(300, T)), (form, k)
                elif w in ("ax", "bx"):  # the constant subtree's partial at row `row`, times x1 on every row
                    # (exact only where the partial is 0 or +-1: b x1 and floor(a / b) x1 round in T)
                    worst = max(worst, _check(gc[t][k], part[w[0]][row] * x1, case in C.EXACT_BIN and case != "mod", dt,
                                              (form, "c", k)))
                else:
                    worst = max(worst, _check(gc[t][k][rows], part[w][rows], exact, dt, (form, "c", k)))
    _report("binary", case, dt, worst)


# ---- binary rules, the once-per-lane variants -------------------------------------------------------
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("case", C.BIN_CASES)
def test_binary_rule_constant_subtree_forms(ctx, case, dt, monkeypatch):
    """An operator of constant subtrees is evaluated once per lane by hand-written variants of `A op c`,
    `c op A`, `S[0] op A` and `A op S[0]` (csrc/srhip_grad_tile.inc, UN_UNIFORM_FLAG), each with its own
    operand order.  They run only where a lane holds several rows: in constant-gradient launches of
    Float64 programs that need at most 2 stack slots with 4 tangents per chunk (forced here, as these
    trees have up to 6 constants), and in every value-only pass -- never in the per-row launches of
    eval_grad_predict.  So: eval_loss_grad of B(..) * x1 over x1 = 1 under L1 with y far below, where the
    gradient by each constant is the mean of B's partial over 300 equal rows.  Float32 takes the per-row
    variants here and is held to the same table.  The losses and gradients must also be the bits of a
    program compiled with SRHIP_GRAD_UNIFORM=0, value-only passes included."""
    sr = _sr()
    T = C.NP[dt]
    a, b, fa, fb = C.binary_inputs(case, dt)
    part = {"a": fa, "b": fb}
    forms = C.uniform_trees(sr, case, a, b)
    opts = C.binary_options(sr, case)
    nodes, offs = sr.flatten([f[1] for f in forms], opts, T)
    ds = sr.DeviceDataset(ctx, np.ones((3, 300), T), np.full(300, -1e6, T))
    loss = sr.L1DistLoss()
    monkeypatch.setenv("SRHIP_GRAD_KT", "4")
    res = {}
    for uni in ("1", "0"):
        monkeypatch.setenv("SRHIP_GRAD_UNIFORM", uni)
        prog = sr.Program(ctx, nodes, offs, opts, T)
        full = prog.eval_loss_grad(ds, loss)
        monkeypatch.setenv("SRHIP_GRAD_VALUE_ONLY", "1")
        vl, _, vok = prog.eval_loss_grad(ds, loss)
        monkeypatch.delenv("SRHIP_GRAD_VALUE_ONLY")
        res[uni] = (full, (vl, [np.zeros(0)], vok))
        prog.close()
    (l, g, ok), value_only = res["1"]
    assert ok.all()
    assert _same(res["0"][0], res["1"][0]) and _same(res["0"][1], res["1"][1]), "per lane = per row, bit for bit"
    assert np.array_equal(_bits(np.asarray(value_only[0], np.float64)), _bits(np.asarray(l, np.float64)))
    exact = case in C.EXACT_BIN and case != "mod"  # (a partial of 0 or +-1: the mean of 300 equal terms is exact)
    worst = 0.0
    for t, (form, _, row, const) in enumerate(forms):
        assert g[t].shape == (len(const),), form
        for k, w in enumerate(const):
            worst = max(worst, _check(g[t][k:k + 1], part[w[0]][row:row + 1], exact, dt, (form, k)))
    _report("binary_const", case, dt, worst)


# ---- loss derivative rules --------------------------------------------------------------------------
def _loss_problem(kind, dt, weighted):
    """x1 + c1 (c1 = 0.5) with y such that pred - y = d (distance) or y pred = a, y = +-1 (margin), exactly."""
    T = C.NP[dt]
    z = C.table()
    rng = np.random.default_rng(7)
    dl = z[f"loss_dl_{dt}"][C.LOSS_KINDS.index(kind)]
    if kind in C.RULES.DIST:
        d = z[f"loss_d_{dt}"]
        x1 = (rng.integers(-8, 9, 300) / 8).astype(T)
        y = (x1 + T(0.5)) - d
        assert np.array_equal((x1 + T(0.5)) - y, d)
        dpred = dl
    else:
        a = z[f"loss_a_{dt}"]
        y = np.where(rng.random(300) < 0.5, -1, 1).astype(T)
        x1 = a * y - T(0.5)
        assert np.array_equal(y * (x1 + T(0.5)), a)
        dpred = y.astype(np.float64) * dl  # chain rule: d l(y pred) / d pred
    w = rng.uniform(0.5, 2.0, 300).astype(T) if weighted else None
    return np.stack([x1, np.zeros_like(x1), np.zeros_like(x1)]), y, w, dpred


@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("kind", C.LOSS_KINDS)
def test_loss_derivative_rule(ctx, kind, dt, weighted):
    """d loss / d c1 of x1 + c1 = sum(w l') / sum(w).  The kernel sums in Float64, so only the per-term
    error counts: the bar is 128 eps(T) sum|w l'| / sum(w); ZeroOne gives exactly 0."""
    import math

    sr = _sr()
    T = C.NP[dt]
    X, y, w, dpred = _loss_problem(kind, dt, weighted)
    opts = sr.Options(binary_operators=("+",), unary_operators=())
    nodes, offs = sr.flatten([sr.Node("+", sr.Node(feature=1), sr.Node(val=0.5))], opts, T)
    prog = sr.Program(ctx, nodes, offs, opts, T)
    ds = sr.DeviceDataset(ctx, X, y, w)
    _, g, ok = prog.eval_loss_grad(ds, C.loss_object(sr, kind))
    assert ok[0] and g[0].shape == (1,)
    w64 = np.ones(300) if w is None else w.astype(np.float64)
    want = math.fsum(w64 * dpred) / math.fsum(w64)
    scale = math.fsum(np.abs(w64 * dpred)) / math.fsum(w64)
    err = abs(g[0][0] - want)
    if kind == "ZeroOne":
        assert g[0][0] == 0.0
    else:
        assert scale > 0.05
        _report("loss", kind + ("_w" if weighted else ""), dt, err / (scale * C.EPS[dt]))
        assert err <= C.BAR * C.EPS[dt] * scale, (err / (scale * C.EPS[dt]))


# ---- the same bits on every path --------------------------------------------------------------------
def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _same(u, v):
    (l0, g0, k0), (l1, g1, k1) = u, v
    return (np.array_equal(_bits(np.asarray(l0, np.float64)), _bits(np.asarray(l1, np.float64)))
            and np.array_equal(_bits(np.concatenate(g0)), _bits(np.concatenate(g1))) and np.array_equal(k0, k1))


@pytest.mark.parametrize("dt", DTS)
def test_all_operators_same_bits_on_every_path(ctx, dt, monkeypatch):
    """The population of every operator in every form gives the same losses, gradients and did_succeed,
    bit for bit, from the row-subset kernel (subsets of 50 and of 257 rows) and from eval_loss_grad(idx=),
    from the value-only pass and the full pass, with constant subtrees per lane or per row
    (SRHIP_GRAD_UNIFORM) and with or without the derived view (SRHIP_GRAD_DERIVED): the population's
    U(x1) * c trees make every non-inline unary operator of x1 a derived column (24 of the view's 32), which
    tests/test_oracle_grad_rules.py asserts from the node tables."""
    sr = _sr()
    T = C.NP[dt]
    opts, nodes, offs, X, y = C.all_operator_population(sr, dt)
    ntrees = len(offs) - 1
    ds = sr.DeviceDataset(ctx, X, y)
    loss = sr.L2DistLoss()
    monkeypatch.setenv("SRHIP_GRAD_DERIVED_MIN_ROWS", "0")  # the derived view is otherwise off below 8192 rows
    prog = sr.Program(ctx, nodes, offs, opts, T)
    base = prog.eval_loss_grad(ds, loss)
    assert base[2].sum() > ntrees // 2 and not base[2].all()
    # row subsets: four distinct ones per size, tree t on subset t % 4
    rng = np.random.default_rng(13)
    for m in (50, 257):
        sets = [rng.integers(0, 300, m) for _ in range(4)]
        rl, rg, rok = prog.eval_loss_grad_rowsets(ds, loss, [sets[t % 4] for t in range(ntrees)])
        for s in range(4):
            il, ig, iok = prog.eval_loss_grad(ds, loss, idx=sets[s])
            for t in range(s, ntrees, 4):
                assert _same((rl[t:t + 1], [rg[t]], rok[t:t + 1]), (il[t:t + 1], [ig[t]], iok[t:t + 1])), (m, t)
    monkeypatch.setenv("SRHIP_GRAD_VALUE_ONLY", "1")
    vl, _, vok = prog.eval_loss_grad(ds, loss)
    monkeypatch.delenv("SRHIP_GRAD_VALUE_ONLY")
    assert np.array_equal(_bits(np.asarray(vl, np.float64)), _bits(np.asarray(base[0], np.float64)))
    assert np.array_equal(vok, base[2])
    prog.close()
    for var in ("SRHIP_GRAD_UNIFORM", "SRHIP_GRAD_DERIVED"):
        monkeypatch.setenv(var, "0")
        p2 = sr.Program(ctx, nodes, offs, opts, T)
        assert _same(p2.eval_loss_grad(ds, loss), base), var
        monkeypatch.setenv("SRHIP_GRAD_VALUE_ONLY", "1")
        l2, _, ok2 = p2.eval_loss_grad(ds, loss)
        monkeypatch.delenv("SRHIP_GRAD_VALUE_ONLY")
        assert np.array_equal(_bits(np.asarray(l2, np.float64)), _bits(np.asarray(vl, np.float64))), var
        assert np.array_equal(ok2, vok), var
        p2.close()
        monkeypatch.delenv(var)


# ---- composition ------------------------------------------------------------------------------------
def test_composed_rules_match_the_oracle_gradient(ctx, oracle):
    """Chains of rules: the L2 gradient of random trees over all operators against the oracle's exact
    dual-number gradient, within 1e-9 max(1, |g|), for every tree the oracle evaluates as ok.  At least 30
    of the 48 trees and 60 finite components compare (the seed was picked with the oracle alone so that
    they do: 34 and 63, no tree with a non-finite exact gradient)."""
    sr = _sr()
    opts, nodes, offs, X, y = C.composition_problem(sr)
    ref = C.composition_reference(sr, oracle)
    prog = sr.Program(ctx, nodes, offs, opts, np.float64)
    _, g, ok = prog.eval_loss_grad(sr.DeviceDataset(ctx, X, y), sr.L2DistLoss())
    trees = comps = 0
    worst = 0.0
    for t, r in enumerate(ref):
        if r is None:
            continue
        fin = np.isfinite(r)
        if not fin.all():  # an Inf or NaN of the exact gradient must be the device's too (none at this seed)
            assert np.array_equal(np.isnan(g[t]), np.isnan(r)) and np.array_equal(g[t][~fin & ~np.isnan(r)],
                                                                                  r[~fin & ~np.isnan(r)]), t
        else:
            assert ok[t], t
        err = np.abs(g[t][fin] - r[fin]) / np.maximum(1.0, np.abs(r[fin]))
        worst = max(worst, float(err.max(initial=0.0)))
        assert np.all(err <= 1e-9), (t, err.max(initial=0.0))
        trees += 1
        comps += int(fin.sum())
    print(f"RULE_ERR composition trees={trees} components={comps} worst={worst:.3e}")
    assert trees >= 30 and comps >= 60, (trees, comps)


# ---- conventions (DESIGN.md "Derivative conventions") -----------------------------------------------
def _per_row(ctx, dt, binary, unary, tree, X, variable):
    sr = _sr()
    T = C.NP[dt]
    opts = sr.Options(binary_operators=binary, unary_operators=unary)
    nodes, offs = sr.flatten([tree], opts, T)
    prog = sr.Program(ctx, nodes, offs, opts, T)
    _, g, ok = prog.eval_grad_predict(sr.DeviceDataset(ctx, np.asarray(X, T)), variable=variable)
    return g[0], bool(ok[0])


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("op", ["abs", "relu"])
def test_convention_kink_at_zero_has_derivative_zero(ctx, op, dt):
    """abs'(0) = 0, relu'(0) = 0 (at +0 and at -0)."""
    sr = _sr()
    X = np.array([[0.0, -0.0, 1.0, -1.0]] * 3)
    g, ok = _per_row(ctx, dt, ("+",), (op,), sr.Node(op, sr.Node(feature=1)), X, True)
    assert ok and np.array_equal(g[0], [0.0, 0.0, 1.0, -1.0 if op == "abs" else 0.0])


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("op", ["max", "min"])
def test_convention_tie_gives_the_second_operand(ctx, op, dt):
    """max and min at a tie: partials (0, 1), in the leaf-leaf form and in both accumulator forms."""
    sr = _sr()
    N = sr.Node
    X = np.array([[1.0, -2.0, 0.0, 0.5], [1.5, -1.5, 0.5, 1.0], [1.5, -1.5, 0.5, 1.0]])  # x1 + 0.5 = x2 = x3
    for tree, want in ((N(op, N(feature=2), N(feature=3)), ([0] * 4, [0] * 4, [1] * 4)),
                       (N(op, N("+", N(feature=1), N(val=0.5)), N(feature=2)), ([0] * 4, [1] * 4, [0] * 4)),
                       (N(op, N(feature=2), N("+", N(feature=1), N(val=0.5))), ([1] * 4, [0] * 4, [0] * 4))):
        g, ok = _per_row(ctx, dt, ("+", op), (), tree, X, True)
        assert ok and np.array_equal(g, np.array(want, g.dtype)), (tree, g)


@pytest.mark.parametrize("dt", DTS)
def test_convention_cond_at_zero_has_second_partial_zero(ctx, dt):
    sr = _sr()
    X = np.array([[0.0, -0.0, 2.0, -2.0], [3.0, 3.0, 3.0, 3.0], [0.0] * 4])
    g, ok = _per_row(ctx, dt, ("cond",), (), sr.Node("cond", sr.Node(feature=1), sr.Node(feature=2)), X, True)
    assert ok and not g[0].any() and np.array_equal(g[1], [0.0, 0.0, 1.0, 0.0])


@pytest.mark.parametrize("dt", DTS)
def test_convention_pow_of_nonpositive_base_has_no_exponent_partial(ctx, dt):
    """a ^ b with a <= 0 (b an integer, or the value is NaN): d/db = 0; d/da = b a^(b - 1) as everywhere."""
    sr = _sr()
    X = np.array([[0.0, -1.5, -2.0, 2.0], [2.0, 2.0, 3.0, 2.0], [0.0] * 4])
    g, ok = _per_row(ctx, dt, ("^",), (), sr.Node("^", sr.Node(feature=1), sr.Node(feature=2)), X, True)
    assert ok and np.array_equal(g[0], [0.0, -3.0, 12.0, 4.0])
    assert np.array_equal(g[1][:3], [0.0, 0.0, 0.0]) and g[1][3] > 2.7  # 4 ln 2


@pytest.mark.parametrize("dt", DTS)
def test_convention_gamma_has_no_derivative(ctx, dt):
    """Every tangent through gamma is NaN, eval_grad_predict reports ok = False, and optimize_constants
    leaves gamma(c1 * x1) as it was (improved = False)."""
    sr = _sr()
    T = C.NP[dt]
    N = sr.Node
    X = np.stack([np.linspace(1.0, 3.0, 300)] * 3).astype(T)
    tree = N("gamma", N("*", N(val=1.25), N(feature=1)))
    for variable in (True, False):
        g, ok = _per_row(ctx, dt, ("*",), ("gamma",), tree, X, variable)
        assert not ok and np.isnan(g[0]).all()
    opts = sr.Options(binary_operators=("*",), unary_operators=("gamma",))
    nodes, offs = sr.flatten([tree], opts, T)
    prog = sr.Program(ctx, nodes, offs, opts, T)
    ds = sr.DeviceDataset(ctx, X, (2 * X[0]).astype(T))
    before = np.concatenate(prog.get_constants())
    _, improved, _ = prog.optimize_constants(ds, sr.L2DistLoss(), iterations=4, nrestarts=1, seed=1)
    after = np.concatenate(prog.get_constants())
    assert not improved[0] and np.array_equal(_bits(before), _bits(after)) and after[0] == 1.25
