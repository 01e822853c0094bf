"""Every built-in loss value (the bodies loss_elem and margin_loss of csrc/srhip_ops.h, applied by loss_tile in
csrc/srhip_eval_impl.h and by the dual-number tile) against exact math on every scoring path: the golden table
tests/golden/loss_values.npz through the data and the bars of tests/loss_values_common.py.

The prediction tree is the leaf x1, so what the loss epilogue sees is bit for bit the tabulated residual
d = x1 - y or agreement a = y * x1.  20 kinds x Float32 / Float64 x unweighted / weighted; every test prints
the worst multiple of eps * scale it saw (LOSS_ERR ...; the device column of DESIGN.md's table)."""
import ctypes

import numpy as np
import pytest

import forward_values_common as fv
import loss_values_common as C

pytestmark = pytest.mark.gpu

DTS = ["f32", "f64"]
WEIGHTED = [False, True]
NPOP = 24  # the population of the tiled tests
SMALL, PERSISTENT, GRID = 0, 1, 2
cases = pytest.mark.parametrize("weighted", WEIGHTED, ids=["plain", "weighted"])
dts = pytest.mark.parametrize("dt", DTS)
kinds = pytest.mark.parametrize("kind", C.KINDS)
_CACHE = {}


def _sr():
    import srhip

    return srhip


def _program(ctx, dt, ntrees, const=None):
    """ntrees copies of the tree x1 (const: of x1 + const)."""
    sr = _sr()
    key = ("prog", dt, ntrees, const)
    if key not in _CACHE:
        N = sr.Node
        opts = sr.Options(binary_operators=("+",), unary_operators=())
        tree = (lambda: N(feature=1)) if const is None else (lambda: N("+", N(feature=1), N(val=const)))
        nodes, offs = sr.flatten([tree() for _ in range(ntrees)], opts, C.NP[dt])
        _CACHE[key] = sr.Program(ctx, nodes, offs, opts, C.NP[dt])
    return _CACHE[key]


def _dataset(ctx, blk, w, tag):
    """The device dataset of a Block (one column, x1) with weights w; uploaded once per tag."""
    key = ("ds", blk.family, blk.dt, blk.n, tag)
    if key not in _CACHE:
        _CACHE[key] = _sr().DeviceDataset(ctx, blk.x1[None, :], blk.y, w)
    return _CACHE[key]


def _problem(ctx, kind, dt, weighted, which=("general", "kinks"), n=None, pow2=False, shift=0.0):
    """(block, weights or None, dataset, loss object) of one case."""
    blk = C.rows(C.family(kind), dt, which=which, n=n, shift=shift)
    w = C.weights(dt, blk.n, pow2) if weighted else None
    ds = _dataset(ctx, blk, w, (tuple(which), shift, weighted, pow2))
    return blk, w, ds, C.loss_object(_sr(), kind)


def _same_bits(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return bool(np.all((C.bits(a) == C.bits(b)) | (np.isnan(a) & np.isnan(b))))


def _plan(dt, nlive, m, weighted, loss):
    import srhip._lib as L

    q = dict(dtype=L.F32 if dt == "f32" else L.F64, mode=0, nlive=nlive, m=m, maxfeat=1, nd=0, kmax=2, dkmax=0, wide_ops=0,
             weighted=int(weighted), sharded=0, have_recs=1, loss_kind=loss.c_struct().kind, num_cu=256, lds_max=163840)
    out = L.PlanInfo()
    assert L.load().srhip_plan_eval(ctypes.byref(L.PlanQuery(**q)), ctypes.byref(out)) == 0
    return {name: getattr(out, name) for name, _ in L.PlanInfo._fields_ if name != "pad"}


# ---- 1. per-row values ------------------------------------------------------------------------------
@cases
@dts
@kinds
def test_per_row_values(ctx, oracle, kind, dt, weighted):
    """One x1 tree per row, tree t scored on the row set {t} in one eval_loss_rowsets launch: with weights
    that are powers of two, out_loss[t] is row t's loss in T.  General and kink rows meet the per-row bar
    against the table; extreme rows have the class of the CPU restatement of the formula in T, the finite
    ones meet the bar too, and ok = 1 everywhere (the prediction is finite).  eval_loss(idx=[t]) returns
    the same bits (three rows)."""
    blk, w, ds, loss = _problem(ctx, kind, dt, weighted, which=("general", "kinks", "extreme"), pow2=True)
    prog = _program(ctx, dt, blk.n)
    got, ok = prog.eval_loss_rowsets(ds, loss, [[t] for t in range(blk.n)])
    assert ctx.rowsets_fallback_trees() == 0, "the row-set kernel did not answer"
    assert ok.all()
    exact, x = blk.exact_of(kind), blk.v
    ntab = blk.n - len(C.table()[f"ext_{'d' if blk.family == 'dist' else 'a'}_{dt}"])
    tab = np.arange(blk.n) < ntab
    assert np.isfinite(got[tab]).all(), (kind, dt, x[tab][~np.isfinite(got[tab])][:5])
    worst = C.check_rows(kind, dt, got[tab], exact[tab], x[tab], "device rows")
    ref = C.oracle_rows(oracle, _sr(), kind, blk)
    cls, rcls = C.classes(got), C.classes(ref)
    assert np.array_equal(cls[~tab], rcls[~tab]), (kind, dt, [(float(v), C.CLASS_NAMES[a], C.CLASS_NAMES[b])
                                                               for v, a, b in zip(x[~tab], cls[~tab], rcls[~tab])])
    fin = ~tab & (rcls == 0)
    worst_ext = C.check_rows(kind, dt, got[fin], exact[fin], x[fin], "device extreme rows")
    for t in (0, ntab - 1, blk.n - 1):
        l1, ok1 = prog.eval_loss(ds, loss, idx=[t])
        assert ok1.all() and _same_bits(l1[t], got[t]) and _same_bits(l1, np.full(blk.n, l1[0])), (kind, dt, t)
    C.report("rows", kind, dt, worst, "_w" if weighted else "")
    C.report("rows_extreme", kind, dt, worst_ext, "_w" if weighted else "")


@cases
@dts
def test_parameter_the_type_does_not_hold(ctx, dt, weighted):
    """L1EpsilonIns at 0.3 (not a Float32 number) at |d| = prev, T(0.3), next: equality with exact math at
    T(0.3), which a kernel that used the decimal parameter misses at |d| = T(0.3) (0 against 1.2e-8)."""
    kind = C.GEN.PAR_KIND
    blk = C.rows("dist", dt, which=("param",))
    w = C.weights(dt, blk.n, True) if weighted else None
    ds = _dataset(ctx, blk, w, ("param", weighted))
    loss = C.param_loss(_sr())
    prog = _program(ctx, dt, blk.n)
    got, ok = prog.eval_loss_rowsets(ds, loss, [[t] for t in range(blk.n)])
    assert ctx.rowsets_fallback_trees() == 0 and ok.all()
    C.check_rows(kind, dt, got, blk.exact_of(kind), blk.v, "parameter rows")
    assert got[1] == 0 and got[4] == 0 and got[2] > 0
    l1, ok1 = prog.eval_loss(ds, loss, idx=[1])
    assert ok1.all() and np.all(l1 == 0)


# ---- 2. one block, fused reduction ------------------------------------------------------------------
@cases
@dts
@kinds
def test_one_block_mean(ctx, monkeypatch, kind, dt, weighted):
    """eval_loss over the general and kink rows (one row block: the waves finish the reduction themselves)
    meets the bar of a mean; the reduce kernel (SRHIP_NO_FUSED_REDUCE=1) returns the same bits."""
    blk, w, ds, loss = _problem(ctx, kind, dt, weighted)
    prog = _program(ctx, dt, NPOP)
    got, ok = prog.eval_loss(ds, loss)
    assert ok.all() and _same_bits(got, np.full(NPOP, got[0]))
    assert _plan(dt, NPOP, blk.n, weighted, loss)["fused"] == 1
    mult = C.check_mean(kind, dt, got[0], blk.exact_of(kind), blk.v, w, "one block")
    monkeypatch.setenv("SRHIP_NO_FUSED_REDUCE", "1")
    assert _plan(dt, NPOP, blk.n, weighted, loss)["fused"] == 0
    g2, ok2 = prog.eval_loss(ds, loss)
    monkeypatch.delenv("SRHIP_NO_FUSED_REDUCE")
    assert ok2.all() and _same_bits(g2, got)
    C.report("one_block", kind, dt, mult, "_w" if weighted else "")


# ---- 3. tiled shapes and every launch form, 4. gathered view, 5. partials ---------------------------
@cases
@dts
@kinds
def test_tiled_every_launch_form(ctx, monkeypatch, kind, dt, weighted):
    """The points cyclically over 4096 + 65 rows (Float32: R = 16, a ragged last tile, the persistent hot
    form) or 3 * 256 + 7 rows (Float64: a grid launch), 24 trees: the form the plan names is the form that
    ran, every form meets the bar of a mean, and the general persistent form and the grid launch return the
    hot form's bits.  The same data through a gathered view (a permutation of the rows plus 37
    duplicates) against the table by index, and through eval_loss_partials + finalize with the bits of
    eval_loss."""
    n = fv.TILED_ROWS[dt]
    blk, w, ds, loss = _problem(ctx, kind, dt, weighted, n=n)
    prog = _program(ctx, dt, NPOP)
    exact, x = blk.exact_of(kind), blk.v
    pl = _plan(dt, NPOP, n, weighted, loss)
    if dt == "f32":
        assert (pl["kind"], pl["R"], pl["hot"], pl["fused"]) == (PERSISTENT, 16, 1, 0)
    else:
        assert pl["kind"] == GRID and pl["hot"] == 0
    h0 = ctx.hot_form_launches()
    got, ok = prog.eval_loss(ds, loss)
    assert ok.all() and _same_bits(got, np.full(NPOP, got[0]))
    mult = C.check_mean(kind, dt, got[0], exact, x, w, "tiled")
    if dt == "f32":
        assert ctx.hot_form_launches() == h0 + 1, "not a hot-form launch"
        for flag, want in (("SRHIP_NO_HOT_FORM", dict(kind=PERSISTENT, hot=0)), ("SRHIP_NO_PERSISTENT", dict(kind=GRID, hot=0))):
            monkeypatch.setenv(flag, "1")
            p2 = _plan(dt, NPOP, n, weighted, loss)
            assert {k: p2[k] for k in want} == want, flag
            g2, ok2 = prog.eval_loss(ds, loss)
            monkeypatch.delenv(flag)
            assert ok2.all() and _same_bits(g2, got), flag
        assert ctx.hot_form_launches() == h0 + 1
    # 4. a gathered view
    rng = np.random.default_rng(5)
    idx = np.concatenate([rng.permutation(n), rng.integers(0, n, 37)])
    gi, oki = prog.eval_loss(ds, loss, idx=idx)
    assert oki.all() and _same_bits(gi, np.full(NPOP, gi[0]))
    mult_g = C.check_mean(kind, dt, gi[0], exact[idx], x[idx], None if w is None else w[idx], "gathered")
    # 5. partials
    sums, chk = prog.eval_loss_partials(ds, loss)
    lp, okp, st = prog.finalize(1, sums, chk)
    assert okp.all() and not (st == 2).any() and _same_bits(lp, got)
    C.report("tiled", kind, dt, mult, "_w" if weighted else "")
    C.report("gathered", kind, dt, mult_g, "_w" if weighted else "")


@cases
@dts
@kinds
def test_small_population_form(ctx, kind, dt, weighted):
    """Few trees over many rows (64 * 4096 + 65 rows of one column, 4 trees): the launch of one wave per tree
    and loss chunk, reading X from global memory."""
    n = C.SMALL_POP_ROWS
    blk, w, ds, loss = _problem(ctx, kind, dt, weighted, n=n)
    prog = _program(ctx, dt, 4)
    assert _plan(dt, 4, n, weighted, loss)["kind"] == SMALL
    got, ok = prog.eval_loss(ds, loss)
    assert ok.all() and _same_bits(got, np.full(4, got[0]))
    C.report("small_pop", kind, dt, C.check_mean(kind, dt, got[0], blk.exact_of(kind), blk.v, w, "small"),
             "_w" if weighted else "")


# ---- 6. the gradient kernel's loss ------------------------------------------------------------------
@cases
@dts
@kinds
def test_gradient_kernels_loss(ctx, kind, dt, weighted):
    """eval_loss_grad's out_loss (the dual-number tile applies the loss through loss_dloss_generic) of the
    tree x1 + c: at c = 0.5 on the general rows with x1 = pred - 0.5 (exact there), and at c = 0 on the
    general and kink rows (pred - 0.5 is not representable beside the kinks at 0).  eval_loss_grad_rowsets on
    full-length sets returns the same bits."""
    worst = 0.0
    for const, which in ((0.5, ("general",)), (0.0, ("general", "kinks"))):
        blk, w, ds, loss = _problem(ctx, kind, dt, weighted, which=which, shift=const)
        prog = _program(ctx, dt, 2, const=const)
        got, g, ok = prog.eval_loss_grad(ds, loss)
        assert ok.all() and _same_bits(got, np.full(2, got[0])) and g[0].shape == (1,)
        worst = max(worst, C.check_mean(kind, dt, got[0], blk.exact_of(kind), blk.v, w, ("grad", const)))
        rl, rg, rok = prog.eval_loss_grad_rowsets(ds, loss, [np.arange(blk.n)] * 2)
        assert rok.all() and _same_bits(rl, got) and _same_bits(np.concatenate(rg), np.concatenate(g)), (kind, dt, const)
    C.report("grad_loss", kind, dt, worst, "_w" if weighted else "")


# ---- 7. a non-finite loss on the last row -----------------------------------------------------------
@pytest.mark.parametrize("pos", ["last", "middle"])
@pytest.mark.parametrize("n", [300, 4096 + 65])
@pytest.mark.parametrize("dt,kind,point", [(dt, k, p) for dt in DTS for k, p in C.INF_POINTS[dt]])
def test_infinite_loss_at_a_finite_prediction(ctx, oracle, dt, kind, point, n, pos):
    """Weighted data whose row count is no multiple of the tile, one row's loss being +Inf at a finite
    prediction: the weighted mean is +Inf with ok = 1 (sum(w .* l) / sum(w), the CPU restatement's result),
    from eval_loss, from a gathered view that ends with that row and from row sets that end with it.  The
    rows that pad the last tile repeat the last row with weight 0, and 0 * Inf must not reach the sum."""
    sr = _sr()
    T = C.NP[dt]
    fam = C.family(kind)
    blk = C.rows(fam, dt, which=("general",), n=n)
    at = n - 1 if pos == "last" else n // 2
    x1, y = blk.x1.copy(), blk.y.copy()
    if fam == "dist":
        x1[at], y[at] = T(point), T(0)
    else:
        x1[at] = T(point) / y[at]
        assert y[at] * x1[at] == T(point)
    w = C.weights(dt, n, False)
    loss = C.loss_object(sr, kind)
    ls = loss.c_struct()
    opts = sr.Options(binary_operators=("+",), unary_operators=())
    nodes, offs = sr.flatten([sr.Node(feature=1)] * 2, opts, T)
    ref, _, rok = oracle.eval_loss(nodes[offs[0]:offs[1]].copy(), opts.binop_codes, opts.unaop_codes, x1[None, :], y, w,
                                   kind=ls.kind, p0=ls.p0)
    assert rok and ref == np.inf
    ds = sr.DeviceDataset(ctx, x1[None, :], y, w)
    prog = _program(ctx, dt, 2)
    got, ok = prog.eval_loss(ds, loss)
    assert ok.all() and np.all(got == np.inf), ("eval_loss", got)
    rng = np.random.default_rng(9)
    others = np.delete(np.arange(n), at)
    perm = rng.permutation(others)
    idx = np.concatenate([perm, [at]]) if pos == "last" else np.concatenate([perm[:n // 2], [at], perm[n // 2:]])
    got, ok = prog.eval_loss(ds, loss, idx=idx)
    assert ok.all() and np.all(got == np.inf), ("eval_loss idx", got)
    sets = [np.concatenate([perm[:m - 1], [at]]) if pos == "last" else np.concatenate([perm[:m // 2], [at], perm[m // 2:m - 1]])
            for m in (50, 257)]
    got, ok = prog.eval_loss_rowsets(ds, loss, sets)
    assert ctx.rowsets_fallback_trees() == 0
    assert ok.all() and np.all(got == np.inf), ("eval_loss_rowsets", got)


@pytest.mark.parametrize("zero", [0.0, -0.0], ids=["+0", "-0"])
@pytest.mark.parametrize("n", [300, 4096 + 65])
@pytest.mark.parametrize("dt,kind,point", [(dt, *C.INF_POINTS[dt][0]) for dt in DTS] + [(dt, *C.INF_POINTS[dt][2]) for dt in DTS])
def test_a_callers_zero_weight_on_an_infinite_loss_is_nan(ctx, oracle, dt, kind, point, n, zero):
    """Only the rows that pad a tile are left out.  A caller's own weight of zero, of either sign (an uploaded
    -0.0 is stored as +0.0, so that it is not taken for the padding weight), on the last row, whose loss is
    +Inf: 0 * Inf = NaN, as sum(w .* l) / sum(w) and the CPU restatement give, with ok = 1."""
    sr = _sr()
    T = C.NP[dt]
    fam = C.family(kind)
    blk = C.rows(fam, dt, which=("general",), n=n)
    at = n - 1
    x1, y = blk.x1.copy(), blk.y.copy()
    if fam == "dist":
        x1[at], y[at] = T(point), T(0)
    else:
        x1[at] = T(point) / y[at]
    w = C.weights(dt, n, False).copy()
    w[at] = T(zero)
    assert w[at] == 0 and bool(np.signbit(w[at])) == bool(np.signbit(zero))
    loss = C.loss_object(sr, kind)
    ls = loss.c_struct()
    opts = sr.Options(binary_operators=("+",), unary_operators=())
    nodes, offs = sr.flatten([sr.Node(feature=1)] * 2, opts, T)
    ref, _, rok = oracle.eval_loss(nodes[offs[0]:offs[1]].copy(), opts.binop_codes, opts.unaop_codes, x1[None, :], y, w,
                                   kind=ls.kind, p0=ls.p0)
    assert rok and np.isnan(ref)
    ds = sr.DeviceDataset(ctx, x1[None, :], y, w)
    prog = _program(ctx, dt, 2)
    got, ok = prog.eval_loss(ds, loss)
    assert ok.all() and np.isnan(got).all(), ("eval_loss", got)
    perm = np.random.default_rng(9).permutation(n - 1)
    got, ok = prog.eval_loss(ds, loss, idx=np.concatenate([perm, [at]]))
    assert ok.all() and np.isnan(got).all(), ("eval_loss idx", got)
    got, ok = prog.eval_loss_rowsets(ds, loss, [np.concatenate([perm[:m - 1], [at]]) for m in (50, 257)])
    assert ctx.rowsets_fallback_trees() == 0
    assert ok.all() and np.isnan(got).all(), ("eval_loss_rowsets", got)


# ---- 8. Int32 ---------------------------------------------------------------------------------------
def _wrap(v):
    return (int(v) + 2 ** 31) % 2 ** 32 - 2 ** 31


def test_int32_losses_wrap_as_python_integers(ctx):
    """L1 and L2 on 67 rows whose pred - y are the Int32 edge values (-2^31, 46341, ...), once directly
    (y = 0) and once as a wrapped difference of two of them: wrap to 32 bits, sum exactly, divide by n.
    Every other kind is SRHIP_ERR_UNSUPPORTED."""
    sr = _sr()
    a, b = fv.int_inputs()
    opts = sr.Options(binary_operators=("+",), unary_operators=())
    nodes, offs = sr.flatten([sr.Node(feature=1)] * 2, opts, np.int32)
    prog = sr.Program(ctx, nodes, offs, opts, np.int32)
    n = len(a)
    assert n == 67 and -2 ** 31 in a and 46341 in a
    for y in (np.zeros(n, np.int32), b):
        ds = sr.DeviceDataset(ctx, a[None, :], y)
        d = [_wrap(int(p) - int(q)) for p, q in zip(a, y)]
        for kind, f in (("L1", lambda v: _wrap(abs(v))), ("L2", lambda v: _wrap(v * v))):
            want = sum(f(v) for v in d) / n
            got, ok = prog.eval_loss(ds, C.loss_object(sr, kind))
            assert ok.all() and got[0] == want and got[1] == want, (kind, got, want)
    for kind in C.KINDS:
        if kind not in ("L1", "L2"):
            with pytest.raises(sr._lib.SrhipError) as e:
                prog.eval_loss(ds, C.loss_object(sr, kind))
            assert e.value.code == sr._lib.ERR_UNSUPPORTED, kind
