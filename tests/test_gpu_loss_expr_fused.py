"""A loss given as an expression in ONE launch (csrc/srhip_eval_lossx.hip): srhip_eval_loss_expr_fused,
srhip_eval_loss_expr_submit / srhip_eval_loss_wait and the expression coalescer, bit for bit against the
two-pass srhip_eval_loss_expr (Program.eval_loss under an ExprLoss), which this work leaves as it is.
Every comparison is == on bits unless it says exact integers."""
import ctypes
import threading

import numpy as np
import pytest

import srhip
from srhip import _lib
from srhip import search as S

import loss_expr_common as X

pytestmark = pytest.mark.gpu

B = 4096  # LOSSX_BLOCK_ROWS (tests/test_gpu_loss_expr.py checks it against the library's getter)
DTYPES = [np.float32, np.float64]
DT_IDS = ["f32", "f64"]
TREE_OPS = dict(binary_operators=("+", "-", "*", "/"), unary_operators=("cos", "exp"))
NFEAT = 5


def _bits(v):
    return np.asarray(v, dtype=np.float64).view(np.uint64)


def _x(i):
    return srhip.Node(feature=i)


def _c(v):
    return srhip.Node(val=float(v))


def _cos(a):
    return srhip.Node("cos", a)


def _exp(a):
    return srhip.Node("exp", a)


def _program(ctx, trees, dtype, opts=None):
    opts = opts or srhip.Options(**TREE_OPS)
    nodes, offs = srhip.flatten(trees, opts, dtype)
    return srhip.Program(ctx, nodes, offs, opts, dtype)


def _lp():
    return X.N("abs", X.diff()) ** X.C(2.5)


def _loss(weighted):
    return srhip.ExprLoss(X.W() * _lp() if weighted else _lp(), X.options())


def _population():
    """A leaf; nine constants; cos of an operator output; a stack need above 2; a static failure; a tree that
    fails only where x5 is huge (exp overflows) -- no other tree reads x5."""
    nine = (_x(1) * 1.5 + _x(2) * -0.25) * 0.75 + (_x(3) * 2.5 - _x(4) * 0.125) * 1.25 + (_x(1) * 3.5 + 0.0625) * -1.75
    deep = ((_x(1) * _x(2) + _x(3) * _x(4)) * (_x(2) * _x(3) - _x(4) * _x(1))) + ((_x(1) + _x(3)) * (_x(2) - _x(4)))
    return [_x(2), nine, _cos(_x(1) * _x(2) + _x(3)), deep, _x(1) + _c(np.inf), _exp(_x(5)) + _x(1)]


def _data(dtype, m, seed=0, last_bad=True):
    rng = np.random.default_rng(seed + m)
    Xd = rng.standard_normal((NFEAT, m)).astype(dtype)
    if last_bad:
        Xd[4, m - 1] = 1000.0  # exp overflows in both types: the sixth tree fails on this row, in the last block
    y = (2 * np.cos(Xd[1]) + Xd[0] ** 2 - 2).astype(dtype)
    w = rng.uniform(0.5, 2.0, m).astype(dtype)
    return Xd, y, w


def _same(got, gok, want, wok):
    assert np.array_equal(gok, wok), (gok, wok)
    assert np.array_equal(_bits(got), _bits(want)), (got, want)


# ---- 1. fused equals two-pass -----------------------------------------------------------------------------
SIZES = [1, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 4095, 4096, 4097, 8191, 8192, 8193, 12289]


@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weighted"])
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("m", SIZES)
def test_fused_equals_two_pass(ctx, m, dtype, weighted):
    Xd, y, w = _data(dtype, m)
    ds = srhip.DeviceDataset(ctx, Xd, y, w if weighted else None)
    prog = _program(ctx, _population(), dtype)
    loss = _loss(weighted)
    want, wok = prog.eval_loss(ds, loss)
    got, gok = prog.eval_loss_fused(ds, loss)
    assert wok.tolist() == [True, True, True, True, False, False]
    _same(got, gok, want, wok)
    assert np.all(np.isposinf(got[~gok])) and np.all(np.isfinite(got[gok]))
    assert ctx.last_kernel_ms() >= 0
    prog.close()


# ---- 2. the same with idx ---------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weighted"])
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_fused_equals_two_pass_with_idx(ctx, dtype, weighted):
    n = 20000
    Xd, y, w = _data(dtype, n, last_bad=False)
    Xd[4, 777] = 1000.0
    ds = srhip.DeviceDataset(ctx, Xd, y, w if weighted else None)
    prog = _program(ctx, _population(), dtype)
    loss = _loss(weighted)
    rng = np.random.default_rng(5)
    for nidx in (1, 4097, 8193):
        idx = rng.integers(0, n, size=nidx)
        if nidx > 1:
            idx[-1] = idx[0]  # a duplicate
            idx[nidx - 2] = 777  # the failing row, in the last block
        want, wok = prog.eval_loss(ds, loss, idx)
        got, gok = prog.eval_loss_fused(ds, loss, idx)
        _same(got, gok, want, wok)
        assert bool(gok[5]) == (nidx == 1 and idx[0] != 777)
    prog.close()


# ---- 3. many items per workgroup --------------------------------------------------------------------------
def test_many_items_per_workgroup(ctx):
    opts = srhip.Options(**TREE_OPS)
    dtype = np.float32
    loss = _loss(False)
    # 3 trees x 38 row blocks: one tree group, more row blocks than a group has waves
    m = 37 * B + 5
    Xd, y, _ = _data(dtype, m)
    ds = srhip.DeviceDataset(ctx, Xd, y)
    prog = _program(ctx, _population()[1:4], dtype)
    _same(*prog.eval_loss_fused(ds, loss), *prog.eval_loss(ds, loss))
    prog.close()
    # 1500 trees x 3 rows: more tree groups than workgroups
    trees = srhip.random_population(1500, opts, NFEAT, dtype, seed=13, max_size=20)
    Xd, y, _ = _data(dtype, 3, last_bad=False)
    ds = srhip.DeviceDataset(ctx, Xd, y)
    prog = _program(ctx, trees, dtype)
    want, wok = prog.eval_loss(ds, loss)
    got, gok = prog.eval_loss_fused(ds, loss)
    assert wok.sum() > 1000
    _same(got, gok, want, wok)
    prog.close()


# ---- 4. a tree whose record leaves did_succeed open -------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_near_overflow_tree(ctx, dtype):
    """tests/test_gpu_precise.py's huge operands cancelling to zero: every row is finite, the check statistic
    is in the undecided band, the precise pass says ok.  (Float64: 1e305 |x| over 5000 rows of |x| ~ 0.8 adds up
    past 2^1023, the signed sum stays near 1e307.)"""
    big = 1.0e35 if dtype == np.float32 else 1.0e305
    m = 5000
    Xd, y, _ = _data(dtype, m, last_bad=False)
    trees = [_x(1) * big - _x(1) * big, _x(1) + _x(2), (_x(1) * big) * _x(2) * big * big * big]
    ds = srhip.DeviceDataset(ctx, Xd, y)
    prog = _program(ctx, trees, dtype)
    psums, pchk = prog.eval_loss_partials(ds, srhip.L2DistLoss())
    _, _, st = prog.finalize(NFEAT, psums, pchk)
    assert st[0] == 2, st  # undecided by the record
    loss = _loss(False)
    want, wok = prog.eval_loss(ds, loss)
    got, gok = prog.eval_loss_fused(ds, loss)
    assert wok.tolist() == [True, True, False]
    _same(got, gok, want, wok)
    prog.close()


# ---- 5. exact integer sums, independent of the reference route --------------------------------------------
INT_FORMS = [
    (lambda k: _x(1) + _x(2) + float(k), lambda F, k: F[0] + F[1] + k),
    (lambda k: _x(1) * _x(2) - _x(3) + float(k), lambda F, k: F[0] * F[1] - F[2] + k),
    (lambda k: _x(3) - _x(1) * float(k), lambda F, k: F[2] - F[0] * k),
    (lambda k: _x(2) * _x(3) + _x(1), lambda F, k: F[1] * F[2] + F[0]),
    (lambda k: _x(1) + float(k), lambda F, k: F[0] + k),
]


@pytest.mark.parametrize("m", [1, 63, 64, 65, 255, 256, 257, B - 1, B, B + 1, 3 * B + 1])
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_exact_integer_sums(ctx, dtype, m):
    """Integer features (|v| <= 16), targets j mod 97, weights 1..7: every prediction, every abs(p - t) and
    every partial sum is an integer that T and double hold exactly, so the device's loss times the divisor is
    the exact integer whatever the summation order: its quotient by the divisor has one bit pattern."""
    rng = np.random.default_rng(1000 + m)
    F = rng.integers(-16, 17, size=(3, m))
    y = np.arange(m) % 97
    w = rng.integers(1, 8, size=m)
    lopts = X.options()
    l1 = srhip.ExprLoss(X.N("abs", X.diff()), lopts)
    l1w = srhip.ExprLoss(X.W() * X.N("abs", X.diff()), lopts)
    ds = srhip.DeviceDataset(ctx, F.astype(dtype), y.astype(dtype))
    dsw = srhip.DeviceDataset(ctx, F.astype(dtype), y.astype(dtype), w.astype(dtype))
    nb = len(INT_FORMS)
    for npop in (1, 37):
        trees = [INT_FORMS[k % nb][0](k // nb) for k in range(npop)]
        preds = [INT_FORMS[k % nb][1](F, k // nb) for k in range(npop)]
        prog = _program(ctx, trees, dtype)
        got, ok = prog.eval_loss_fused(ds, l1)
        assert ok.all()
        want = np.array([int(np.abs(p - y).sum()) / m for p in preds])
        assert np.array_equal(_bits(got), _bits(want))
        got, ok = prog.eval_loss_fused(dsw, l1w)
        want = np.array([int((w * np.abs(p - y)).sum()) / int(w.sum()) for p in preds])
        assert ok.all() and np.array_equal(_bits(got), _bits(want))
        prog.close()


# ---- 6. the reduction contract ------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_reduction_contract(ctx, dtype):
    """A tree's loss is the same bits alone, at any position of a permuted population, beside failed trees, and
    in populations of 1 / 2 / 37 trees."""
    m = 3 * B + 1
    Xd, y, _ = _data(dtype, m)
    ds = srhip.DeviceDataset(ctx, Xd, y)
    loss = _loss(False)
    opts = srhip.Options(**TREE_OPS)
    base = _population() + srhip.random_population(31, opts, 4, dtype, seed=11, max_size=14)
    assert len(base) == 37
    alone = []
    for t in base:
        prog = _program(ctx, [t], dtype)
        l, ok = prog.eval_loss_fused(ds, loss)
        alone.append((l[0], bool(ok[0])))
        prog.close()
    assert alone[4][1] is False and alone[5][1] is False and sum(ok for _, ok in alone) >= 20
    rng = np.random.default_rng(3)
    for perm in (np.arange(37), rng.permutation(37), rng.permutation(37)[:2], np.array([6, 4, 5, 1, 4])):
        prog = _program(ctx, [base[k] for k in perm], dtype)
        got, gok = prog.eval_loss_fused(ds, loss)
        for pos, k in enumerate(perm):
            assert bool(gok[pos]) == alone[k][1], (pos, k)
            assert _bits(got[pos]) == _bits(alone[k][0]), (pos, k, got[pos], alone[k][0])
        prog.close()


# ---- 7. residency -------------------------------------------------------------------------------------------
def test_no_residency_cap(ctx, monkeypatch):
    dtype = np.float32
    m = 8193
    opts = srhip.Options(**TREE_OPS)
    trees = srhip.random_population(64, opts, NFEAT, dtype, seed=17, max_size=16)
    Xd, y, _ = _data(dtype, m, last_bad=False)
    ds = srhip.DeviceDataset(ctx, Xd, y)
    prog = _program(ctx, trees, dtype)
    loss = _loss(False)
    want, wok = prog.eval_loss(ds, loss)
    monkeypatch.setenv("SRHIP_LOSSX_MAX_BYTES", "1048576")
    with pytest.raises(srhip.SrhipError) as ei:
        prog.eval_loss(ds, loss)
    assert ei.value.code == _lib.ERR_NOMEM
    got, gok = prog.eval_loss_fused(ds, loss)
    monkeypatch.delenv("SRHIP_LOSSX_MAX_BYTES")
    _same(got, gok, want, wok)
    prog.close()


# ---- 8. submit / wait -----------------------------------------------------------------------------------------
def test_submit_wait(ctx):
    dtype = np.float32
    m = 2 * B + 17
    opts = srhip.Options(**TREE_OPS)
    Xd, y, _ = _data(dtype, m)
    ds = srhip.DeviceDataset(ctx, Xd, y)
    loss = _loss(False)
    progs = [_program(ctx, _population() + srhip.random_population(20 + 7 * k, opts, 4, dtype, seed=40 + k, max_size=14),
                      dtype) for k in range(3)]
    want = [p.eval_loss(ds, loss) for p in progs]
    tickets = [p.eval_loss_submit(ds, loss) for p in progs]
    with pytest.raises(srhip.SrhipError) as ei:
        progs[0].eval_loss_submit(ds, loss)
    assert ei.value.code == _lib.ERR_INVALID and "3 evaluations already in flight" in str(ei.value)
    for k in (2, 1, 0):
        _same(*tickets[k].wait(), *want[k])
    # one built-in and two expression tickets count as three
    l2 = srhip.L2DistLoss()
    want_l2 = progs[1].eval_loss(ds, l2)
    tickets = [progs[0].eval_loss_submit(ds, loss), progs[1].eval_loss_submit(ds, l2), progs[2].eval_loss_submit(ds, loss)]
    for sub_loss in (loss, l2):
        with pytest.raises(srhip.SrhipError) as ei:
            progs[0].eval_loss_submit(ds, sub_loss)
        assert "3 evaluations already in flight" in str(ei.value)
    _same(*tickets[1].wait(), *want_l2)
    _same(*tickets[2].wait(), *want[2])
    _same(*tickets[0].wait(), *want[0])
    # idx at submit
    idx = np.random.default_rng(9).integers(0, m, size=B + 3)
    t = progs[0].eval_loss_submit(ds, loss, idx)
    _same(*t.wait(), *progs[0].eval_loss(ds, loss, idx))
    for p in progs:
        p.close()


# ---- 9. validation ----------------------------------------------------------------------------------------------
def _raw(name, ctx, ds, prog, handle):
    lib = _lib.load()
    out, ok = np.empty(max(1, prog.ntrees)), np.empty(max(1, prog.ntrees), np.uint8)
    if name == "srhip_eval_loss_expr_submit":
        t = ctypes.c_void_p()
        rc = lib.srhip_eval_loss_expr_submit(ctx.handle, ds.handle, prog.handle, handle, None, 0, ctypes.byref(t))
        assert rc != 0 and not t.value
    else:
        rc = getattr(lib, name)(ctx.handle, ds.handle, prog.handle, handle, None, 0, _lib.ptr(out), _lib.ptr(ok))
    return rc, lib.srhip_last_error().decode() if rc else ""


def test_validation(ctx):
    m = 300
    rng = np.random.default_rng(3)
    Xd = rng.standard_normal((2, m)).astype(np.float32)
    y, w = rng.standard_normal(m).astype(np.float32), rng.uniform(1, 2, m).astype(np.float32)
    ds, dsw = srhip.DeviceDataset(ctx, Xd, y), srhip.DeviceDataset(ctx, Xd, y, w)
    prog = _program(ctx, [_x(1) + _x(2), _x(1) * _x(2)], np.float32)
    lopts = X.options()
    l2 = srhip.ExprLoss(X.N("square", X.diff()), lopts)
    l3 = srhip.ExprLoss(X.W() * X.N("square", X.diff()), lopts)
    iopts = srhip.Options(binary_operators=("+", "*"), unary_operators=())
    Xi = rng.integers(-5, 6, size=(2, m)).astype(np.int32)
    dsi = srhip.DeviceDataset(ctx, Xi, Xi[0])
    progi = _program(ctx, [_x(1) + _x(2)], np.int32, iopts)
    cases = [
        (ds, prog, None),                    # a null expression
        (ds, prog, l2.handle(np.float64)),   # a Float64 expression for a Float32 program
        (ds, prog, l3.handle(np.float32)),   # nargs 3 on an unweighted dataset
        (dsw, prog, l2.handle(np.float32)),  # nargs 2 on a weighted dataset
        (dsi, progi, l2.handle(np.float32)), # an Int32 program
    ]
    for d, p, h in cases:
        want = _raw("srhip_eval_loss_expr", ctx, d, p, h)
        assert want[0] != 0 and want[1]
        for name in ("srhip_eval_loss_expr_fused", "srhip_eval_loss_expr_submit"):
            assert _raw(name, ctx, d, p, h) == want, name
    assert _raw("srhip_eval_loss_expr", ctx, dsi, progi, l2.handle(np.float32))[0] == _lib.ERR_UNSUPPORTED
    # the coalescer's constructor: the same code and message for what it can see before any program exists
    # (the flushes' programs take the dataset's dtype)
    lib = _lib.load()
    for d, p, h in cases:
        want = _raw("srhip_eval_loss_expr", ctx, d, p, h)
        cops = (iopts if p is progi else srhip.Options(**TREE_OPS)).c_operators()
        b = ctypes.c_void_p()
        rc = lib.srhip_batcher_create_expr(ctx.handle, d.handle, ctypes.byref(cops), h, 8, 100, ctypes.byref(b))
        assert (rc, lib.srhip_last_error().decode()) == want and not b.value
    # the context still works, and no ticket was taken
    _same(*prog.eval_loss_fused(ds, l2), *prog.eval_loss(ds, l2))
    ts = [prog.eval_loss_submit(ds, l2) for _ in range(3)]
    for t in ts:
        t.wait()


# ---- 10. the coalescer ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
def test_coalescer_under_an_expression(dtype):
    o = srhip.Options(**TREE_OPS)
    m = 5000
    Xd, y, _ = _data(dtype, m, last_bad=False)
    loss = _loss(False)
    trees = srhip.random_population(96, o, NFEAT, dtype, seed=3, max_size=20)
    nodes, offs = srhip.flatten(trees, o, dtype)
    rng = np.random.default_rng(8)
    idxs = [rng.integers(0, m, size=50) if i % 3 == 0 else None for i in range(len(trees))]
    ref_ctx = srhip.Context(0)
    ref_ds = srhip.DeviceDataset(ref_ctx, Xd, y)
    ref = []
    for i in range(len(trees)):
        p = srhip.Program(ref_ctx, nodes[offs[i]:offs[i + 1]], np.array([0, offs[i + 1] - offs[i]], np.int64), o, dtype)
        l, ok = p.eval_loss(ref_ds, loss, idxs[i])
        ref.append((l[0], bool(ok[0])))
        p.close()
    ctx = srhip.Context(0)
    ds = srhip.DeviceDataset(ctx, Xd, y)
    co = srhip.Coalescer(ctx, ds, o, loss, max_batch=64, max_wait_us=500, nclients=8)
    got = [None] * len(trees)

    def client(k):
        for i in range(k, len(trees), 8):
            got[i] = co.score_loss(nodes[offs[i]:offs[i + 1]], idxs[i])

    th = [threading.Thread(target=client, args=(k,)) for k in range(8)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    st = co.stats()
    # a request that fails to compile returns its own error and the others succeed
    good, _ = srhip.flatten([_x(1) * 2.0], o, dtype)
    bad, _ = srhip.flatten([_x(1) * _x(9)], o, dtype)  # feature 9 of 5
    t1, t2, t3 = co.submit(good), co.submit(bad), co.submit(good)
    l1, ok1 = co.wait(t1)
    with pytest.raises(srhip.SrhipError):
        co.wait(t2)
    l3, ok3 = co.wait(t3)
    co.close()
    assert ok1 and ok3 and _bits(l1) == _bits(l3)
    for i, (l, ok) in enumerate(got):
        assert ok == ref[i][1], i
        assert _bits(l) == _bits(ref[i][0]), (i, l, ref[i][0])
    assert sum(ok for _, ok in ref) > 48
    assert st["requests"] == len(trees)
    assert st["launches"] < st["requests"], st


# ---- 11. the search ------------------------------------------------------------------------------------------------
def test_search_under_an_expression():
    """The README problem of tests/test_gpu_search.py with elementwise_loss = ExprLoss(square(p - t)): the
    default (non-batching) search scores through the expression coalescer."""
    rng = np.random.default_rng(0)
    Xd = rng.standard_normal((2, 100))
    y = 2 * np.cos(Xd[1]) + Xd[0] ** 2 - 2
    ops = dict(binary_operators=("+", "*", "/", "-"), unary_operators=("cos", "exp"))
    loss = srhip.ExprLoss(X.N("square", X.diff()), X.options())
    o = srhip.Options(populations=8, population_size=33, ncycles_per_iteration=100, maxsize=20, deterministic=True,
                      seed=1, elementwise_loss=loss, **ops)
    res = S.equation_search(Xd, y, o, niterations=2)
    hof = res.hall_of_fame
    members = [m for m, e in zip(hof.members, hof.exists) if e]
    front = res.pareto_frontier()
    assert 1 <= len(front) <= len(members)  # (the frontier is the dominating subset of those members)
    assert res.coalescer_stats["launches"] < res.coalescer_stats["requests"]
    ctx = srhip.get_context(0)
    ds = srhip.DeviceDataset(ctx, Xd, y)
    for mem in members:  # every hall-of-fame member, dominated ones included
        prog = _program(ctx, [mem.tree], np.float64, srhip.Options(**ops))
        l, ok = prog.eval_loss(ds, loss)
        assert _bits(l[0]) == _bits(mem.loss), (mem.loss, l[0])
        prog.close()
