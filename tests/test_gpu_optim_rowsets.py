"""srhip_eval_loss_grad_rowsets / srhip_optimize_constants_rowsets: every tree's constant gradient and
constant optimisation on a row subset of its own, the whole population in one call (the batching
mode's per-member minibatch of optimize_constants).  The contract is bit equality with the single-idx
entry points on the one-tree program with idx = the tree's set (and, for the optimiser, seed = the
tree's seed); the oracle on the gathered rows is the second reference for did_succeed and, for Float64,
for the gradient (the bound of tests/test_gpu_optim.py / test_gpu_configs.py's gradient checks:
1e-5 * max(1, |reference|); the suite holds Float32 gradients to no oracle bound, so Float32 is held to
the single calls' bits and the oracle's did_succeed).

Set lengths cycle through one row, a sub-tile set, the 256-row block edge on both sides, two and three
blocks, a set only Float32 can stage (1025 > the Float64 cap of 768 rows with 5 features) and one past
every cap (2049), where the call runs the tree through the single-idx path."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LENGTHS = [1, 2, 50, 64, 65, 255, 256, 257, 513, 1025, 2049]
N, NFEAT, NTREES = 5000, 5, 44
SEED = 101


def _sr():
    import srhip

    return srhip


def _opts(sr):
    return sr.Options(binary_operators=("+", "-", "*", "/"), unary_operators=("cos", "exp"))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _flat(gs):
    return np.concatenate([np.ravel(g) for g in gs]) if len(gs) else np.zeros(0)


def _one_tree(sr, ctx, nodes, offs, t, opts, dtype):
    nd = nodes[offs[t]:offs[t + 1]]
    return sr.Program(ctx, nd, np.array([0, len(nd)], dtype=np.int64), opts, dtype)


def _single_grads(sr, ctx, ds, nodes, offs, opts, dtype, loss, idxs, which=None):
    """prog_t.eval_loss_grad(ds, loss, idx=idx_t), one one-tree program per call."""
    out = {}
    for t in (range(len(idxs)) if which is None else which):
        p = _one_tree(sr, ctx, nodes, offs, t, opts, dtype)
        l, g, ok = p.eval_loss_grad(ds, loss, idx=idxs[t])
        p.close()
        out[t] = (_bits(l[:1])[0], _bits(g[0]).tolist(), bool(ok[0]))
    return out


def _as_triples(l, g, ok, which=None):
    return {t: (_bits(l[t:t + 1])[0], _bits(g[t]).tolist(), bool(ok[t])) for t in (range(len(ok)) if which is None else which)}


def _oracle_ok(oracle, nodes, offs, opts, X, y, w, idxs, kind=0, p0=0.0):
    ook = np.empty(len(idxs), dtype=bool)
    for t, i in enumerate(idxs):
        i = np.asarray(i)
        ook[t] = oracle.eval_loss(nodes[offs[t]:offs[t + 1]], opts.binop_codes, opts.unaop_codes, X[:, i].copy(), y[i].copy(),
                                  None if w is None else w[i].copy(), kind, p0)[2]
    return ook


_shared = {}


def _fixture(ctx, oracle, dtype, weighted):
    """One (dtype, weighting) case: data, sets, the rowsets call, the per-tree calls, the oracle's
    did_succeed -- computed once, shared by the tests below, never modified."""
    key = (np.dtype(dtype).name, weighted)
    if key in _shared:
        return _shared[key]
    sr = _sr()
    opts = _opts(sr)
    rng = np.random.default_rng(SEED + 1)
    X = rng.standard_normal((NFEAT, N)).astype(dtype)
    y = rng.standard_normal(N).astype(dtype)
    w = np.abs(rng.standard_normal(N)).astype(dtype) if weighted else None
    idxs = [rng.integers(0, N, size=LENGTHS[t % len(LENGTHS)]) for t in range(NTREES)]
    trees = sr.random_population(NTREES, opts, NFEAT, dtype, SEED, 20)
    nodes, offs = sr.flatten(trees, opts, dtype)
    ds = sr.DeviceDataset(ctx, X, y, w)
    prog = sr.Program(ctx, nodes, offs, opts, dtype)
    l, g, ok = prog.eval_loss_grad_rowsets(ds, sr.L2DistLoss(), idxs)
    kernel_ms = ctx.last_kernel_ms()
    single = _single_grads(sr, ctx, ds, nodes, offs, opts, dtype, sr.L2DistLoss(), idxs)
    ook = _oracle_ok(oracle, nodes, offs, opts, X, y, w, idxs)
    f = dict(sr=sr, opts=opts, X=X, y=y, w=w, idxs=idxs, nodes=nodes, offs=offs, ds=ds, prog=prog, l=l, g=g, ok=ok,
             single=single, ook=ook, kernel_ms=kernel_ms, dtype=dtype)
    _shared[key] = f
    return f


@pytest.mark.parametrize("dtype,weighted", [(np.float32, False), (np.float64, False), (np.float32, True)])
def test_gradient_parity_with_single_calls_and_oracle(ctx, oracle, dtype, weighted):
    f = _fixture(ctx, oracle, dtype, weighted)
    sr, opts, nodes, offs, X, y, w, idxs = (f[k] for k in ("sr", "opts", "nodes", "offs", "X", "y", "w", "idxs"))
    print(f"grad rowsets {np.dtype(dtype).name} weighted={weighted}: oracle ok {int(f['ook'].sum())}/{NTREES}, "
          f"kernel {f['kernel_ms']:.4f} ms")
    assert f["ook"].sum() >= 0.9 * NTREES, int(f["ook"].sum())
    got = _as_triples(f["l"], f["g"], f["ok"])
    for t in range(NTREES):
        assert got[t] == f["single"][t], (t, len(idxs[t]), got[t], f["single"][t])
    assert np.array_equal(f["ok"], f["ook"]), np.nonzero(f["ok"] != f["ook"])[0]
    assert f["kernel_ms"] > 0.0
    if dtype == np.float64:
        worst = 0.0
        for t in np.nonzero(f["ook"])[0]:
            i = idxs[t]
            ref = oracle.loss_grad(nodes[offs[t]:offs[t + 1]], opts.binop_codes, opts.unaop_codes, X[:, i].copy(), y[i].copy(),
                                   None if w is None else w[i].copy(), 0)
            assert len(ref) == len(f["g"][t])
            for k in range(len(ref)):
                a, b = f["g"][t][k], ref[k]
                if a == b or (np.isnan(a) and np.isnan(b)):
                    continue
                worst = max(worst, abs(a - b) / max(1.0, abs(b)))
                assert abs(a - b) <= 1e-5 * max(1.0, abs(b)), (t, k, a, b)
        print(f"  gradient vs oracle.loss_grad: worst |d| / max(1, |ref|) = {worst:.3e}")


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_results_do_not_depend_on_the_batch(ctx, oracle, dtype):
    f = _fixture(ctx, oracle, dtype, False)
    sr, opts, nodes, offs, ds, idxs = f["sr"], f["opts"], f["nodes"], f["offs"], f["ds"], f["idxs"]
    want = _as_triples(f["l"], f["g"], f["ok"])
    rev = list(range(NTREES))[::-1]
    rn = np.concatenate([nodes[offs[t]:offs[t + 1]] for t in rev])
    ro = np.concatenate([[0], np.cumsum([offs[t + 1] - offs[t] for t in rev])]).astype(np.int64)
    p = sr.Program(ctx, rn, ro, opts, dtype)
    l, g, ok = p.eval_loss_grad_rowsets(ds, sr.L2DistLoss(), [idxs[t] for t in rev])
    p.close()
    got = _as_triples(l, g, ok)
    assert [got[NTREES - 1 - t] for t in range(NTREES)] == [want[t] for t in range(NTREES)]
    # a tree alone with its set: lengths 1, 2, 50, 256, 257, 1025, 2049
    for t in (0, 1, 2, 6, 7, 9, 10):
        p = _one_tree(sr, ctx, nodes, offs, t, opts, dtype)
        l, g, ok = p.eval_loss_grad_rowsets(ds, sr.L2DistLoss(), [idxs[t]])
        p.close()
        assert _as_triples(l, g, ok)[0] == want[t], (t, len(idxs[t]))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_near_overflow_trees_are_settled(ctx, oracle, dtype):
    """tests/test_gpu_rowsets.py's construction: c * x1 over positive x1 with the set's exact sum just
    below (ok) or just above (fail) the type's threshold -- every row finite, the fast bound undecided, so
    the item is settled by the precise pass on a view of its own set."""
    sr = _sr()
    opts = sr.Options(binary_operators=("*", "+"), unary_operators=("cos",))
    n = 1000
    rng = np.random.default_rng(17)
    x = rng.uniform(0.25, 1.0, n).astype(dtype)
    X = np.stack([x, rng.standard_normal(n).astype(dtype)])
    y = np.zeros(n, dtype=dtype)
    thr = 2.0 ** 128 - 2.0 ** 103 if dtype == np.float32 else float(np.finfo(np.float64).max)
    trees, idxs, expect = [], [], []
    for i in range(16):
        idx = rng.integers(0, n, size=50)
        idxs.append(idx)
        if i % 2 == 0:
            k = i // 2
            s = float(np.sum(x[idx].astype(np.longdouble)))
            rel = (1 - 2e-5 * (k + 1)) if k % 2 == 0 else (1 + 2e-5 * (k + 1))
            trees.append(sr.Node(1, sr.Node(val=dtype(thr / s * rel)), sr.Node(feature=1)))  # c * x1
            expect.append(k % 2 == 0)
        else:
            trees.append(sr.Node(2, sr.Node(feature=2), sr.Node(val=1.5)))
            expect.append(True)
    nodes, offs = sr.flatten(trees, opts, dtype)
    ds = sr.DeviceDataset(ctx, X, y)
    prog = sr.Program(ctx, nodes, offs, opts, dtype)
    ook = _oracle_ok(oracle, nodes, offs, opts, X, y, None, idxs)
    assert list(ook) == expect, "the fixture's near-threshold sums"
    single = _single_grads(sr, ctx, ds, nodes, offs, opts, dtype, sr.L2DistLoss(), idxs)
    for _ in range(2):
        l, g, ok = prog.eval_loss_grad_rowsets(ds, sr.L2DistLoss(), idxs)
        assert np.array_equal(ok, ook), np.nonzero(ok != ook)[0]
        assert [bool(o) for o in ok] == [single[t][2] for t in range(16)]
        assert _as_triples(l, g, ok) == single
    prog.close()


def _optim_problem(sr, dtype, ntrees=40, n=3000, seed=11, max_size=20):
    """tests/test_gpu_optim.py::_problem's generator."""
    opts = sr.Options(binary_operators=("+", "-", "*", "/"), unary_operators=("cos", "exp", "sin"))
    trees = sr.random_population(ntrees, opts, 3, dtype, seed=seed, max_size=max_size)
    nodes, offs = sr.flatten(trees, opts, dtype)
    rng = np.random.default_rng(seed + 1)
    X = rng.standard_normal((3, n)).astype(dtype)
    y = (np.cos(1.3 * X[0]) * 2.0 + X[1] * 0.7 - 0.3).astype(dtype)
    return opts, trees, nodes, offs, X, y


def _optim_loop(sr, ctx, ds, nodes, offs, opts, dtype, loss, idxs, seeds, which, **kw):
    """The loop the one call replaces: one-tree optimize_constants(idx=set_t, seed=seeds[t])."""
    out = {}
    for t in which:
        p = _one_tree(sr, ctx, nodes, offs, t, opts, dtype)
        l, imp, fc, st = p.optimize_constants(ds, loss, idx=idxs[t], seed=seeds[t], return_starts=True, **kw)
        out[t] = (_bits(l)[0], bool(imp[0]), int(fc[0]), _bits(p.get_constants()[0]).tolist(), _bits(st).ravel().tolist())
        p.close()
    return out


def _optim_rowsets(prog, ds, loss, idxs, seeds, which=None, starts=None, **kw):
    l, imp, fc, st = prog.optimize_constants_rowsets(ds, loss, idxs, seeds=seeds, starts=starts, return_starts=True, **kw)
    consts = prog.get_constants()
    co = np.concatenate([[0], np.cumsum([len(c) for c in consts])]).astype(int)
    got = {t: (_bits(l[t:t + 1])[0], bool(imp[t]), int(fc[t]), _bits(consts[t]).tolist(),
               _bits(st[:, co[t]:co[t + 1]]).ravel().tolist()) for t in (range(len(consts)) if which is None else which)}
    return got, st


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_optimizer_parity_with_the_one_tree_loop(ctx, dtype):
    sr = _sr()
    opts, _, nodes, offs, X, y = _optim_problem(sr, dtype)
    nt = len(offs) - 1
    rng = np.random.default_rng(23)
    lens = [50] * nt
    for t, m in zip((3, 11, 19, 27, 35), (1, 256, 257, 1025, 2049)):
        lens[t] = m
    idxs = [rng.integers(0, X.shape[1], size=m) for m in lens]
    seeds = [int(s) for s in rng.integers(0, 2 ** 63 - 1, size=nt)]
    ds = sr.DeviceDataset(ctx, X, y)
    loss = sr.L2DistLoss()
    kw = dict(iterations=8, nrestarts=2)
    want = _optim_loop(sr, ctx, ds, nodes, offs, opts, dtype, loss, idxs, seeds, range(nt), **kw)
    prog = sr.Program(ctx, nodes, offs, opts, dtype)
    nconst = prog.num_constants()
    got, starts = _optim_rowsets(prog, ds, loss, idxs, seeds, **kw)
    prog.close()
    for t in range(nt):
        assert got[t] == want[t], (t, lens[t], int(nconst[t]), got[t][:3], want[t][:3])
    one, many, none = np.nonzero(nconst == 1)[0], np.nonzero(nconst >= 2)[0], np.nonzero(nconst == 0)[0]
    assert len(one) >= 3 and len(many) >= 10 and len(none) >= 1, (len(one), len(many), len(none))
    assert any(got[t][1] for t in one) and any(got[t][1] for t in many)
    assert all(got[t][2] == 0 and not got[t][1] for t in none)
    # the returned starts given back, other seeds: the same bits
    prog = sr.Program(ctx, nodes, offs, opts, dtype)
    again, _ = _optim_rowsets(prog, ds, loss, idxs, [s ^ 0x5A5A for s in seeds], starts=starts, **kw)
    prog.close()
    assert again == got


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_one_call_crosses_every_kind_of_tree(ctx, dtype):
    """One optimize_constants_rowsets call whose program holds every kind of tree the call's shared steps
    (starts, acceptance, the one-tree path, install, re-score, fcalls) treat differently: staged sets (one
    row, a sub-tile set, two blocks; BFGS and Newton), a set over every cap (2049 rows: the one-tree
    path), a tree without constants and a tree that fails statically (a non-finite constant leaf).
    Constants, loss, improved and fcalls equal, bit for bit, the per-tree optimize_constants calls with
    the same seeds and starts."""
    sr = _sr()
    opts = sr.Options(binary_operators=("+", "-", "*", "/"), unary_operators=("cos", "exp"))
    N_ = sr.Node
    n = 4096
    rng = np.random.default_rng(41)
    X = rng.standard_normal((5, n)).astype(dtype)
    y = (np.cos(1.3 * X[1]) * 2.0 + X[0] * 0.7 - 0.3).astype(dtype)
    trees = [N_(val=0.5) * N_("x1") + N_(val=0.1),                                        # BFGS, staged
             N_("cos", N_(val=1.1) * N_("x2")),                                           # Newton, over every cap
             N_("x1") + N_("x3"),                                                         # no constants
             N_("x1") * N_(val=np.inf),                                                   # fails statically
             N_("cos", N_(val=1.2) * N_("x2")) * N_(val=1.5) + N_(val=0.6) * N_("x1") - N_(val=0.2),  # BFGS, two blocks
             N_(val=0.3) * N_("x5")]                                                      # Newton, one row
    lens = [50, 2049, 50, 50, 257, 1]
    nt = len(trees)
    nodes, offs = sr.flatten(trees, opts, dtype)
    idxs = [rng.integers(0, n, size=m) for m in lens]
    seeds = [int(s) for s in rng.integers(0, 2 ** 63 - 1, size=nt)]
    ds = sr.DeviceDataset(ctx, X, y)
    loss = sr.L2DistLoss()
    kw = dict(iterations=3, nrestarts=1)
    want = _optim_loop(sr, ctx, ds, nodes, offs, opts, dtype, loss, idxs, seeds, range(nt), **kw)
    prog = sr.Program(ctx, nodes, offs, opts, dtype)
    nconst = prog.num_constants()
    assert list(nconst) == [2, 1, 0, 1, 4, 1]
    got, starts = _optim_rowsets(prog, ds, loss, idxs, seeds, **kw)
    prog.close()
    for t in range(nt):
        assert got[t] == want[t], (t, lens[t], got[t][:3], want[t][:3])
    # every kind did what it is there for: the optimised trees improved, the other two were left alone
    assert all(got[t][1] and got[t][2] > 0 for t in (0, 1, 4)), [got[t][1:3] for t in range(nt)]
    assert all(got[t][2] == 0 and not got[t][1] for t in (2, 3))
    assert got[3][0] == _bits(np.array([np.inf]))[0] and got[3][3] == _bits(np.array([np.inf])).tolist()
    # the same starts given to both sides explicitly, other seeds: the same bits again
    co = np.concatenate([[0], np.cumsum(nconst)]).astype(int)
    want2 = {}
    for t in range(nt):
        p = _one_tree(sr, ctx, nodes, offs, t, opts, dtype)
        l, imp, fc = p.optimize_constants(ds, loss, idx=idxs[t], seed=seeds[t] ^ 0x33, starts=starts[:, co[t]:co[t + 1]], **kw)
        want2[t] = (_bits(l)[0], bool(imp[0]), int(fc[0]), _bits(p.get_constants()[0]).tolist())
        p.close()
    prog = sr.Program(ctx, nodes, offs, opts, dtype)
    again, _ = _optim_rowsets(prog, ds, loss, idxs, [s ^ 0x5A5A for s in seeds], starts=starts, **kw)
    prog.close()
    assert again == got
    assert {t: again[t][:4] for t in range(nt)} == want2


@pytest.mark.parametrize("kind_name,args", [("HuberLoss", (0.7,)), ("LogitMarginLoss", ())])
def test_loss_kinds(ctx, kind_name, args):
    sr = _sr()
    loss = getattr(sr, kind_name)(*args)
    opts = _opts(sr)
    rng = np.random.default_rng(302)
    X = rng.standard_normal((4, 1500))
    y = rng.standard_normal(1500)
    if isinstance(loss, sr.MarginLoss):
        y = np.where(y > 0, 1.0, -1.0)
    w = np.abs(rng.standard_normal(1500))
    trees = sr.random_population(24, opts, 4, np.float64, 301, 12)
    idxs = [rng.integers(0, 1500, size=50) for _ in trees]
    nodes, offs = sr.flatten(trees, opts, np.float64)
    ds = sr.DeviceDataset(ctx, X, y, w)
    prog = sr.Program(ctx, nodes, offs, opts, np.float64)
    l, g, ok = prog.eval_loss_grad_rowsets(ds, loss, idxs)
    prog.close()
    single = _single_grads(sr, ctx, ds, nodes, offs, opts, np.float64, loss, idxs)
    assert _as_triples(l, g, ok) == single
    assert ok.sum() >= 12


def test_more_chunks_than_one_round_of_waves(ctx):
    """2048 trees on 50-row sets: more single-wave workgroups than the chip holds at once, so late
    workgroups start as earlier ones retire."""
    sr = _sr()
    opts = _opts(sr)
    ntrees = 2048
    rng = np.random.default_rng(202)
    X = rng.standard_normal((NFEAT, N)).astype(np.float32)
    y = rng.standard_normal(N).astype(np.float32)
    trees = sr.random_population(ntrees, opts, NFEAT, np.float32, 201, 20)
    idxs = [rng.integers(0, N, size=50) for _ in trees]
    seeds = [int(s) for s in rng.integers(0, 2 ** 63 - 1, size=ntrees)]
    nodes, offs = sr.flatten(trees, opts, np.float32)
    ds = sr.DeviceDataset(ctx, X, y)
    loss = sr.L2DistLoss()
    kw = dict(iterations=2, nrestarts=0)
    sample = sorted(int(t) for t in rng.choice(ntrees, size=32, replace=False))
    want = _optim_loop(sr, ctx, ds, nodes, offs, opts, np.float32, loss, idxs, seeds, sample, **kw)
    prog = sr.Program(ctx, nodes, offs, opts, np.float32)
    got, _ = _optim_rowsets(prog, ds, loss, idxs, seeds, which=sample, **kw)
    prog.close()
    assert got == want
    assert sum(got[t][1] for t in sample) >= 4


def test_validation(ctx, oracle):
    f = _fixture(ctx, oracle, np.float32, False)
    sr, ds, nodes, offs, opts = f["sr"], f["ds"], f["nodes"], f["offs"], f["opts"]
    prog = sr.Program(ctx, nodes, offs, opts, np.float32)
    lib = sr._lib.load()
    ls = sr.L2DistLoss().c_struct()
    nall = int(prog.num_constants().sum())
    opt = sr._lib.OptimOptions(2, 1, 5, 1e-8)
    P = sr._lib.ptr

    def grad(offsets, rows):
        offsets, rows = np.asarray(offsets, dtype=np.int64), np.asarray(rows, dtype=np.int64)
        out, g, ok = np.empty(NTREES), np.empty(nall), np.empty(NTREES, dtype=np.uint8)
        sr._lib.check(lib.srhip_eval_loss_grad_rowsets(ctx.handle, ds.handle, prog.handle, ctypes.byref(ls), P(offsets), P(rows),
                                                       P(out), P(g), P(ok)))
        return out, g, ok

    def optim(offsets, rows):
        offsets, rows = np.asarray(offsets, dtype=np.int64), np.asarray(rows, dtype=np.int64)
        out, imp, fc = np.empty(NTREES), np.empty(NTREES, dtype=np.uint8), np.empty(NTREES, dtype=np.int64)
        sr._lib.check(lib.srhip_optimize_constants_rowsets(ctx.handle, ds.handle, prog.handle, ctypes.byref(ls), P(offsets),
                                                           P(rows), ctypes.byref(opt), None, None, None, P(out), P(imp), P(fc)))
        return out, imp, fc

    good = np.arange(NTREES + 1) * 2
    rows = np.arange(2 * NTREES) % N
    before = _bits(np.concatenate(prog.get_constants()))
    for call in (grad, optim):
        for offsets, rr, what in ((np.where(np.arange(NTREES + 1) == 7, 11, good), rows, r"row_offsets\[7\] = 11 < row_offsets\[6\] = 12"),
                                  (np.where(np.arange(NTREES + 1) == 7, 12, good), rows, r"tree 6 has an empty row set"),
                                  (good, np.where(np.arange(2 * NTREES) == 21, N, rows), r"tree 10: .*position 1 of its set.* = 5000"),
                                  (good, np.where(np.arange(2 * NTREES) == 0, -1, rows), r"tree 0: .*= -1"),
                                  (good + 1, np.arange(2 * NTREES + 1) % N, r"row_offsets\[0\]")):
            with pytest.raises(sr.SrhipError, match=what) as e:
                call(offsets, rr)
            assert e.value.code == sr._lib.ERR_INVALID
    with pytest.raises(sr.SrhipError, match="null"):
        sr._lib.check(lib.srhip_eval_loss_grad_rowsets(ctx.handle, ds.handle, prog.handle, ctypes.byref(ls), None, None, None, None,
                                                       None))
    with pytest.raises(sr.SrhipError, match="null"):
        sr._lib.check(lib.srhip_optimize_constants_rowsets(ctx.handle, ds.handle, prog.handle, ctypes.byref(ls), None, None,
                                                           ctypes.byref(opt), None, None, None, None, None, None))
    assert np.array_equal(_bits(np.concatenate(prog.get_constants())), before)  # failed calls left the constants alone
    # Int32 programs: unsupported, as in the single-idx entry points
    iopts = sr.Options(binary_operators=("+", "*"), unary_operators=("neg",))
    inodes, ioffs = sr.flatten([sr.Node("x1") + sr.Node(val=2.0)], iopts, np.int32)
    ids = sr.DeviceDataset(ctx, np.arange(40, dtype=np.int32).reshape(2, 20), np.arange(20, dtype=np.int32))
    ip = sr.Program(ctx, inodes, ioffs, iopts, np.int32)
    for fn in (lambda: ip.eval_loss_grad_rowsets(ids, sr.L2DistLoss(), [np.arange(5)]),
               lambda: ip.optimize_constants_rowsets(ids, sr.L2DistLoss(), [np.arange(5)])):
        with pytest.raises(sr.SrhipError) as e:
            fn()
        assert e.value.code == sr._lib.ERR_UNSUPPORTED
    ip.close()
    # the same calls with good arguments succeed afterwards
    sets = [rows[2 * t:2 * t + 2] for t in range(NTREES)]
    out, g, ok = grad(good, rows)
    l2, g2, ok2 = prog.eval_loss_grad_rowsets(ds, sr.L2DistLoss(), sets)
    assert np.array_equal(_bits(out), _bits(l2)) and np.array_equal(_bits(g), _bits(_flat(g2))) and np.array_equal(ok.astype(bool), ok2)
    out, imp, fc = optim(good, rows)
    assert np.isfinite(out).sum() > NTREES // 2 and (fc >= 0).all()
    prog.close()


def test_api_batching_list_is_one_call_with_the_loops_bits(ctx, monkeypatch):
    """sr.optimize_constants in batching mode on a member list: the loop it replaces, restated by hand with
    a twin generator (all subsets first, then all seeds, then one one-tree device call per member and the
    member bookkeeping), member for member; and exactly one optimize_constants_rowsets call."""
    sr = _sr()
    from srhip.api import _ctx, batch_sample, compile_trees, loss_to_score
    from srhip.node import set_constants

    opts = sr.Options(binary_operators=("+", "-", "*", "/"), unary_operators=("cos", "exp"), batching=True, batch_size=50)
    rng = np.random.default_rng(502)
    X = rng.standard_normal((NFEAT, N)).astype(np.float32)
    ds = sr.Dataset(X, (2 * np.cos(X[3]) + X[0] ** 2 - 2).astype(np.float32))
    sr.update_baseline_loss(ds, opts)

    class Member:
        def __init__(self, tree):
            self.tree, self.loss, self.score, self.birth = tree, np.float32(0), np.float32(0), 0

    pop = sr.random_population(30, opts, NFEAT, np.float32, 501, 20)
    ma = [Member(t.copy()) for t in pop]
    mb = [Member(t.copy()) for t in pop]
    calls = []
    orig = sr.Program.optimize_constants_rowsets
    monkeypatch.setattr(sr.Program, "optimize_constants_rowsets",
                        lambda self, *a, **k: (calls.append(self.ntrees), orig(self, *a, **k))[1], raising=False)
    ra, rb = np.random.default_rng(7), np.random.default_rng(7)
    _, evals_a = sr.optimize_constants(ds, ma, opts, rng=ra)
    # the hand-written loop
    L = ds.loss_type.type
    subsets = [batch_sample(ds, opts, rb) for _ in mb]
    seeds = [int(rb.integers(0, 2 ** 63 - 1)) for _ in mb]
    evals_b = 0.0
    for m, idx, seed in zip(mb, subsets, seeds):
        prog = compile_trees([m.tree], opts, ds.X.dtype)
        losses, improved, fcalls = prog.optimize_constants(ds.device(_ctx(opts)), opts.elementwise_loss,
                                                           iterations=opts.optimizer_iterations,
                                                           nrestarts=opts.optimizer_nrestarts, seed=seed, idx=idx)
        consts = prog.get_constants()
        prog.close()
        evals_b += float(fcalls[0]) * (opts.batch_size / ds.n)
        if not improved[0]:
            continue
        set_constants(m.tree, consts[0])
        m.loss = L(losses[0])
        m.score = loss_to_score(m.loss, ds.use_baseline, ds.baseline_loss, m, opts)
    for a, b in zip(ma, mb):
        assert _bits(sr.get_constants(a.tree)).tolist() == _bits(sr.get_constants(b.tree)).tolist()
        assert (float(a.loss), float(a.score)) == (float(b.loss), float(b.score))
    assert evals_a == evals_b and evals_a > 0
    assert ra.integers(0, 1 << 30) == rb.integers(0, 1 << 30)
    assert calls == [30], calls
